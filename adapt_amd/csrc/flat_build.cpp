// flat_build.cpp — host side of the flat sweep (traverse.hpp "Flat sweep"): the scene's primitives as precomputed-transform records.
//
// Replaces, for small scenes in the fast build, the data the reference's brute-force intersector reads per ray: `prims` / `precom_vec`
// (tracer/tracer_base.py:117-134, 184-212).  Per planar primitive its corner p0 and the rows U, V, T of [e1 e2 n]^-1 (n = e1 x e2), so
// that for a point x:  u = U . (x - p0), v = V . (x - p0), height over the plane = T . (x - p0)
// (Baldwin & Weber, "Fast Ray-Triangle Intersections by Coordinate Transformation", JCGT 5(3), 2016).  Computed in double, stored as
// float.  Two coplanar triangles of one object that share an edge and form a convex outline become ONE record in the basis (corner opposite
// the shared edge, edge, edge): a parallelogram (inside <=> u, v in [0, 1]) or a general convex quadrilateral (u, v >= 0 and two more edge
// functions of (u, v)); which triangle a hit belongs to is u + v <= 1, and each triangle's own barycentrics are an affine map of the
// record's (u, v) (coefficients in {-1, 0, 1} for a parallelogram).  Degenerate triangles get a record no ray can hit (upstream: det = 0 -> non-finite barycentrics -> never accepted).
#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>

#include "bvh_build.hpp"

namespace apt {
namespace {
struct D3 { double x, y, z; };
inline D3 sub(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline D3 add(D3 a, D3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline D3 cross(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline D3 vtx(const float* prims, int k, int v) { const float* p = prims + 9 * (size_t)k + 3 * v; return {p[0], p[1], p[2]}; }

struct Planar { float P0[3], U[4], V[4], T[4]; int prim_a, prim_b; float map_a[6], map_b[6]; bool ok; int obj; bool tie; float lo[3], hi[3]; float far_edges[6]; };

// rows of [e1 e2 n]^-1 applied to (x - p0)
bool make_rows(D3 p0, D3 e1, D3 e2, Planar& r) {
    const D3 n = cross(e1, e2);
    const double det = dot(n, n);
    if (!(det > 0.0) || !std::isfinite(det)) return false;
    const D3 ru = cross(e2, n), rv = cross(n, e1);
    const D3 U = {ru.x / det, ru.y / det, ru.z / det}, V = {rv.x / det, rv.y / det, rv.z / det};
    // t = -T(s) / T(d) does not depend on the scale or sign of the T row: store the plane in a canonical form - unit normal with its first
    // non-zero component positive, offset rounded once - so that COPLANAR primitives (a box resting on the floor, a decal on a wall) are
    // recognisable by bit-identical rows (T[3], the offset, serves only that comparison).  Their records go to the tie sections of the
    // stream, where the reference's own arithmetic settles which of two faces at the same distance is "hit" (traverse.hpp flat_tie_break).
    const double len = std::sqrt(det);
    D3 T = {n.x / len, n.y / len, n.z / len};
    auto snap = [](double a) { return std::fabs(a) < 1e-12 ? 0.0 : ((std::fabs(std::fabs(a) - 1.0) < 1e-12) ? std::copysign(1.0, a) : a); };
    T = {snap(T.x), snap(T.y), snap(T.z)};
    const double lead = (T.x != 0.0) ? T.x : ((T.y != 0.0) ? T.y : T.z);
    if (lead < 0.0) T = {-T.x, -T.y, -T.z};
    T = {T.x + 0.0, T.y + 0.0, T.z + 0.0};                                    // -0 -> +0: the rows are compared bit for bit
    T = {(double)(float)T.x, (double)(float)T.y, (double)(float)T.z};        // the stored normal; the offset below belongs to exactly these floats
    const double uw = -dot(U, p0), vw = -dot(V, p0), tw = -dot(T, p0) + 0.0;
    const double all[12] = {U.x, U.y, U.z, uw, V.x, V.y, V.z, vw, T.x, T.y, T.z, tw};
    for (double a : all) if (!std::isfinite(a) || std::fabs(a) > 1e30) return false;
    r.P0[0] = (float)p0.x; r.P0[1] = (float)p0.y; r.P0[2] = (float)p0.z;      // exact: p0 is one of the float32 vertices
    r.U[0] = (float)U.x; r.U[1] = (float)U.y; r.U[2] = (float)U.z; r.U[3] = (float)uw;
    r.V[0] = (float)V.x; r.V[1] = (float)V.y; r.V[2] = (float)V.z; r.V[3] = (float)vw;
    r.T[0] = (float)T.x; r.T[1] = (float)T.y; r.T[2] = (float)T.z; r.T[3] = (float)tw;
    return true;
}
// triangle k's own barycentrics as an affine map of the record's (u, v) - k lies in the record's plane, so the map is exact: evaluate
// k's barycentrics at the record's corner and edge ends.  (For a parallelogram half the coefficients come out in {-1, 0, 1}.)
bool bary_map(const float* prims, int k, D3 p0, D3 e1, D3 e2, float m[6]) {
    const D3 q0 = vtx(prims, k, 0), f1 = sub(vtx(prims, k, 1), q0), f2 = sub(vtx(prims, k, 2), q0);
    const D3 n = cross(f1, f2); const double det = dot(n, n);
    if (!(det > 0.0) || !std::isfinite(det)) return false;
    auto bary = [&](D3 x, double& a, double& b) { const D3 w = sub(x, q0); a = dot(cross(w, f2), n) / det; b = dot(cross(f1, w), n) / det; };
    double a0, b0, a1, b1, a2, b2;
    bary(p0, a0, b0); bary(add(p0, e1), a1, b1); bary(add(p0, e2), a2, b2);
    const double c[6] = {a0, a1 - a0, a2 - a0, b0, b1 - b0, b2 - b0};
    for (int i = 0; i < 6; i++) {
        const double r = std::nearbyint(c[i]);
        m[i] = (float)((std::fabs(c[i] - r) < 1e-9) ? r + 0.0 : c[i]);
    }
    return true;
}

// Do two convex polygons of one plane overlap with positive area?  Separating-axis test over the in-plane normals of both polygons'
// edges, with a margin: polygons that only share an edge or a corner (the two triangles of a non-parallelogram face) do not count.
typedef std::vector<D3> Poly;
bool convex_overlap(const Poly& A, const Poly& B, const float plane[4]) {
    const D3 n = {plane[0], plane[1], plane[2]};
    double ext = 0.0;
    for (const D3& p : A) for (const D3& q : A) ext = std::max(ext, std::sqrt(dot(sub(p, q), sub(p, q))));
    const double margin = 1e-5 * ext + 1e-9;
    for (int pass = 0; pass < 2; pass++) {
        const Poly& P = pass ? B : A;
        for (size_t i = 0; i < P.size(); i++) {
            const D3 e = sub(P[(i + 1) % P.size()], P[i]);
            D3 ax = cross(n, e);
            const double len = std::sqrt(dot(ax, ax));
            if (len < 1e-20) continue;
            ax = {ax.x / len, ax.y / len, ax.z / len};
            double a0 = 1e300, a1 = -1e300, b0 = 1e300, b1 = -1e300;
            for (const D3& p : A) { const double t = dot(ax, p); a0 = std::min(a0, t); a1 = std::max(a1, t); }
            for (const D3& p : B) { const double t = dot(ax, p); b0 = std::min(b0, t); b1 = std::max(b1, t); }
            if (std::min(a1, b1) - std::max(a0, b0) <= margin) return false;       // a separating axis (or mere contact)
        }
    }
    return true;
}
const int kRecordFloats[4] = {12, 18, 12, 4};      // stream floats per record: parallelogram, convex quad, triangle, sphere (layout: build_flat)
}  // namespace

// One triangle as the BVH walk of the product build reads it (traverse.hpp tri_two): corner p0, rows U, V, T of [e1 e2 n]^-1, 12 floats.
// A degenerate triangle gets all-zero rows: T . d = 0 -> t is NaN or inf -> never accepted (upstream: det = 0 -> NaN barycentrics).
void planar_rows(const float* tri9, float out12[12]) {
    const D3 p0 = {tri9[0], tri9[1], tri9[2]}, e1 = sub({tri9[3], tri9[4], tri9[5]}, p0), e2 = sub({tri9[6], tri9[7], tri9[8]}, p0);
    Planar r;
    for (int a = 0; a < 12; a++) out12[a] = 0.f;
    out12[0] = tri9[0]; out12[1] = tri9[1]; out12[2] = tri9[2];
    if (!make_rows(p0, e1, e2, r)) return;
    for (int a = 0; a < 3; a++) { out12[3 + a] = r.U[a]; out12[6 + a] = r.V[a]; out12[9 + a] = r.T[a]; }
}

// stream: [parallelograms][same, of coplanar groups] x 12 floats, [convex quads][same, of coplanar groups] x 18, [triangles][same, of
// coplanar groups] x 12, [spheres] x 4; a planar record = corner p0, rows U, V, T (3 floats each); a convex quad appends its two far
// edges as functions a u + b v + c of the record's (u, v) that are >= 0 inside.  tab: 28 floats per record, in stream order (7 float4: (U, p0.x), (V, p0.y), (prim_a, prim_b, class_a,
// class_b), map_a, map_b, (p0.z, -, -, -)).
// prim_class: material class per primitive (sorted shading) or null.
// A record joins a coplanar group when another record lies in the same plane (to 2e-5) and their outlines overlap - the configurations in
// which upstream's answer hangs on the last bit of two distances (traverse.hpp flat_tie_break): a glass box resting on the floor, a decal on a wall.
int build_flat(const float* prims, int n_prims, const int32_t* obj_info, int n_objects, const int32_t* prim_class,
               std::vector<float>& stream, std::vector<float>& tab, int counts[7]) {
    std::vector<Planar> quads, gquads, tris;
    std::vector<int> spheres;
    std::vector<uint8_t> used((size_t)n_prims, 0);
    const float ident[6] = {0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    auto bounds = [&](Planar& p) {
        for (int a = 0; a < 3; a++) { p.lo[a] = 1e30f; p.hi[a] = -1e30f; }
        for (int k : {p.prim_a, p.prim_b}) if (k >= 0) for (int v = 0; v < 3; v++) for (int a = 0; a < 3; a++) {
            const float x = prims[9 * (size_t)k + 3 * v + a]; p.lo[a] = std::min(p.lo[a], x); p.hi[a] = std::max(p.hi[a], x);
        }
    };
    for (int o = 0; o < n_objects; o++) {
        const int first = obj_info[3 * o], count = obj_info[3 * o + 1];
        if (first < 0 || count < 0 || first + count > n_prims) return -1;
        if (obj_info[3 * o + 2]) { for (int k = first; k < first + count; k++) spheres.push_back(k); continue; }
        for (int k = first; k < first + count; k++) {
            if (used[(size_t)k]) continue;
            used[(size_t)k] = 1;
            const D3 A = vtx(prims, k, 0), B = vtx(prims, k, 1), C = vtx(prims, k, 2);
            const double ext = std::sqrt(std::max(dot(sub(B, A), sub(B, A)), dot(sub(C, A), sub(C, A)))), tol = 1e-6 * ext + 1e-12;
            // a partner in the same object that shares an edge, lies in the same plane and makes a convex outline with this triangle.  In this
            // triangle's frame (corner = the vertex opposite the shared edge) the partner's third vertex sits at (ud, vd): (1, 1) closes a
            // parallelogram; any other point with ud > 0, vd > 0, ud + vd > 1 a convex quadrilateral.
            bool paired = false;
            const D3 tv[3] = {A, B, C};
            for (int k2 = k + 1; k2 < first + count && !paired; k2++) {
                if (used[(size_t)k2]) continue;
                const D3 w[3] = {vtx(prims, k2, 0), vtx(prims, k2, 1), vtx(prims, k2, 2)};
                for (int opp = 0; opp < 3 && !paired; opp++) {            // this triangle's vertex opposite the shared edge
                    const D3 s1 = tv[(opp + 1) % 3], s2 = tv[(opp + 2) % 3];
                    auto same = [&](D3 a, D3 b) { const D3 d = sub(a, b); return dot(d, d) <= tol * tol; };
                    int hit_s1 = -1, hit_s2 = -1;
                    for (int j = 0; j < 3; j++) { if (same(w[j], s1)) hit_s1 = j; else if (same(w[j], s2)) hit_s2 = j; }
                    if (hit_s1 < 0 || hit_s2 < 0 || hit_s1 == hit_s2) continue;
                    const D3 far = w[3 - hit_s1 - hit_s2];
                    const D3 p0 = tv[opp], e1 = sub(s1, p0), e2 = sub(s2, p0), n = cross(e1, e2);
                    const double det = dot(n, n);
                    if (!(det > 0.0)) continue;
                    const D3 fd = sub(far, p0);
                    if (std::fabs(dot(fd, n)) / std::sqrt(det) > tol) continue;                                  // not in this triangle's plane
                    const double ud = dot(cross(fd, e2), n) / det, vd = dot(cross(e1, fd), n) / det;
                    if (!(ud > 1e-4 && vd > 1e-4 && ud + vd > 1.0 + 1e-4)) continue;                             // the outline would not be convex
                    Planar q{}; q.prim_a = k; q.prim_b = k2; q.obj = o;
                    if (!make_rows(p0, e1, e2, q)) continue;
                    if (!bary_map(prims, k, p0, e1, e2, q.map_a) || !bary_map(prims, k2, p0, e1, e2, q.map_b)) continue;
                    q.ok = true; bounds(q); used[(size_t)k2] = 1; paired = true;
                    if (std::fabs(ud - 1.0) <= 1e-6 && std::fabs(vd - 1.0) <= 1e-6) { quads.push_back(q); break; }
                    // the far edges (1, 0) -> (ud, vd) and (ud, vd) -> (0, 1) as functions that are >= 0 inside
                    const double fe[6] = {-vd, ud - 1.0, vd, vd - 1.0, -ud, ud};
                    for (int i = 0; i < 6; i++) q.far_edges[i] = (float)fe[i];
                    gquads.push_back(q);
                }
            }
            if (paired) continue;
            Planar t{}; t.prim_a = k; t.prim_b = -1; t.obj = o; memcpy(t.map_a, ident, sizeof(ident)); memcpy(t.map_b, ident, sizeof(ident));
            t.ok = make_rows(A, sub(B, A), sub(C, A), t);
            bounds(t);
            tris.push_back(t);
        }
    }
    auto poly = [&](const Planar& p) {                      // the record's outline: triangle, or parallelogram corner, corner + e1, far corner, corner + e2
        Poly out;
        if (p.prim_b < 0) { for (int v = 0; v < 3; v++) out.push_back(vtx(prims, p.prim_a, v)); return out; }
        // the four distinct vertices of the two triangles, ordered around the centroid
        std::vector<D3> pts;
        for (int k : {p.prim_a, p.prim_b}) for (int v = 0; v < 3; v++) {
            const D3 x = vtx(prims, k, v); bool dup = false;
            for (const D3& y : pts) { const D3 dd = sub(x, y); if (dot(dd, dd) < 1e-12 * (1.0 + dot(x, x))) dup = true; }
            if (!dup) pts.push_back(x);
        }
        D3 c = {0, 0, 0}; for (const D3& x : pts) c = add(c, x); c = {c.x / pts.size(), c.y / pts.size(), c.z / pts.size()};
        const D3 n = {p.T[0], p.T[1], p.T[2]}, ref = sub(pts[0], c);
        std::vector<std::pair<double, int>> ang;
        for (size_t i = 0; i < pts.size(); i++) { const D3 r = sub(pts[i], c); ang.push_back({std::atan2(dot(cross(ref, r), n), dot(ref, r)), (int)i}); }
        std::sort(ang.begin(), ang.end());
        for (auto& a : ang) out.push_back(pts[(size_t)a.second]);
        return out;
    };
    {   // coplanar groups
        std::vector<Planar*> all;
        for (Planar& p : quads) all.push_back(&p);
        for (Planar& p : gquads) all.push_back(&p);
        for (Planar& p : tris) all.push_back(&p);
        for (size_t i = 0; i < all.size(); i++) for (size_t j = i + 1; j < all.size(); j++) {
            Planar &a = *all[i], &b = *all[j];
            if (!a.ok || !b.ok) continue;
            // the same plane up to what a ray can tell apart: the tie sections accept candidates within 1e-5 t + 1e-6 of each other, so planes
            // a few 1e-5 apart (a box "on" the floor whose transformed vertices sit at y = 1e-16) have to be in them
            bool same_plane = std::fabs((double)a.T[3] - (double)b.T[3]) <= 2e-5 * (1.0 + std::fabs((double)a.T[3]));
            for (int c = 0; c < 3; c++) if (std::fabs((double)a.T[c] - (double)b.T[c]) > 1e-5) same_plane = false;
            if (!same_plane) continue;
            // (opaque pairs too: a decal on a wall is coplanar geometry seen from outside, and upstream's picture of it is decided by the same last bits)
            bool overlap = convex_overlap(poly(a), poly(b), a.T);
            if (overlap) { a.tie = true; b.tie = true; }
        }
    }
    auto split = [](std::vector<Planar>& v) {               // stable: plain records first, coplanar-group records after, scene order inside each
        std::vector<Planar> plain, tie;
        for (const Planar& p : v) (p.tie ? tie : plain).push_back(p);
        const int n_tie = (int)tie.size();
        v = plain; v.insert(v.end(), tie.begin(), tie.end());
        return n_tie;
    };
    const int nq_tie = split(quads), ng_tie = split(gquads), nt_tie = split(tris);
    counts[0] = (int)quads.size() - nq_tie; counts[1] = nq_tie; counts[2] = (int)gquads.size() - ng_tie; counts[3] = ng_tie;
    counts[4] = (int)tris.size() - nt_tie; counts[5] = nt_tie; counts[6] = (int)spheres.size();
    const int n_quads = (int)quads.size(), n_gquads = (int)gquads.size(), n_tris = (int)tris.size(), n_spheres = (int)spheres.size();
    stream.assign((size_t)n_quads * kRecordFloats[0] + (size_t)n_gquads * kRecordFloats[1] + (size_t)n_tris * kRecordFloats[2] + (size_t)n_spheres * kRecordFloats[3] + 4, 0.f);
    tab.assign((size_t)(n_quads + n_gquads + n_tris + n_spheres) * 28, 0.f);
    size_t at = 0, rec = 0;
    auto cls_of = [&](int k) -> int32_t { return (prim_class && k >= 0) ? prim_class[k] : -1; };
    auto put_planar = [&](const std::vector<Planar>& v, int stride) {
        for (const Planar& p : v) {
            float* r = stream.data() + at;
            float* e = tab.data() + 28 * rec;
            int32_t ids[4] = {p.prim_a, p.ok ? p.prim_b : -1, cls_of(p.prim_a), cls_of(p.prim_b)};
            if (p.ok) {
                for (int c = 0; c < 3; c++) { r[c] = p.P0[c]; r[3 + c] = p.U[c]; r[6 + c] = p.V[c]; r[9 + c] = p.T[c]; e[c] = p.U[c]; e[4 + c] = p.V[c]; }
                e[3] = p.P0[0]; e[7] = p.P0[1]; e[24] = p.P0[2];
                memcpy(e + 12, p.map_a, 24); memcpy(e + 18, p.map_b, 24);
                if (stride == kRecordFloats[1]) memcpy(r + 12, p.far_edges, 24);
            }                                                    // a degenerate triangle keeps its slot with all-zero rows: t = -0 / 0 = NaN, which no comparison accepts
            memcpy(e + 8, ids, 16);
            at += (size_t)stride; rec++;
        }
    };
    put_planar(quads, kRecordFloats[0]);
    put_planar(gquads, kRecordFloats[1]);
    put_planar(tris, kRecordFloats[2]);
    for (int k : spheres) {
        float* r = stream.data() + at;
        float* e = tab.data() + 28 * rec;
        const float* p = prims + 9 * (size_t)k;
        r[0] = p[0]; r[1] = p[1]; r[2] = p[2]; r[3] = p[3] * p[3];               // radius2 = r ** 2 in float32 (tracer_base.py:186)
        int32_t ids[4] = {k, -1, cls_of(k), -1};
        memcpy(e + 8, ids, 16);
        memcpy(e + 12, ident, 24); memcpy(e + 18, ident, 24);
        at += kRecordFloats[3]; rec++;
    }
    return 0;
}

// The stream two records at a time, for the one-ray any-hit sweep (traverse.hpp FlatScene::pairs): in each section the floats of records
// 2j and 2j + 1 interleaved; an odd tail repeats its record.
std::vector<float> flat_pairs(const std::vector<float>& stream, const int counts[7]) {
    const int n[4] = {counts[0] + counts[1], counts[2] + counts[3], counts[4] + counts[5], counts[6]};
    std::vector<float> out;
    const float* src = stream.data();
    for (int sec = 0; sec < 4; src += (size_t)n[sec] * kRecordFloats[sec], sec++)
        for (int j = 0, w = kRecordFloats[sec]; 2 * j < n[sec]; j++) {
            const float* a = src + (size_t)(2 * j) * w; const float* b = (2 * j + 1 < n[sec]) ? a + w : a;
            for (int k = 0; k < w; k++) { out.push_back(a[k]); out.push_back(b[k]); }
        }
    if (out.empty()) out.push_back(0.f);
    return out;
}

// The points an emitter's light samples aim at (shading.hpp emitter_sample_hit): point and spot lights their position, an area light on a
// mesh every vertex of the mesh (a sample is a convex combination of them), an area light on a sphere the sphere's box, padded.  Any other
// emitter gets no points - and with them the full stream.
void emitter_points(const float* prims, const int32_t* obj_info, int n_objects, const int32_t* src_i, const float* src_f, int n_sources,
                    std::vector<float>& pts, std::vector<int32_t>& off) {
    pts.clear(); off.assign(1, 0);
    for (int e = 0; e < n_sources; e++) {
        const int type = src_i[4 * e], obj = src_i[4 * e + 2];
        const float* pos = src_f + 11 * e + 6;
        if (type == 0 || type == 2) pts.insert(pts.end(), pos, pos + 3);
        else if (type == 1 && obj >= 0 && obj < n_objects) {
            const int first = obj_info[3 * obj], count = obj_info[3 * obj + 1];
            if (obj_info[3 * obj + 2]) {
                const float* c = prims + 9 * (size_t)first; const double r = std::fabs((double)c[3]) * (1.0 + 1e-3) + 1e-6 * (1.0 + std::fabs((double)c[0]) + std::fabs((double)c[1]) + std::fabs((double)c[2]));
                for (int k = 0; k < 8; k++) for (int a = 0; a < 3; a++) pts.push_back((float)((double)c[a] + (((k >> a) & 1) ? r : -r)));
            } else for (int k = first; k < first + count; k++) pts.insert(pts.end(), prims + 9 * (size_t)k, prims + 9 * (size_t)k + 9);
        }
        off.push_back((int32_t)(pts.size() / 3));
    }
}

// Which records can block a light sample (traverse.hpp flat_any1).  A record R blocks a shadow ray only where
// flat_blocks() accepts it: inside R, t > 1e-4, t < dist - 1e-4.  h(x) = T . (x - p0) is the height over R's plane exactly as the
// kernel computes it (its stored rows), oriented so that the emitter's points are on the positive side, at height >= delta > 0.  If every
// vertex of the scene (and every sphere's padded box) is at height >= h_min, every shadow-ray origin - a hit point on some record S, off S
// by the rounding of its intersector - is at height >= h_min - eta, and h is affine along the ray, so the segment from an origin to the
// light crosses R's plane at most once, at t <= (eta - h_min) maxdist / delta (maxdist: the farthest light point from any vertex), and
// nowhere if the origin is above the plane.  The kernel's own t adds its rounding (e_o below).  If that bound stays below HALF the 1e-4
// floor, R can only ever be "hit" as a self-intersection that flat_blocks() already rejects: R is left out of the emitter's list.
// Rounding, with u = 2^-24, ext = the extent of scene and lights per axis, L = |ext|, M = the largest |coordinate| per axis:
//  * height of a hit point x over its own record S's plane (planar_solve: t = -T.s * rcp(T.d), s = o - p0 and the products rounded, the
//    rcp within 1 ulp, |t| <= L):  7 u sum|T_S| ext + 3 u L;
//  * how far outside S's outline the inside test may accept x: an edge function g = a u + b v + c, with u, v from U . P, V . P at
//    P = fma(t, d, s), is off by 5 u (|a| sum|U| ext + |b| sum|V| ext) - divided by |a U + b V| a distance in the plane;
//  * x itself, d * t + o rounded per component: u (L + |M|);
//  * R's own t: T_R . s to 4 u sum|T_R| ext, T_R . d >= delta / maxdist.
// The reference-order code that serves the rare deferred rays (prim_test, sweep) rounds its hit points to the same order; the factor 2 of
// the floor covers it.  Spheres keep their records (their hit points enter through their padded boxes).
int flat_occluders(const float* prims, int n_prims, const std::vector<float>& stream, const std::vector<float>& tab, const int counts[7],
                   const float* pts, const int32_t* off, int n_emit, bool cull, std::vector<float>& pairs, std::vector<int32_t>& table, std::vector<uint8_t>& keep) {
    const double u = std::ldexp(1.0, -24);
    const int nsec[4] = {counts[0] + counts[1], counts[2] + counts[3], counts[4] + counts[5], counts[6]};
    const int n_rec = nsec[0] + nsec[1] + nsec[2] + nsec[3];
    struct Rec { int sec; size_t at; std::vector<D3> vs; };
    std::vector<Rec> recs;
    std::vector<D3> geo;                                    // every vertex of the scene, every sphere's padded box
    {
        size_t at = 0;
        for (int sec = 0, r = 0; sec < 4; sec++) for (int j = 0; j < nsec[sec]; j++, r++, at += (size_t)kRecordFloats[sec]) {
            int32_t ids[2]; memcpy(ids, tab.data() + 28 * (size_t)r + 8, 8);
            Rec rc; rc.sec = sec; rc.at = at;
            if (ids[0] < 0 || ids[0] >= n_prims || ids[1] >= n_prims) return -1;
            if (sec < 3) { for (int k : {ids[0], ids[1]}) if (k >= 0) for (int v = 0; v < 3; v++) rc.vs.push_back(vtx(prims, k, v)); }
            else {
                const float* c = prims + 9 * (size_t)ids[0];
                const double rr = std::fabs((double)c[3]);
                // a grazing sphere hit is off by up to ~sqrt(u) L along the ray (a difference of squares): pad the box by more than that
                const double pad = 1e-3 * rr + 1e-6 * (1.0 + std::fabs((double)c[0]) + std::fabs((double)c[1]) + std::fabs((double)c[2])) + 1e-3;
                for (int k = 0; k < 8; k++) rc.vs.push_back({c[0] + (((k >> 0) & 1) ? rr + pad : -rr - pad), c[1] + (((k >> 1) & 1) ? rr + pad : -rr - pad), c[2] + (((k >> 2) & 1) ? rr + pad : -rr - pad)});
            }
            geo.insert(geo.end(), rc.vs.begin(), rc.vs.end());
            recs.push_back(rc);
        }
    }
    const int n_pts = n_emit > 0 ? off[n_emit] : 0;
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300}, M[3] = {0, 0, 0};
    auto grow = [&](D3 p) { const double c[3] = {p.x, p.y, p.z}; for (int a = 0; a < 3; a++) { lo[a] = std::min(lo[a], c[a]); hi[a] = std::max(hi[a], c[a]); M[a] = std::max(M[a], std::fabs(c[a])); } };
    for (const D3& p : geo) grow(p);
    for (int k = 0; k < n_pts; k++) grow({pts[3 * k], pts[3 * k + 1], pts[3 * k + 2]});
    const D3 ext = {hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]};
    const double L = std::sqrt(dot(ext, ext)), Mn = std::sqrt(M[0] * M[0] + M[1] * M[1] + M[2] * M[2]);
    auto absdot = [](D3 a, D3 b) { return std::fabs(a.x) * b.x + std::fabs(a.y) * b.y + std::fabs(a.z) * b.z; };
    auto row = [&](const Rec& r, int k) -> D3 { const float* p = stream.data() + r.at + 3 * k; return {p[0], p[1], p[2]}; };      // k: 0 p0, 1 U, 2 V, 3 T
    // eta: how far below the outline of the record it lies on a shadow-ray origin can be, the worst over all planar records
    double eta = 0.0;
    for (const Rec& r : recs) {
        if (r.sec == 3) continue;
        const D3 U = row(r, 1), V = row(r, 2), T = row(r, 3);
        if (dot(T, T) == 0.0) continue;                          // a degenerate triangle: never hit, never an origin
        std::vector<std::array<double, 2>> edges = {{1, 0}, {0, 1}};
        if (r.sec == 2) edges.push_back({1, 1});               // w = 1 - u - v (a parallelogram's u = 1, v = 1 have the gradients of u, v)
        if (r.sec == 1) for (int e = 0; e < 2; e++) { const float* f = stream.data() + r.at + 12 + 3 * e; edges.push_back({f[0], f[1]}); }
        double ovs = 0.0;
        for (const auto& g : edges) {
            const D3 grad = add({g[0] * U.x, g[0] * U.y, g[0] * U.z}, {g[1] * V.x, g[1] * V.y, g[1] * V.z});
            const double gl = std::sqrt(dot(grad, grad));
            if (!(gl > 0.0)) return -1;
            ovs = std::max(ovs, 5.0 * u * (std::fabs(g[0]) * absdot(U, ext) + std::fabs(g[1]) * absdot(V, ext)) / gl);
        }
        eta = std::max(eta, 7.0 * u * absdot(T, ext) / std::sqrt(dot(T, T)) + 3.0 * u * L + ovs);
    }
    eta += u * (L + Mn);
    keep.assign((size_t)n_emit * (size_t)n_rec, 1);
    pairs.clear(); table.assign((size_t)n_emit * 8, 0);
    for (int e = 0; e < n_emit; e++) {
        uint8_t* kp = keep.data() + (size_t)e * n_rec;
        const int p0 = off[e], p1 = off[e + 1];
        if (cull && p1 > p0) for (int ri = 0; ri < n_rec; ri++) {
            const Rec& r = recs[(size_t)ri];
            if (r.sec == 3) continue;
            const D3 P = row(r, 0), T = row(r, 3);
            if (dot(T, T) == 0.0) continue;
            auto h = [&](D3 x) { return dot(T, sub(x, P)); };
            double lmin = 1e300, lmax = -1e300;
            for (int k = p0; k < p1; k++) { const double v = h({pts[3 * k], pts[3 * k + 1], pts[3 * k + 2]}); lmin = std::min(lmin, v); lmax = std::max(lmax, v); }
            const double sgn = lmin > 0.0 ? 1.0 : (lmax < 0.0 ? -1.0 : 0.0);
            if (sgn == 0.0) continue;                            // the emitter straddles (or touches) R's plane
            const double delta = (sgn > 0 ? lmin : -lmax) - 4.0 * u * Mn;      // (an area-light sample is a rounded combination of its vertices)
            double hmin = 1e300, maxdist = 0.0;
            for (const D3& g : geo) hmin = std::min(hmin, sgn * h(g));
            for (int k = p0; k < p1; k++) for (const D3& g : geo) { const D3 dd = sub({pts[3 * k], pts[3 * k + 1], pts[3 * k + 2]}, g); maxdist = std::max(maxdist, std::sqrt(dot(dd, dd))); }
            const double e_o = 4.0 * u * absdot(T, ext);
            const double reach = (std::max(0.0, -hmin) + eta + e_o) * (maxdist + eta) / delta * (1.0 + 1e-3);
            if (delta > 0.0 && reach <= 0.5e-4) kp[ri] = 0;
        }
        // the kept records, sections as in the stream (coplanar-group records inside their sections), two by two
        std::vector<float> st; int c[7] = {0, 0, 0, 0, 0, 0, 0};
        for (int ri = 0; ri < n_rec; ri++) if (kp[ri]) {
            const Rec& r = recs[(size_t)ri];
            st.insert(st.end(), stream.begin() + (long)r.at, stream.begin() + (long)(r.at + (size_t)kRecordFloats[r.sec]));
            c[2 * r.sec]++;
        }
        int32_t* t = table.data() + 8 * (size_t)e;
        t[0] = (int32_t)pairs.size(); t[1] = c[0]; t[2] = c[2]; t[3] = c[4]; t[4] = c[6];
        std::vector<float> pr = flat_pairs(st, c);
        pairs.insert(pairs.end(), pr.begin(), pr.end());
    }
    if (pairs.empty()) pairs.push_back(0.f);
    return 0;
}

namespace {
// The pyramid of block b (local pixels 64 b .. 64 b + 63) for camera_strips and light_strips below: the inward unit normals of the four
// side planes through cam_t and the image-plane rectangle the block's pixels span, widened by `widen` pixels.  false: a singular camera matrix.
double strip_widen(const CamFilm& cf) { return 64.0 * std::ldexp(1.0, -24) * ((double)cf.width + (double)cf.height + 1.0 / std::fabs((double)cf.inv_focal)); }
bool strip_pyramid(const CamFilm& cf, int npix, int b, double widen, D3 n[4]) {
    auto world = [&](double x, double y) -> D3 {
        const float* R = cf.cam_r;
        return {R[0] * x + R[1] * y + R[2], R[3] * x + R[4] * y + R[5], R[6] * x + R[7] * y + R[8]};
    };
    int i0 = 1 << 30, i1 = -(1 << 30), j0 = 1 << 30, j1 = -(1 << 30);
    for (int lp = 64 * b; lp < std::min(npix, 64 * b + 64); lp++) {      // local_to_global (stages.hpp)
        const int lc = lp / cf.height, j = lp % cf.height, i = (lc / cf.band_width * cf.world + cf.rank) * cf.band_width + lc % cf.band_width;
        i0 = std::min(i0, i); i1 = std::max(i1, i); j0 = std::min(j0, j); j1 = std::max(j1, j);
    }
    // image-plane rectangle of the block: x = (half_w + vx - i) inv_focal, y = (j - half_h - vy) inv_focal, vx, vy in [0, 1]
    const double f = cf.inv_focal;
    double xa = ((double)cf.half_w - i1 - widen) * f, xb = ((double)cf.half_w + 1.0 - i0 + widen) * f;
    double ya = ((double)j0 - cf.half_h - 1.0 - widen) * f, yb = ((double)j1 - cf.half_h + widen) * f;
    if (xa > xb) std::swap(xa, xb);
    if (ya > yb) std::swap(ya, yb);
    const D3 c[4] = {world(xa, ya), world(xb, ya), world(xb, yb), world(xa, yb)}, mid = world(0.5 * (xa + xb), 0.5 * (ya + yb));
    for (int k = 0; k < 4; k++) {
        D3 m = cross(c[k], c[(k + 1) & 3]);
        const double len = std::sqrt(dot(m, m));
        if (!(len > 0.0) || !std::isfinite(len)) return false;
        if (dot(m, mid) < 0.0) m = {-m.x, -m.y, -m.z};
        n[k] = {m.x / len, m.y / len, m.z / len};
    }
    return true;
}
}  // namespace

// Which record PAIRS of FlatScene::pairs a camera ray of a pixel strip can hit (stages.hpp generate_body, traverse.hpp flat_closest1's
// mask).  A wave of k_generate_trace holds 64 consecutive local pixels; block b = local pixels 64 b .. 64 b + 63.  Every
// ray of the block leaves cam_t with a direction R (x, y, 1), (x, y) inside the rectangle that the block's pixels span on the image
// plane - whatever the jitter, which stays in [0, 1] of its pixel - so it lies inside the pyramid with apex cam_t through that
// rectangle.  masks[b] bit k is CLEAR when, for each record of pair k, all its vertices (a sphere: the corners of its padded box) are
// outside ONE of the pyramid's four side planes by more than a margin; otherwise set.  cull = false: every bit set.
//
// Why a cleared record cannot change flat_closest1's answer.  flat_candidate() leaves the running best untouched unless
// `inside && t > 1e-4`, so it is enough that this is false for every ray of the block, in the kernel's float32 arithmetic.  Let n be
// the inward unit normal of the separating side plane: n . (x - cam_t) <= -margin for every vertex x, n . d >= 0 for every ray
// (the rectangle is widened by `widen` pixels for the rounding of d, below).  Take the kernel's t and the exact point
// X = cam_t + t d.  If t > 1e-4 then n . (X - cam_t) = t (n . d) >= 0.  If the inside test accepts, X is within eps of the record's
// outline (below), hence n . (X - cam_t) <= -margin + eps < 0: both cannot hold.  Records BEHIND the camera drop out by the same test:
// they are outside every side plane, their t is negative.  With u = 2^-24, ext = the extent per axis of scene and camera, L = |ext|:
//  * height of X over the record's plane.  t = -fl(T . s) rcp(fl(T . d)), s = fl(o - p0): with e_o <= 4 u sum|T| ext the error of
//    T . s, e_d <= 3 sqrt(3) u |T| that of T . d and 3 u for rcp and the product, T . (X - p0) = t t_d' (3 u) - e_o - t e_d
//    (t_d' the computed T . d, |t t_d'| <= sum|T| ext), and |t| <= L + height because X is over the outline:
//    height <= (7 u sum|T| ext + 6 u L) / |T|;
//  * how far outside the outline the inside test may accept X: u, v come from U . P, V . P at P = fma(t, d, s), off by
//    5 u sum|U| ext and 5 u sum|V| ext; an edge function g = a u + b v + c adds its own three roundings, 3 u (|a| + |b| + |c|)
//    (the comparisons with 0 and 1/2 are exact) - divided by |a U + b V| a distance in the plane.
//  eps is the sum of the two, and margin = 16 eps: the factor covers a corner where two edges meet at an angle (the distance to the
//  outline is the overshoot over one edge divided by the sine) down to ~7 degrees and costs a strip nothing it could measure - 16 eps
//  is ~1e-4 of the Cornell box, a hundredth of a pixel's footprint on its back wall.
//  * spheres (flat_closest1's last loop): `c2ray < r2` is the squared distance of the centre from the LINE, off by <= 16 u D^2
//    (D = |centre - cam_t|; |d|^2 - 1 <= 4 u included), and a camera with cn2 <= r2 + 1e-4 takes the far root.  The box is that of
//    the radius sqrt(r^2 (1 + 4 u) + 1.1e-4 + 32 u D^2): it contains every point where an accepted line is closest to the centre, and
//    a camera that is inside the sphere or within the 1e-4 rule (the apex is then not separable: kept).  Where the box is separated, the
//    closest point has t < 0, the near root proj - cut is below proj <= -margin + 6 u D, and nothing is valid.
//  * the direction: (half_w + vx - i) inv_focal, (j - half_h - vy) inv_focal, R ., normalize: four roundings of numbers up to
//    W + H + 1 / inv_focal pixels in the image plane, then relative ones that keep the ray on its line (a positive scale) or move it by
//    <= 3 u of |(x, y, 1)| per matrix row.  widen = 64 u (W + H + 1 / inv_focal) pixels (a few 1e-3 of a pixel) is ten times their sum.
// Rays that flat_needs_cull() defers never use the sweep's answer (generate_body hands them to the reference-order code as before).
int camera_strips(const float* prims, int n_prims, const std::vector<float>& stream, const std::vector<float>& tab, const int counts[7],
                  const CamFilm& cf, bool cull, std::vector<uint64_t>& masks) {
    static_assert((APT_FLAT_MAX_PRIMS + 4) / 2 <= 64, "a strip's pair list is one 64-bit word (four sections, each with at most one odd tail)");
    const double u = std::ldexp(1.0, -24);
    const int nsec[4] = {counts[0] + counts[1], counts[2] + counts[3], counts[4] + counts[5], counts[6]};
    const int n_pairs = (nsec[0] + 1) / 2 + (nsec[1] + 1) / 2 + (nsec[2] + 1) / 2 + (nsec[3] + 1) / 2;
    const int npix = cf.n_cols * cf.height, n_blocks = (npix + 63) / 64;
    if (npix <= 0 || cf.height <= 0 || cf.band_width <= 0 || cf.world <= 0) return -1;
    const uint64_t all = ~(uint64_t)0;
    masks.assign((size_t)n_blocks, all);
    if (!cull || n_pairs > 64) return 0;
    const D3 cam = {cf.cam_t[0], cf.cam_t[1], cf.cam_t[2]};
    struct Rec { int pair; std::vector<D3> vs; double margin; };
    std::vector<Rec> recs;
    double lo[3] = {cam.x, cam.y, cam.z}, hi[3] = {cam.x, cam.y, cam.z};
    {
        size_t at = 0; int pair0 = 0;
        for (int sec = 0, r = 0; sec < 4; pair0 += (nsec[sec] + 1) / 2, sec++) for (int j = 0; j < nsec[sec]; j++, r++, at += (size_t)kRecordFloats[sec]) {
            int32_t ids[2]; memcpy(ids, tab.data() + 28 * (size_t)r + 8, 8);
            if (ids[0] < 0 || ids[0] >= n_prims || ids[1] >= n_prims) return -1;
            Rec rc; rc.pair = pair0 + j / 2; rc.margin = 0.0;
            if (sec < 3) { for (int k : {ids[0], ids[1]}) if (k >= 0) for (int v = 0; v < 3; v++) rc.vs.push_back(vtx(prims, k, v)); }
            else {
                const float* c = prims + 9 * (size_t)ids[0];
                const D3 dc = sub({c[0], c[1], c[2]}, cam);
                const double D2 = dot(dc, dc), rr = std::sqrt((double)c[3] * (double)c[3] * (1.0 + 4.0 * u) + 1.1e-4 + 32.0 * u * D2);
                for (int k = 0; k < 8; k++) rc.vs.push_back({c[0] + ((k & 1) ? rr : -rr), c[1] + ((k & 2) ? rr : -rr), c[2] + ((k & 4) ? rr : -rr)});
                rc.margin = 16.0 * 6.0 * u * (std::sqrt(D2) + rr);
            }
            for (const D3& p : rc.vs) { const double c[3] = {p.x, p.y, p.z}; for (int a = 0; a < 3; a++) { lo[a] = std::min(lo[a], c[a]); hi[a] = std::max(hi[a], c[a]); } }
            recs.push_back(rc);
        }
    }
    const D3 ext = {hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]};
    const double L = std::sqrt(dot(ext, ext));
    auto absdot = [](D3 a, D3 b) { return std::fabs(a.x) * b.x + std::fabs(a.y) * b.y + std::fabs(a.z) * b.z; };
    {
        size_t at = 0;
        for (int sec = 0, r = 0; sec < 3; sec++) for (int j = 0; j < nsec[sec]; j++, r++, at += (size_t)kRecordFloats[sec]) {
            const float* p = stream.data() + at;
            const D3 U = {p[3], p[4], p[5]}, V = {p[6], p[7], p[8]}, T = {p[9], p[10], p[11]};
            if (dot(T, T) == 0.0) continue;                      // a degenerate triangle: t = NaN, never valid; its vertices still decide its bit (margin 0)
            std::vector<std::array<double, 3>> edges = {{1, 0, 0}, {0, 1, 0}};
            if (sec == 0) { edges.push_back({1, 0, 0.5}); edges.push_back({0, 1, 0.5}); }      // |u - 1/2| <= 1/2
            if (sec == 2) edges.push_back({1, 1, 1});
            if (sec == 1) for (int e = 0; e < 2; e++) edges.push_back({p[12 + 3 * e], p[13 + 3 * e], p[14 + 3 * e]});
            double ovs = 0.0;
            for (const auto& g : edges) {
                const D3 grad = add({g[0] * U.x, g[0] * U.y, g[0] * U.z}, {g[1] * V.x, g[1] * V.y, g[1] * V.z});
                const double gl = std::sqrt(dot(grad, grad));
                if (!(gl > 0.0)) return -1;
                ovs = std::max(ovs, (5.0 * u * (std::fabs(g[0]) * absdot(U, ext) + std::fabs(g[1]) * absdot(V, ext)) + 3.0 * u * (std::fabs(g[0]) + std::fabs(g[1]) + std::fabs(g[2]))) / gl);
            }
            recs[(size_t)r].margin = 16.0 * ((7.0 * u * absdot(T, ext) + 6.0 * u * L) / std::sqrt(dot(T, T)) + ovs);
        }
    }
    const double widen = strip_widen(cf);
    for (int b = 0; b < n_blocks; b++) {
        D3 n[4];
        if (!strip_pyramid(cf, npix, b, widen, n)) continue;     // (a singular camera matrix: the full stream)
        uint64_t m = 0;
        for (const Rec& r : recs) {
            bool out = false;
            for (int k = 0; k < 4 && !out; k++) {
                double top = -1e300;
                for (const D3& p : r.vs) top = std::max(top, dot(n[k], sub(p, cam)));
                out = top < -r.margin;
            }
            if (!out) m |= (uint64_t)1 << r.pair;
        }
        masks[(size_t)b] = m;
    }
    return 0;
}

// Which PAIRS of an emitter's occluder list (flat_occluders above, in its order and pairing) can block the light sample of a CAMERA
// vertex of a pixel strip (shade_stage.hpp shade_traced<.., CAM>, traverse.hpp flat_any1's mask).  masks[e * n_blocks + b]
// bit k is CLEAR when both records of pair k of emitter e's list are separated from every shadow segment block b can produce; the rows of
// the first min(n_emit, APT_LIGHT_STRIP_EMITTERS) emitters are built.  Every bit of a word stays set when cull is false, the emitter has no
// points (it sweeps the full stream), its list has more than 64 pairs, there are more than APT_LIGHT_STRIP_EMITTERS emitters, the camera
// matrix is singular, or the block's pyramid meets a sphere record; a sphere record of the list is never separated.  It does not look at
// the camera masks.
//
// The segments.  A shadow ray of the camera vertex runs from o = fl(d t + cam_t), the hit point of a camera ray on a planar record S
// (flat_closest1 accepted it: inside S, t > 1e-4), to a light point l.  Patch = the outlines of ALL planar records (each of their
// triangles), clipped in double (Sutherland-Hodgman) against the four side planes of the block's widened pyramid (strip_pyramid),
// each plane moved OUT by E (below).  A record Q is separated when for one unit direction m
//        max over Q's vertices of m . q  <  min over the patch's vertices and the emitter's points of m . x  -  margin,
// i.e. a plane with normal m has patch and light points on its inner side and Q outside it by more than the margin.  Directions tried:
// Q's own plane (the stored T row, both signs), the six axis directions and - for an emitter of ONE point l - the planes through l and
// each edge (a, b) of a clipped polygon, (a - l) x (b - l), both signs: the faces of the cone the strip's shadow segments fill.
//
// Why a separated Q cannot block.  flat_blocks() accepts only `inside && 1e-4 < t < dist - 1e-4`.  Take the kernel's t for Q and the
// exact point X = o + t dir.  With u = 2^-24, ext = the extent per axis of scene, camera and light points, L = |ext|, Mn = |largest
// coordinates|, and eps_R of a planar record R as in camera_strips (height over R's plane of an accepted point,
// (7 u sum|T| ext + 6 u L) / |T|, plus the inside test's overshoot over an edge, ovs_R), E = 16 max_R eps_R (the factor: corners, as there):
//  * the camera ray's exact point Y = cam_t + t d is inside the pyramid (n_k . d >= 0, t > 0: camera_strips) and within E of S's
//    outline; the outline's nearest point is then at most E outside every side plane, so it lies in the clipped outline: Y is within E
//    of the patch's hull (the hit point's distance off its record and outside its outline, and the widening of the pyramid);
//  * o = fl(fl(d t) + cam_t) per component: |o - Y| <= u (L + Mn), taken twice;
//  * l: a point light's position is exact; an area-light sample is a rounded combination of its vertices, within 4 u Mn of their hull;
//  * dir = fl((l - o) / fl(|l - o|)): three subtractions, the norm, three divisions (1 ulp in the product build) leave each component
//    within 6 u of a positive multiple of the exact direction, and t < fl(|l - o|) - 1e-4 may pass the segment's end by 9 u |l - o|:
//    X is within 16 u |l - o| of the segment from o to l - 32 u L taken;
//  hence X is within rho = E + 2 u (L + Mn) + 4 u Mn + 32 u L of the hull of patch and light points: m . X >= min - rho;
//  * the inside test of Q accepts X only within E of Q's outline (eps_Q with the corner factor): m . X <= max over Q + E.
// With margin = (1 + 1e-3) (rho + E) both cannot hold, so the OR over the remaining pairs is the same boolean.  A degenerate record
// (all-zero rows: t = NaN) accepts nothing and counts as separated.  origin_slack returns E + 2 u (L + Mn), the origin's share of rho.
int light_strips(const float* prims, int n_prims, const std::vector<float>& stream, const std::vector<float>& tab, const int counts[7], const CamFilm& cf,
                 const float* pts, const int32_t* off, int n_emit, const uint8_t* keep, bool cull, std::vector<uint64_t>& masks, std::vector<int32_t>& n_pairs, double* origin_slack) {
    const double u = std::ldexp(1.0, -24);
    const int nsec[4] = {counts[0] + counts[1], counts[2] + counts[3], counts[4] + counts[5], counts[6]};
    const int n_rec = nsec[0] + nsec[1] + nsec[2] + nsec[3];
    const int npix = cf.n_cols * cf.height, n_blocks = (npix + 63) / 64, rows = std::min(n_emit, (int)APT_LIGHT_STRIP_EMITTERS);
    if (npix <= 0 || cf.height <= 0 || cf.band_width <= 0 || cf.world <= 0 || n_emit < 0) return -1;
    masks.assign((size_t)n_blocks * (size_t)rows, ~(uint64_t)0);
    n_pairs.assign((size_t)n_emit, 0);
    if (origin_slack) *origin_slack = 0.0;
    // the pair of every kept record in its emitter's list
    std::vector<int> pair_of((size_t)n_emit * (size_t)n_rec, -1);
    for (int e = 0; e < n_emit; e++) {
        int pair0 = 0, r = 0;
        for (int sec = 0; sec < 4; sec++) {
            int kept = 0;
            for (int j = 0; j < nsec[sec]; j++, r++) if (keep[(size_t)e * n_rec + r]) pair_of[(size_t)e * n_rec + r] = pair0 + (kept++) / 2;
            pair0 += (kept + 1) / 2;
        }
        n_pairs[(size_t)e] = pair0;
    }
    if (!cull || n_emit > (int)APT_LIGHT_STRIP_EMITTERS) return 0;
    const D3 cam = {cf.cam_t[0], cf.cam_t[1], cf.cam_t[2]};
    struct Rec { int sec; std::vector<D3> vs; D3 P, T; double eps, sph_margin; };
    std::vector<Rec> recs;
    double lo[3] = {cam.x, cam.y, cam.z}, hi[3] = {cam.x, cam.y, cam.z}, M[3] = {std::fabs(cam.x), std::fabs(cam.y), std::fabs(cam.z)};
    auto grow = [&](D3 p) { const double c[3] = {p.x, p.y, p.z}; for (int a = 0; a < 3; a++) { lo[a] = std::min(lo[a], c[a]); hi[a] = std::max(hi[a], c[a]); M[a] = std::max(M[a], std::fabs(c[a])); } };
    {
        size_t at = 0;
        for (int sec = 0, r = 0; sec < 4; sec++) for (int j = 0; j < nsec[sec]; j++, r++, at += (size_t)kRecordFloats[sec]) {
            int32_t ids[2]; memcpy(ids, tab.data() + 28 * (size_t)r + 8, 8);
            if (ids[0] < 0 || ids[0] >= n_prims || ids[1] >= n_prims) return -1;
            const float* p = stream.data() + at;
            Rec rc; rc.sec = sec; rc.eps = 0.0; rc.sph_margin = 0.0; rc.P = {p[0], p[1], p[2]}; rc.T = {0, 0, 0};
            if (sec < 3) { rc.T = {p[9], p[10], p[11]}; for (int k : {ids[0], ids[1]}) if (k >= 0) for (int v = 0; v < 3; v++) rc.vs.push_back(vtx(prims, k, v)); }
            else {                                               // the sphere's box, as camera_strips pads it
                const float* c = prims + 9 * (size_t)ids[0];
                const D3 dc = sub({c[0], c[1], c[2]}, cam);
                const double D2 = dot(dc, dc), rr = std::sqrt((double)c[3] * (double)c[3] * (1.0 + 4.0 * u) + 1.1e-4 + 32.0 * u * D2);
                for (int k = 0; k < 8; k++) rc.vs.push_back({c[0] + ((k & 1) ? rr : -rr), c[1] + ((k & 2) ? rr : -rr), c[2] + ((k & 4) ? rr : -rr)});
                rc.sph_margin = 16.0 * 6.0 * u * (std::sqrt(D2) + rr);
            }
            for (const D3& q : rc.vs) grow(q);
            recs.push_back(rc);
        }
    }
    const int n_pts = n_emit > 0 ? off[n_emit] : 0;
    for (int k = 0; k < n_pts; k++) grow({pts[3 * k], pts[3 * k + 1], pts[3 * k + 2]});
    const D3 ext = {hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]};
    const double L = std::sqrt(dot(ext, ext)), Mn = std::sqrt(M[0] * M[0] + M[1] * M[1] + M[2] * M[2]);
    auto absdot = [](D3 a, D3 b) { return std::fabs(a.x) * b.x + std::fabs(a.y) * b.y + std::fabs(a.z) * b.z; };
    double E = 0.0;
    {
        size_t at = 0;
        for (int sec = 0, r = 0; sec < 3; sec++) for (int j = 0; j < nsec[sec]; j++, r++, at += (size_t)kRecordFloats[sec]) {
            const float* p = stream.data() + at;
            const D3 U = {p[3], p[4], p[5]}, V = {p[6], p[7], p[8]}, T = {p[9], p[10], p[11]};
            if (dot(T, T) == 0.0) continue;
            std::vector<std::array<double, 3>> edges = {{1, 0, 0}, {0, 1, 0}};
            if (sec == 0) { edges.push_back({1, 0, 0.5}); edges.push_back({0, 1, 0.5}); }
            if (sec == 2) edges.push_back({1, 1, 1});
            if (sec == 1) for (int e = 0; e < 2; e++) edges.push_back({p[12 + 3 * e], p[13 + 3 * e], p[14 + 3 * e]});
            double ovs = 0.0;
            for (const auto& g : edges) {
                const D3 grad = add({g[0] * U.x, g[0] * U.y, g[0] * U.z}, {g[1] * V.x, g[1] * V.y, g[1] * V.z});
                const double gl = std::sqrt(dot(grad, grad));
                if (!(gl > 0.0)) return -1;
                ovs = std::max(ovs, (5.0 * u * (std::fabs(g[0]) * absdot(U, ext) + std::fabs(g[1]) * absdot(V, ext)) + 3.0 * u * (std::fabs(g[0]) + std::fabs(g[1]) + std::fabs(g[2]))) / gl);
            }
            recs[(size_t)r].eps = (7.0 * u * absdot(T, ext) + 6.0 * u * L) / std::sqrt(dot(T, T)) + ovs;
            E = std::max(E, 16.0 * recs[(size_t)r].eps);
        }
    }
    const double rho = E + 2.0 * u * (L + Mn) + 4.0 * u * Mn + 32.0 * u * L, margin = (1.0 + 1e-3) * (rho + E);
    if (origin_slack) *origin_slack = E + 2.0 * u * (L + Mn);
    const double widen = strip_widen(cf);
    std::vector<D3> patch;                                      // the vertices of the block's clipped outlines
    std::vector<D3> poly, tmp;
    std::vector<uint8_t> sep((size_t)n_rec);
    for (int b = 0; b < n_blocks; b++) {
        D3 n[4];
        if (!strip_pyramid(cf, npix, b, widen, n)) continue;
        bool sphere_seen = false;
        for (const Rec& r : recs) if (r.sec == 3) {
            bool out = false;
            for (int k = 0; k < 4 && !out; k++) {
                double top = -1e300;
                for (const D3& p : r.vs) top = std::max(top, dot(n[k], sub(p, cam)));
                out = top < -r.sph_margin;
            }
            if (!out) sphere_seen = true;
        }
        if (sphere_seen) continue;
        patch.clear();
        std::vector<std::array<D3, 2>> edges;
        for (const Rec& r : recs) {
            if (r.sec == 3 || dot(r.T, r.T) == 0.0) continue;
            for (size_t t0 = 0; t0 + 3 <= r.vs.size(); t0 += 3) {
                poly.assign(r.vs.begin() + (long)t0, r.vs.begin() + (long)t0 + 3);
                for (int k = 0; k < 4 && !poly.empty(); k++) {   // keep n_k . (x - cam) >= -E
                    tmp.clear();
                    for (size_t i = 0; i < poly.size(); i++) {
                        const D3 a = poly[i], c = poly[(i + 1) % poly.size()];
                        const double ha = dot(n[k], sub(a, cam)) + E, hc = dot(n[k], sub(c, cam)) + E;
                        if (ha >= 0.0) tmp.push_back(a);
                        if ((ha >= 0.0) != (hc >= 0.0)) { const double s = ha / (ha - hc); tmp.push_back({a.x + s * (c.x - a.x), a.y + s * (c.y - a.y), a.z + s * (c.z - a.z)}); }
                    }
                    poly.swap(tmp);
                }
                for (size_t i = 0; i < poly.size(); i++) { patch.push_back(poly[i]); if (poly.size() > 1) edges.push_back({poly[i], poly[(i + 1) % poly.size()]}); }
            }
        }
        for (int e = 0; e < rows; e++) {
            const int p0 = off[e], p1 = off[e + 1], np_e = n_pairs[(size_t)e];
            if (p1 <= p0 || np_e > 64) continue;
            const uint8_t* kp = keep + (size_t)e * n_rec;
            int open = 0;                                       // kept planar records not yet separated
            for (int r = 0; r < n_rec; r++) { sep[(size_t)r] = (kp[r] && recs[(size_t)r].sec < 3 && dot(recs[(size_t)r].T, recs[(size_t)r].T) == 0.0) ? 1 : 0; if (kp[r] && recs[(size_t)r].sec < 3 && !sep[(size_t)r]) open++; }
            auto try_dir = [&](D3 m) {
                const double len = std::sqrt(dot(m, m));
                if (!(len > 0.0) || !std::isfinite(len)) return;
                m = {m.x / len, m.y / len, m.z / len};
                double inner = 1e300;
                for (const D3& x : patch) inner = std::min(inner, dot(m, x));
                for (int k = p0; k < p1; k++) inner = std::min(inner, dot(m, {pts[3 * k], pts[3 * k + 1], pts[3 * k + 2]}));
                for (int r = 0; r < n_rec; r++) {
                    if (!kp[r] || sep[(size_t)r] || recs[(size_t)r].sec == 3) continue;
                    double top = -1e300;
                    for (const D3& q : recs[(size_t)r].vs) top = std::max(top, dot(m, q));
                    if (top < inner - margin) { sep[(size_t)r] = 1; open--; }
                }
            };
            for (int a = 0; a < 3 && open > 0; a++) for (double s : {1.0, -1.0}) try_dir({a == 0 ? s : 0.0, a == 1 ? s : 0.0, a == 2 ? s : 0.0});
            for (int r = 0; r < n_rec && open > 0; r++) {
                if (!kp[r] || sep[(size_t)r] || recs[(size_t)r].sec == 3) continue;
                const D3 T = recs[(size_t)r].T;
                try_dir(T); if (!sep[(size_t)r]) try_dir({-T.x, -T.y, -T.z});
            }
            if (p1 - p0 == 1) {
                const D3 l = {pts[3 * p0], pts[3 * p0 + 1], pts[3 * p0 + 2]};
                for (size_t i = 0; i < edges.size() && open > 0; i++) {
                    const D3 m = cross(sub(edges[i][0], l), sub(edges[i][1], l));
                    try_dir(m); if (open > 0) try_dir({-m.x, -m.y, -m.z});
                }
            }
            uint64_t w = 0;
            for (int r = 0; r < n_rec; r++) if (kp[r] && !sep[(size_t)r]) w |= (uint64_t)1 << pair_of[(size_t)e * n_rec + r];
            masks[(size_t)e * n_blocks + (size_t)b] = w;
        }
    }
    return 0;
}
}  // namespace apt
