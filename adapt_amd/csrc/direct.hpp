// direct.hpp - the direct-light viewer (upstream's BlinnPhongTracer, renderer/direct_render.py:26-88): one ray through the
// centre of every pixel of the whole film, the closest hit's Blinn-Phong highlight under ONE point light whose position is an argument of
// every call, a shadow ray that dims (x 0.1) instead of blackening.  No random number, no accumulation, no crop test.
//
// Hit pass, once per renderer (the camera never moves).  Lane = pixel: pix2ray with vx = vy = 0.5 (TracerBase fixes anti_alias = False,
// tracer_base.py:60), the renderer's own closest-hit traversal, build_hit only - no normal or bump map, no albedo texture: upstream calls
// neither process_ns nor get_uv_item here.  Kept per pixel: t (the depth map; 0 for a miss), n_s (the normal map; zero for a miss, which
// is what upstream's zero-initialised field still holds) and the hit object (-1).
//
// Shade pass, once per call.  Lane = pixel: the three words of the hit pass are read ONCE, the centre ray is made again - so that
// hit = ray * t + cam_t has the reference's bits - and then, per light position of the launch, one shadow ray with the renderer's any-hit
// traversal against EVERY record (a viewer's light is anywhere: the per-emitter occluder lists, light strips and shadow culls of the
// product build's light samples are built for the scene's own emitters and are not used) and the arithmetic of direct_render.py:73-84.
// One thread writes a pixel's three words of a frame; nothing is added to: no atomics.
// Params, Queues, DevScene and every other kernel are untouched: DirectQ is a kernel argument of its own.
#pragma once
#include "shade_stage.hpp"

struct DirectQ {
    float* depth;             // [npix], index x * H + y: the closest hit's distance, 0 for a miss (depth_map)
    float* normal;            // [npix][3]: the hit's shading normal as build_hit leaves it - not normalised where it is a mix of vertex normals (norm_map)
    int32_t* obj;             // [npix]: the hit object, -1 for a miss
    const float* emit;        // [n_frames][3]: the launch's light positions
    float* frames;            // [n_frames][npix][3]: `pixels` per light position
    int n_frames;
    float intensity[3];       // the point source's intensity (emit_int)
};

// pix2ray (tracer_base.py:137-157) through the pixel centre
APT_D f3 direct_ray(const Params& p, uint32_t lp) {
    int i, j; local_to_global(p, lp, i, j);
    const f3 cd = mk3((p.half_w + 0.5f - (float)i) * p.inv_focal, ((float)j - p.half_h - 0.5f) * p.inv_focal, 1.f);
    m33 R;
    for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) R.m[a][b] = p.cam_r[3 * a + b];
    return normalize(mul(R, cd));
}
APT_D void direct_no_hit(HitRec& rec) { rec.t = 1e7f; rec.prim = -1; rec.u = 0.f; rec.v = 0.f; }
APT_D void direct_hit_store(const DevScene& sc, const DirectQ& q, uint32_t lp, uint32_t npix, f3 o, f3 d, const HitRec& rec) {
    if (lp >= npix) return;
    float t = 0.f; f3 n = splat3(0.f); int obj = -1;
    if (rec.prim >= 0) {
        Hit it; build_hit(sc, rec.prim, rec.t, rec.u, rec.v, o, d, it);
        t = rec.t; n = it.n_s; obj = it.obj_id;
    }
    q.depth[lp] = t; q.obj[lp] = obj;
    q.normal[3 * (size_t)lp] = n.x; q.normal[3 * (size_t)lp + 1] = n.y; q.normal[3 * (size_t)lp + 2] = n.z;
}

// what a pixel's frames share: the ray, the hit and the hit object's two colours
struct DirectPix { f3 ray, hit, n_s, k_d, k_g; bool live; };
APT_D void direct_load(const DevScene& sc, const Params& p, const DirectQ& q, uint32_t lp, uint32_t npix, f3 cam, DirectPix& px) {
    const uint32_t ix = lp < npix ? lp : npix - 1u;
    const int obj = q.obj[ix];
    px.live = lp < npix && obj >= 0;
    px.ray = direct_ray(p, ix);
    px.hit = px.ray * q.depth[ix] + cam;
    px.n_s = ld3(q.normal + 3 * (size_t)ix);
    const DevBxdf& b = sc.bxdf[obj >= 0 ? obj : 0];
    px.k_d = b.k_d; px.k_g = b.k_g;
}
// the shadow ray towards `e`: direction, distance and search limit (does_intersect's min_depth - 1e-4).  A dead lane, or a light ON the hit
// point (upstream paints NaN there: no direction exists), traces nothing: limit -1 and a direction no intersector minds
struct DirectLight { f3 dir; float dist, limit; bool trace; };
APT_D DirectLight direct_light(const DirectPix& px, f3 e, f3 idle) {
    DirectLight L;
    const f3 to = e - px.hit;
    L.dist = fnorm(to);
    L.trace = px.live && L.dist > 0.f;
    L.dir = L.trace ? fdiv3(to, L.dist) : idle;
    L.limit = L.trace ? shadow_limit(L.dist) : -1.0f;
    return L;
}
// direct_render.py:79-84
APT_D f3 direct_pixel(const DirectQ& q, const DirectPix& px, f3 e, bool occluded) {
    const f3 to = e - px.hit;
    const float dist = fnorm(to);
    const f3 light_dir = fdiv3(to, dist);
    const f3 half = (light_dir - px.ray) * 0.5f;
#if APT_FAST
    const f3 half_way = fnormalize(half);
#else
    const f3 half_way = normalize(half);
#endif
    f3 spec = pow_sv(fmaxf(dot(half_way, px.n_s), 0.f), px.k_g);
    spec = spec * fminf(srcp(1e-5f + dist * dist), 1e5f);
    if (occluded) spec = spec * 0.1f;
    return (spec * mk3(q.intensity[0], q.intensity[1], q.intensity[2])) * px.k_d;
}
APT_D void direct_store(const DirectQ& q, const DirectPix& px, uint32_t lp, uint32_t npix, int f, f3 e, bool occluded) {
    if (lp >= npix) return;
    const f3 c = px.live ? direct_pixel(q, px, e, occluded) : splat3(0.f);
    float* out = q.frames + ((size_t)f * (size_t)npix + (size_t)lp) * 3;
    out[0] = c.x; out[1] = c.y; out[2] = c.z;
}

// MODE: TRACE_BVH, TRACE_SWEEP or TRACE_TILE - the closest hit as k_extend<MODE, 0> finds it (the loop of k_ao_depth)
template <int MODE>
__global__ void __launch_bounds__(TRACE_NT(MODE), (MODE == TRACE_TILE ? APT_TILE_WAVES : 1)) k_direct_hit(DevScene sc, Params p, DirectQ q, LdsPlan plan) {
    __shared__ float s_sweep[MODE == TRACE_SWEEP ? APT_SWEEP_LDS_FLOATS(BLOCK) : 1];
    const uint32_t npix = (uint32_t)p.npix;
    const f3 o = mk3(p.cam_t[0], p.cam_t[1], p.cam_t[2]);
    for (uint32_t base = blockIdx.x * TRACE_NT(MODE); base < npix; base += gridDim.x * TRACE_NT(MODE)) {
        const uint32_t lp = base + threadIdx.x;
        const bool alive = lp < npix;
        const f3 d = alive ? direct_ray(p, lp) : mk3(0.f, 0.f, 1.f);
        HitRec rec; direct_no_hit(rec);
        if (MODE == TRACE_BVH) { if (alive) traverse<false>(sc.bvh, make_stack(plan), o, d, rec); }
        else if (MODE == TRACE_SWEEP) sweep_wg<false, BLOCK>(sc.sweep, o, d, rec, alive, s_sweep);
        else sweep_tile<false, APT_TILE_NT>(sc.sweep, o, d, rec, alive, reinterpret_cast<float*>(s_dyn));
        direct_hit_store(sc, q, lp, npix, o, d, rec);
    }
}
// the any-hit traversal as k_shadow<MODE> runs it, once per light position; F is the same for every lane, so the workgroup's barriers pair up
template <int MODE>
__global__ void __launch_bounds__(TRACE_NT(MODE), (MODE == TRACE_TILE ? APT_TILE_WAVES : 1)) k_direct_shade(DevScene sc, Params p, DirectQ q, LdsPlan plan) {
    __shared__ float s_sweep[MODE == TRACE_SWEEP ? APT_SWEEP_LDS_FLOATS(BLOCK) : 1];
    const uint32_t npix = (uint32_t)p.npix;
    const f3 cam = mk3(p.cam_t[0], p.cam_t[1], p.cam_t[2]);
    for (uint32_t base = blockIdx.x * TRACE_NT(MODE); base < npix; base += gridDim.x * TRACE_NT(MODE)) {
        const uint32_t lp = base + threadIdx.x;
        DirectPix px; direct_load(sc, p, q, lp, npix, cam, px);
        for (int f = 0; f < q.n_frames; f++) {
            const f3 e = ld3(q.emit + 3 * f);
            const DirectLight L = direct_light(px, e, mk3(0.f, 0.f, 1.f));
            HitRec rec; rec.t = L.limit; rec.prim = -1; rec.u = rec.v = 0.f;
            bool occluded = false;
            if (MODE == TRACE_BVH) { if (L.trace) occluded = traverse<true>(sc.bvh, make_stack(plan), px.hit, L.dir, rec); }
            else if (MODE == TRACE_SWEEP) occluded = sweep_wg<true, BLOCK>(sc.sweep, px.hit, L.dir, rec, L.trace, s_sweep);
            else occluded = sweep_tile<true, APT_TILE_NT>(sc.sweep, px.hit, L.dir, rec, L.trace, reinterpret_cast<float*>(s_dyn));
            direct_store(q, px, lp, npix, f, e, occluded && L.trace);
        }
    }
}
#if APT_FAST
// the flat sweep: two pixels per lane.  Both passes settle the rays that need the reference-order intersector in full, here (flat_closest2
// and flat_any2 without DEFER, as ao.hpp's kernels do), against the scene's full record stream
__global__ void __launch_bounds__(BLOCK) k_direct_hit_flat(DevScene sc, Params p, DirectQ q, LdsPlan plan) {
    const uint32_t npix = (uint32_t)p.npix;
    const f3 o = mk3(p.cam_t[0], p.cam_t[1], p.cam_t[2]), idle = splat3(0.57735026f);
    for (uint32_t base = blockIdx.x * FLAT_NT; base < npix; base += gridDim.x * FLAT_NT) {
        const uint32_t i0 = base + 2u * threadIdx.x, i1 = i0 + 1u;
        const f3 d0 = i0 < npix ? direct_ray(p, i0) : idle, d1 = i1 < npix ? direct_ray(p, i1) : idle;
        HitRec r0, r1; direct_no_hit(r0); direct_no_hit(r1);
        int c0, c1;
        flat_closest2(sc.flat, sc.sweep, sc.prim_class, o, d0, o, d1, r0, r1, c0, c1);
        direct_hit_store(sc, q, i0, npix, o, d0, r0);
        direct_hit_store(sc, q, i1, npix, o, d1, r1);
    }
}
__global__ void __launch_bounds__(BLOCK) k_direct_shade_flat(DevScene sc, Params p, DirectQ q, LdsPlan plan) {
    const uint32_t npix = (uint32_t)p.npix;
    const f3 cam = mk3(p.cam_t[0], p.cam_t[1], p.cam_t[2]), idle = splat3(0.57735026f);
    for (uint32_t base = blockIdx.x * FLAT_NT; base < npix; base += gridDim.x * FLAT_NT) {
        const uint32_t i0 = base + 2u * threadIdx.x, i1 = i0 + 1u;
        DirectPix p0, p1; direct_load(sc, p, q, i0, npix, cam, p0); direct_load(sc, p, q, i1, npix, cam, p1);
        for (int f = 0; f < q.n_frames; f++) {
            const f3 e = ld3(q.emit + 3 * f);
            const DirectLight L0 = direct_light(p0, e, idle), L1 = direct_light(p1, e, idle);
            bool occ0, occ1;
            flat_any2(sc.flat, sc.sweep, p0.hit, L0.dir, p1.hit, L1.dir, L0.limit, L1.limit, occ0, occ1);
            direct_store(q, p0, i0, npix, f, e, occ0 && L0.trace);
            direct_store(q, p1, i1, npix, f, e, occ1 && L1.trace);
        }
    }
}
#endif
