// aov.hpp - the feature-buffer (AOV) pass of the surface renderer and the edge-avoiding denoiser that reads its buffers.
//
// Feature buffers.  A pixel-sample's camera ray is a pure function of (pixel, sample number, seed): camera_ray_dir restates it from the
// counter-based stream, so a pass of its own can produce, at any time, what the rays of samples 1..n saw first - albedo (the k_d the shade
// stage would read: record colour or texture), shading normal (after the maps, world space, not flipped) and hit distance - without a
// field of Params, Queues or any render kernel changing.  One kernel per batch makes the ray, traces it with the renderer's own
// traversal (the device functions of k_extend / k_extend_flat) and writes a two-float4 record per slot (slot = sample in batch * npix +
// local pixel, as the radiance slots); k_aov_sum then adds a pixel's records in sample order - one thread per owned pixel, no atomics, as
// k_finalize does - so the sums do not depend on the batch split and repeat bit for bit.
//
// Denoiser.  Stage 1 is upstream's firefly filter (post_processing.py:15-32, a 3x3 conservative median); stage 2 the a-trous wavelet
// filter of Dammertz et al. 2010 guided by the AOV means.  Film arrays are [x][y] with y fastest: a wave's lanes lie along y, and colour
// and the two guide planes are three float4 arrays, so a tap is three 16-byte loads off wave-uniform bases.  Both stages are pure gathers
// between ping-pong buffers: no atomics, bit-identical from run to run.
#pragma once
#include "shade_stage.hpp"

struct AovQ {
    float4* rec;              // per slot: plane 0 = (albedo rgb, t), plane 1 (at rec + stride) = (n_s xyz, 1); zeros for a miss or a slot outside the crop window
    float4* sum;              // per owned pixel: [2 lp] = (sum albedo rgb, sum t), [2 lp + 1] = (sum n_s xyz, hit count)
    uint32_t stride;          // slots per plane
};

// The camera ray of slot idx of the batch (Params::cnt_base / spp_batch as a render batch sets them); false: no such slot, or its pixel lies
// outside the crop window - the direction is then `idle`, which is traced for nothing and never stored.
APT_D bool aov_ray(const Params& p, uint32_t idx, uint32_t total, f3 idle, f3& dir) {
    dir = idle;
    if (idx >= total) return false;
    const uint32_t lp = idx % (uint32_t)p.npix, s = idx / (uint32_t)p.npix;
    int i, j; local_to_global(p, lp, i, j);
    const bool alive = !p.do_crop || (i >= p.sx && i < p.ex && j >= p.sy && j < p.ey);
    uint32_t draws = 0;
    if (alive) dir = camera_ray_dir(p, i, j, s, draws);
    return alive;
}
// The slot's record: the vertex as the shade stage opens it at a camera ray's hit (build_hit, then the maps where the scene has textures)
APT_D void aov_store(const DevScene& sc, const AovQ& a, uint32_t idx, uint32_t total, bool alive, f3 o, f3 d, const HitRec& rec) {
    if (idx >= total) return;
    float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0;
    if (alive && rec.prim >= 0) {
        Hit it; int light; f3 kd;
        build_hit(sc, rec.prim, rec.t, rec.u, rec.v, o, d, it, light, kd);
        if (sc.tex_i != nullptr) surface_maps(sc, it, rec.prim, rec.u, rec.v, true, kd);
        r0 = make_float4(kd.x, kd.y, kd.z, rec.t);
        r1 = make_float4(it.n_s.x, it.n_s.y, it.n_s.z, 1.f);
    }
    a.rec[idx] = r0;
    a.rec[(size_t)a.stride + idx] = r1;
}

// MODE: TRACE_BVH, TRACE_SWEEP or TRACE_TILE - the closest hit as k_extend<MODE, 0> finds it
template <int MODE>
__global__ void __launch_bounds__(TRACE_NT(MODE), (MODE == TRACE_TILE ? APT_TILE_WAVES : 1)) k_aov_trace(DevScene sc, Params p, AovQ a, LdsPlan plan) {
    __shared__ float s_sweep[MODE == TRACE_SWEEP ? APT_SWEEP_LDS_FLOATS(BLOCK) : 1];
    const uint32_t total = (uint32_t)p.npix * (uint32_t)p.spp_batch;
    const f3 o = mk3(p.cam_t[0], p.cam_t[1], p.cam_t[2]);
    for (uint32_t base = blockIdx.x * TRACE_NT(MODE); base < total; base += gridDim.x * TRACE_NT(MODE)) {      // (whole workgroups: the sweeps synchronise)
        const uint32_t idx = base + threadIdx.x;
        f3 d;
        const bool alive = aov_ray(p, idx, total, mk3(0.f, 0.f, 1.f), d);
        HitRec rec; rec.t = 1e7f; rec.prim = -1; rec.u = 0.f; rec.v = 0.f;
        if (MODE == TRACE_BVH) { if (alive) traverse<false>(sc.bvh, make_stack(plan), o, d, rec); }
        else if (MODE == TRACE_SWEEP) sweep_wg<false, BLOCK>(sc.sweep, o, d, rec, alive, s_sweep);
        else sweep_tile<false, APT_TILE_NT>(sc.sweep, o, d, rec, alive, reinterpret_cast<float*>(s_dyn));
        aov_store(sc, a, idx, total, alive, o, d, rec);
    }
}
#if APT_FAST
// the flat sweep: two slots per lane, settled in full here as k_extend_flat's self-contained variant settles explicit rays
__global__ void __launch_bounds__(BLOCK) k_aov_trace_flat(DevScene sc, Params p, AovQ a, LdsPlan plan) {
    const uint32_t total = (uint32_t)p.npix * (uint32_t)p.spp_batch;
    const f3 o = mk3(p.cam_t[0], p.cam_t[1], p.cam_t[2]), idle = splat3(0.57735026f);      // (unit length, no zero component: an idle lane asks for no reference-order sweep)
    for (uint32_t base = blockIdx.x * FLAT_NT; base < total; base += gridDim.x * FLAT_NT) {
        const uint32_t i0 = base + 2u * threadIdx.x, i1 = i0 + 1u;
        f3 d0, d1;
        const bool a0 = aov_ray(p, i0, total, idle, d0), a1 = aov_ray(p, i1, total, idle, d1);
        HitRec r0, r1; r0.t = r1.t = 1e7f; r0.prim = r1.prim = -1; r0.u = r0.v = r1.u = r1.v = 0.f;
        int c0, c1;
        flat_closest2(sc.flat, sc.sweep, sc.prim_class, o, d0, o, d1, r0, r1, c0, c1);
        aov_store(sc, a, i0, total, a0, o, d0, r0);
        aov_store(sc, a, i1, total, a1, o, d1, r1);
    }
}
#endif
// one thread per owned pixel: the batch's records added in sample order (a miss adds zeros)
__global__ void __launch_bounds__(BLOCK) k_aov_sum(Params p, AovQ a) {
    const uint32_t stride = gridDim.x * BLOCK;
    for (uint32_t lp = blockIdx.x * BLOCK + threadIdx.x; lp < (uint32_t)p.npix; lp += stride) {
        float4 s0 = a.sum[2 * (size_t)lp], s1 = a.sum[2 * (size_t)lp + 1];
        for (int s = 0; s < p.spp_batch; s++) {
            const size_t idx = (size_t)s * (size_t)p.npix + lp;
            const float4 r0 = a.rec[idx], r1 = a.rec[(size_t)a.stride + idx];
            s0.x += r0.x; s0.y += r0.y; s0.z += r0.z; s0.w += r0.w;
            s1.x += r1.x; s1.y += r1.y; s1.z += r1.z; s1.w += r1.w;
        }
        a.sum[2 * (size_t)lp] = s0; a.sum[2 * (size_t)lp + 1] = s1;
    }
}

// ------------------------------------------------------------------ denoiser
// What the filter kernels share: the film, the window whose pixels take part (the crop window, or the film), the packed planes
struct DenoiseQ {
    int W, H, x0, x1, y0, y1;
    float4* c[2];             // colour, ping-pong: (r, g, b, -)
    float4* g0; float4* g1;   // guides: (albedo mean rgb, depth mean), (unit normal mean xyz, 1 where hit_fraction > 0)
};
#define DN_BX 4               // workgroup = 64 lanes along y x DN_BX columns
APT_D bool dn_pixel(const DenoiseQ& q, int& x, int& y) {
    y = (int)(blockIdx.x * 64u + threadIdx.x); x = (int)(blockIdx.y * DN_BX + threadIdx.y);
    return x < q.W && y < q.H;
}
APT_D float4 dn_demodulate(float4 c, float4 g0, float4 g1) {      // c / max(albedo, 1e-3) where the pixel was hit
    if (g1.w > 0.f) { c.x = c.x / fmaxf(g0.x, 1e-3f); c.y = c.y / fmaxf(g0.y, 1e-3f); c.z = c.z / fmaxf(g0.z, 1e-3f); }
    return c;
}
// colour (non-finite components -> 0) and the guides from the AOV sums (null: nothing was hit); demod: the colour leaves demodulated
__global__ void __launch_bounds__(256) k_dn_prepare(DenoiseQ q, const float* rgb, const float4* aov_sum, int demod) {
    const uint32_t lp = blockIdx.x * 256u + threadIdx.x;
    if (lp >= (uint32_t)(q.W * q.H)) return;
    const float r = rgb[3 * lp], g = rgb[3 * lp + 1], b = rgb[3 * lp + 2];
    float4 c = make_float4(isfinite(r) ? r : 0.f, isfinite(g) ? g : 0.f, isfinite(b) ? b : 0.f, 0.f);
    float4 g0 = make_float4(0.f, 0.f, 0.f, 0.f), g1 = g0;
    if (aov_sum) {
        const float4 s0 = aov_sum[2 * (size_t)lp], s1 = aov_sum[2 * (size_t)lp + 1];
        if (s1.w > 0.f) {
            g0 = make_float4(s0.x / s1.w, s0.y / s1.w, s0.z / s1.w, s0.w / s1.w);
            f3 n = mk3(s1.x / s1.w, s1.y / s1.w, s1.z / s1.w);
            const float len = sqrtf((n.x * n.x + n.y * n.y) + n.z * n.z);
            if (len > 0.f) n = mk3(n.x / len, n.y / len, n.z / len);
            g1 = make_float4(n.x, n.y, n.z, 1.f);
        }
    }
    if (demod) c = dn_demodulate(c, g0, g1);
    q.c[0][lp] = c; q.g0[lp] = g0; q.g1[lp] = g1;
}
// Stage 1 (post_processing.py:15-32): on the zero-padded film a pixel keeps its value if any of its 8 neighbours lies within Euclidean rgb
// distance < threshold of it, else it becomes the float32 sum of the 8, first index outermost, / 8.  c[src] -> c[src ^ 1].
__global__ void __launch_bounds__(64 * DN_BX) k_dn_firefly(DenoiseQ q, int src, float threshold, int demod) {
    int x, y;
    if (!dn_pixel(q, x, y)) return;
    const float4* in = q.c[src];
    const size_t lp = (size_t)x * q.H + y;
    const float4 c = in[lp];
    bool keep = false;
    float sr = 0.f, sg = 0.f, sb = 0.f;
    for (int dx = -1; dx <= 1; dx++)
        for (int dy = -1; dy <= 1; dy++) {
            if (dx == 0 && dy == 0) continue;
            const int qx = x + dx, qy = y + dy;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (qx >= 0 && qx < q.W && qy >= 0 && qy < q.H) v = in[(size_t)qx * q.H + qy];
            const float ex = v.x - c.x, ey = v.y - c.y, ez = v.z - c.z;
            keep = keep || sqrtf((ex * ex + ey * ey) + ez * ez) < threshold;
            sr += v.x; sg += v.y; sb += v.z;
        }
    float4 o = keep ? c : make_float4(sr / 8.f, sg / 8.f, sb / 8.f, 0.f);
    if (demod) o = dn_demodulate(o, q.g0[lp], q.g1[lp]);
    q.c[src ^ 1][lp] = o;
}
// Stage 2, one a-trous iteration: 5x5 taps `step` apart, weight = h(dx) h(dy) w_n w_z w_a w_c w_hit; taps outside the
// window are skipped, the centre tap counts with h(0)^2 whatever the guides say.  inv_c2 = 1 / (sigma_c 2^-k)^2, 0: no colour term.
// remod: the last iteration multiplies the albedo back.  A pixel outside the window keeps its value.  c[src] -> c[src ^ 1].
struct AtrousPar { int step; float sigma_n, inv_z, inv_a2, inv_c2; int remod; };
__global__ void __launch_bounds__(64 * DN_BX) k_dn_atrous(DenoiseQ q, int src, AtrousPar ap) {
    int x, y;
    if (!dn_pixel(q, x, y)) return;
    const float4* in = q.c[src];
    const size_t lp = (size_t)x * q.H + y;
    const float4 cp = in[lp], ap0 = q.g0[lp], ap1 = q.g1[lp];
    float4 o = cp;
    if (x >= q.x0 && x < q.x1 && y >= q.y0 && y < q.y1) {
        const float hk[3] = {0.375f, 0.25f, 0.0625f};
        const bool hit = ap1.w > 0.f;
        const float zs = ap.inv_z / fmaxf(ap0.w, 1e-6f);
        float sr = 0.f, sg = 0.f, sb = 0.f, sw = 0.f;
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + dx * ap.step;
            if (qx < q.x0 || qx >= q.x1) continue;
            for (int dy = -2; dy <= 2; dy++) {
                const int qy = y + dy * ap.step;
                if (qy < q.y0 || qy >= q.y1) continue;
                const size_t lq = (size_t)qx * q.H + qy;
                const float4 cq = in[lq];
                float w = hk[dx < 0 ? -dx : dx] * hk[dy < 0 ? -dy : dy];
                if (dx != 0 || dy != 0) {
                    const float4 q0 = q.g0[lq], q1 = q.g1[lq];
                    if ((q1.w > 0.f) != hit) continue;
                    const float er = cp.x - cq.x, eg = cp.y - cq.y, eb = cp.z - cq.z;
                    float e = ap.inv_c2 > 0.f ? ((er * er + eg * eg) + eb * eb) * ap.inv_c2 : 0.f;
                    if (hit) {
                        const float ar = ap0.x - q0.x, ag = ap0.y - q0.y, ab = ap0.z - q0.z;
                        e += fabsf(ap0.w - q0.w) * zs + ((ar * ar + ag * ag) + ab * ab) * ap.inv_a2;
                        const float nd = fmaxf((ap1.x * q1.x + ap1.y * q1.y) + ap1.z * q1.z, 0.f);
                        w *= powf(nd, ap.sigma_n);
                    }
                    w *= expf(-e);
                }
                sr += w * cq.x; sg += w * cq.y; sb += w * cq.z; sw += w;
            }
        }
        o = make_float4(sr / sw, sg / sw, sb / sw, 0.f);
    }
    if (ap.remod && ap1.w > 0.f) { o.x *= fmaxf(ap0.x, 1e-3f); o.y *= fmaxf(ap0.y, 1e-3f); o.z *= fmaxf(ap0.z, 1e-3f); }
    q.c[src ^ 1][lp] = o;
}
__global__ void __launch_bounds__(256) k_dn_unpack(DenoiseQ q, int src, float* rgb) {
    const uint32_t lp = blockIdx.x * 256u + threadIdx.x;
    if (lp >= (uint32_t)(q.W * q.H)) return;
    const float4 c = q.c[src][lp];
    rgb[3 * lp] = c.x; rgb[3 * lp + 1] = c.y; rgb[3 * lp + 2] = c.z;
}
