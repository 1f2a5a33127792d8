// ao.hpp - the ambient-occlusion renderer (upstream's SSAORenderer, renderer/ssao.py): screen-space occlusion of the camera
// rays' first hits against a depth map of the film, on one rank.
//
// Depth map, once per renderer (ssao.py:46-63).  Slot (k, pixel) restates the k-th pix2ray call of the pixel's constructor loop: sample
// counter 0 (upstream's cnt before the first render: with stratified jitter every sample falls into stratum 0 - kept), draws 2k, 2k + 1
// of the stream (whatever pix2ray draws under the sensor's jitter settings), traced with the renderer's own traversal.  k_ao_depth_mean
// then adds a pixel's hit distances in sample order, one thread per owned pixel, and divides by the hit count: no atomics.
//
// Render (ssao.py:93-130).  One lane per (pixel, sample of the batch): the camera ray of sample number cnt_base + s + 1 (camera_ray_dir),
// its closest hit, build_hit only - no normal or bump map: upstream does not call process_ns - and the hemisphere loop, whose draws go on
// where the camera ray's ended.  A hemisphere sample is a direction about n_s, a point sample_extent along it, that point's projection
// onto the film (splat_camera / rasterize_pinhole with their gates and int() truncation), one 4-byte gather from the depth map and the
// smooth-stepped compare.  The slot keeps 1 - sum / smp_hemisphere and a hit flag; k_ao_sum adds a pixel's slots in sample order into
// channel 0 of the accumulation and notes whether the LAST sample hit, which is what upstream's `pixels` shows.
// Params, Queues, DevScene and every other kernel are untouched: AoQ is a kernel argument of its own.
#pragma once
#include "shade_stage.hpp"

struct AoQ {
    float2* rec;              // render: per slot (1 - sum / smp_hemisphere, 1 = the ray hit; zeros for a miss or a slot outside the crop window)
    float* t;                 // depth pass: per slot the hit distance, AO_MISS for a miss or a slot outside the crop window (the same memory as rec)
    float* depth;             // [W * H], index x * H + y: the depth map (0: no sample hit)
    int32_t* hits;            // depth pass: per pixel the hits so far
    int32_t* last_hit;        // per pixel: 1 = the last sample rendered hit
    int smp;                  // smp_hemisphere
    int k_base;               // depth pass: number of the batch's first sample
    float extent;             // sample_extent
    float inv_cam_r[9];       // cam_r.inverse(), row-major
    float cam_normal[3];      // (cam_r @ (0, 0, 1)).normalized()
    int x0, x1, y0, y1;       // the window rasterize_pinhole accepts: the crop window, or the film
};
#define AO_MISS (-1.f)

// pix2ray (tracer_base.py:137-157) at an explicit sample counter and first draw: camera_ray_dir's arithmetic for the constructor's loop
APT_D f3 ao_depth_ray(const Params& p, int i, int j, int sample_cnt, uint32_t first_draw) {
    Philox rng; rng_init(rng, (uint32_t)(i * p.H + j), p.seed, (uint32_t)sample_cnt, first_draw);
    float vx = 0.5f, vy = 0.5f;
    if (p.anti_alias) {
        if (p.stratified) {
            int mod_val = pymod(sample_cnt, 16);
            vx = (float)(mod_val % 4) * 0.25f + rng_float(rng) * 0.25f;
            vy = (float)(mod_val / 4) * 0.25f + rng_float(rng) * 0.25f;
        } else {
            const float eps = 1e-4f, inv_eps = (float)(1 - 1e-4 * 2.);
            vx = rng_float(rng) * inv_eps + eps;
            vy = rng_float(rng) * inv_eps + eps;
        }
    }
    f3 cd = mk3((p.half_w + vx - (float)i) * p.inv_focal, ((float)j - p.half_h - vy) * p.inv_focal, 1.f);
    m33 R;
    for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) R.m[a][b] = p.cam_r[3 * a + b];
    return normalize(mul(R, cd));
}
APT_D bool ao_in_crop(const Params& p, int i, int j) { return !p.do_crop || (i >= p.sx && i < p.ex && j >= p.sy && j < p.ey); }
// the ray of depth-pass slot idx (false: no such slot, or outside the crop window - `idle` is traced for nothing)
APT_D bool ao_depth_slot_ray(const Params& p, const AoQ& a, uint32_t idx, uint32_t total, f3 idle, f3& dir) {
    dir = idle;
    if (idx >= total) return false;
    const uint32_t lp = idx % (uint32_t)p.npix, k = idx / (uint32_t)p.npix;
    int i, j; local_to_global(p, lp, i, j);
    const bool alive = ao_in_crop(p, i, j);
    if (alive) dir = ao_depth_ray(p, i, j, 0, p.anti_alias ? 2u * (uint32_t)(a.k_base + (int)k) : 0u);
    return alive;
}
// the camera ray of render slot idx, as aov_ray makes it; draws: where the hemisphere loop goes on
APT_D bool ao_ray(const Params& p, uint32_t idx, uint32_t total, f3 idle, f3& dir, uint32_t& draws, uint32_t& key, uint32_t& ctr) {
    dir = idle; draws = 0u; key = 0u; ctr = 0u;
    if (idx >= total) return false;
    const uint32_t lp = idx % (uint32_t)p.npix, s = idx / (uint32_t)p.npix;
    int i, j; local_to_global(p, lp, i, j);
    const bool alive = ao_in_crop(p, i, j);
    if (alive) { dir = camera_ray_dir(p, i, j, s, draws); key = (uint32_t)(i * p.H + j); ctr = (uint32_t)(p.cnt_base + (int)s + 1); }
    return alive;
}

// smooth_step(0, 1, x) (ssao.py:21-24): (x - 0) / (1 - 0) is x
APT_D float ao_smooth_step(float x) {
    const float t = fminf(fmaxf(x, 0.f), 1.f);
    return (t * t) * (3.f - 2.f * t);
}
// rasterize_pinhole + splat_camera (ssao.py:65-91): the depth map at the film position a unit direction from the camera projects to,
// 0 where a gate refuses it.  local = inv_cam_r @ ray_d, divided by its z component by component.
APT_D float ao_splat_camera(const Params& p, const AoQ& a, f3 ray_d) {
    float test_depth = 0.f;
    if (dot(ray_d, mk3(a.cam_normal[0], a.cam_normal[1], a.cam_normal[2])) > 0.f) {
        m33 Ri;
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) Ri.m[r][c] = a.inv_cam_r[3 * r + c];
        const f3 local = mul(Ri, ray_d);
        const float z = local.z;
        if (z > 0.f) {
#if APT_FAST
            const float lx = sdiv(local.x, z), ly = sdiv(local.y, z);
            const int pi = (int)((p.half_w + 1.0f) - sdiv(lx, p.inv_focal)), pj = (int)((p.half_h + 1.0f) + sdiv(ly, p.inv_focal));
#else
            const float lx = local.x / z, ly = local.y / z;
            const int pi = (int)((p.half_w + 1.0f) - lx / p.inv_focal), pj = (int)((p.half_h + 1.0f) + ly / p.inv_focal);
#endif
            if (pi >= a.x0 && pj >= a.y0 && pi < a.x1 && pj < a.y1) test_depth = a.depth[(size_t)pi * (size_t)p.H + (size_t)pj];      // (inside the window, hence inside the film)
        }
    }
    return test_depth;
}
// the hemisphere loop of one hit (ssao.py:93-109,123-128): 1 - sum / smp_hemisphere.  R depends on n_s only: built once.
APT_D float ao_occlusion(const Params& p, const AoQ& a, f3 o, f3 d, float t, f3 n_s, uint32_t key, uint32_t ctr, uint32_t draw0) {
    const f3 pos = o + d * t;
    m33 R; rotation_between(mk3(0.f, 1.f, 0.f), n_s, R);
    float occlusion = 0.f;
    uint32_t c[4] = {0u, 0u, 0u, 0u}, blk = 0xffffffffu;
    for (int k = 0; k < a.smp; k++) {
        const uint32_t dr = draw0 + 2u * (uint32_t)k, b = dr >> 2;      // (draw0 is 0 or 2: a sample's two draws share a block, a block serves two samples)
        if (b != blk) { philox4x32_10(ctr, b, 0u, 0u, key, p.seed, c); blk = b; }
        const uint32_t w0 = (dr & 2u) ? c[2] : c[0], w1 = (dr & 2u) ? c[3] : c[1];
        // uniform_hemisphere (general_sampling.py:57-62)
        const float cos_theta = window_unit(w0);
        const float sin_theta = ssqrt(1.f - cos_theta * cos_theta);
        const float phi = APT_2PI * window_unit(w1);
        float sp, cp; apt_sincos(phi, &sp, &cp);
        const f3 local_dir = mk3(cp * sin_theta, cos_theta, sp * sin_theta);
        const f3 position = pos + mul(R, local_dir) * a.extent;
        const f3 rel = position - o;
        const float depth = fnorm(rel);
        const f3 ray_d = fdiv3(rel, depth);
        const float queried = ao_splat_camera(p, a, ray_d) + 1e-3f;
        const float x = sdiv(a.extent, fabsf(queried - depth));
        occlusion += ((depth >= queried) ? 1.f : 0.f) * ao_smooth_step(x);
    }
    return 1.f - sdiv(occlusion, (float)a.smp);
}
APT_D void ao_store(const DevScene& sc, const Params& p, const AoQ& a, uint32_t idx, uint32_t total, bool alive, f3 o, f3 d, const HitRec& rec,
                    uint32_t key, uint32_t ctr, uint32_t draws) {
    if (idx >= total) return;
    float2 r = make_float2(0.f, 0.f);
    if (alive && rec.prim >= 0) {
        Hit it; build_hit(sc, rec.prim, rec.t, rec.u, rec.v, o, d, it);
        r = make_float2(ao_occlusion(p, a, o, d, rec.t, it.n_s, key, ctr, draws), 1.f);
    }
    a.rec[idx] = r;
}
APT_D void ao_depth_store(const AoQ& a, uint32_t idx, uint32_t total, bool alive, const HitRec& rec) {
    if (idx < total) a.t[idx] = (alive && rec.prim >= 0) ? rec.t : AO_MISS;
}
APT_D void ao_no_hit(HitRec& rec) { rec.t = 1e7f; rec.prim = -1; rec.u = 0.f; rec.v = 0.f; }

// MODE: TRACE_BVH, TRACE_SWEEP or TRACE_TILE - the closest hit as k_extend<MODE, 0> finds it (the loop of k_aov_trace)
template <int MODE>
__global__ void __launch_bounds__(TRACE_NT(MODE), (MODE == TRACE_TILE ? APT_TILE_WAVES : 1)) k_ao_depth(DevScene sc, Params p, AoQ a, LdsPlan plan) {
    __shared__ float s_sweep[MODE == TRACE_SWEEP ? APT_SWEEP_LDS_FLOATS(BLOCK) : 1];
    const uint32_t total = (uint32_t)p.npix * (uint32_t)p.spp_batch;
    const f3 o = mk3(p.cam_t[0], p.cam_t[1], p.cam_t[2]);
    for (uint32_t base = blockIdx.x * TRACE_NT(MODE); base < total; base += gridDim.x * TRACE_NT(MODE)) {
        const uint32_t idx = base + threadIdx.x;
        f3 d;
        const bool alive = ao_depth_slot_ray(p, a, idx, total, mk3(0.f, 0.f, 1.f), d);
        HitRec rec; ao_no_hit(rec);
        if (MODE == TRACE_BVH) { if (alive) traverse<false>(sc.bvh, make_stack(plan), o, d, rec); }
        else if (MODE == TRACE_SWEEP) sweep_wg<false, BLOCK>(sc.sweep, o, d, rec, alive, s_sweep);
        else sweep_tile<false, APT_TILE_NT>(sc.sweep, o, d, rec, alive, reinterpret_cast<float*>(s_dyn));
        ao_depth_store(a, idx, total, alive, rec);
    }
}
template <int MODE>
__global__ void __launch_bounds__(TRACE_NT(MODE), (MODE == TRACE_TILE ? APT_TILE_WAVES : 1)) k_ao_trace(DevScene sc, Params p, AoQ a, LdsPlan plan) {
    __shared__ float s_sweep[MODE == TRACE_SWEEP ? APT_SWEEP_LDS_FLOATS(BLOCK) : 1];
    const uint32_t total = (uint32_t)p.npix * (uint32_t)p.spp_batch;
    const f3 o = mk3(p.cam_t[0], p.cam_t[1], p.cam_t[2]);
    for (uint32_t base = blockIdx.x * TRACE_NT(MODE); base < total; base += gridDim.x * TRACE_NT(MODE)) {
        const uint32_t idx = base + threadIdx.x;
        f3 d; uint32_t draws, key, ctr;
        const bool alive = ao_ray(p, idx, total, mk3(0.f, 0.f, 1.f), d, draws, key, ctr);
        HitRec rec; ao_no_hit(rec);
        if (MODE == TRACE_BVH) { if (alive) traverse<false>(sc.bvh, make_stack(plan), o, d, rec); }
        else if (MODE == TRACE_SWEEP) sweep_wg<false, BLOCK>(sc.sweep, o, d, rec, alive, s_sweep);
        else sweep_tile<false, APT_TILE_NT>(sc.sweep, o, d, rec, alive, reinterpret_cast<float*>(s_dyn));
        ao_store(sc, p, a, idx, total, alive, o, d, rec, key, ctr, draws);
    }
}
#if APT_FAST
// the flat sweep: two slots per lane, settled in full here (k_aov_trace_flat's loop)
__global__ void __launch_bounds__(BLOCK) k_ao_depth_flat(DevScene sc, Params p, AoQ a, LdsPlan plan) {
    const uint32_t total = (uint32_t)p.npix * (uint32_t)p.spp_batch;
    const f3 o = mk3(p.cam_t[0], p.cam_t[1], p.cam_t[2]), idle = splat3(0.57735026f);
    for (uint32_t base = blockIdx.x * FLAT_NT; base < total; base += gridDim.x * FLAT_NT) {
        const uint32_t i0 = base + 2u * threadIdx.x, i1 = i0 + 1u;
        f3 d0, d1;
        const bool a0 = ao_depth_slot_ray(p, a, i0, total, idle, d0), a1 = ao_depth_slot_ray(p, a, i1, total, idle, d1);
        HitRec r0, r1; ao_no_hit(r0); ao_no_hit(r1);
        int c0, c1;
        flat_closest2(sc.flat, sc.sweep, sc.prim_class, o, d0, o, d1, r0, r1, c0, c1);
        ao_depth_store(a, i0, total, a0, r0);
        ao_depth_store(a, i1, total, a1, r1);
    }
}
__global__ void __launch_bounds__(BLOCK) k_ao_trace_flat(DevScene sc, Params p, AoQ a, LdsPlan plan) {
    const uint32_t total = (uint32_t)p.npix * (uint32_t)p.spp_batch;
    const f3 o = mk3(p.cam_t[0], p.cam_t[1], p.cam_t[2]), idle = splat3(0.57735026f);
    for (uint32_t base = blockIdx.x * FLAT_NT; base < total; base += gridDim.x * FLAT_NT) {
        const uint32_t i0 = base + 2u * threadIdx.x, i1 = i0 + 1u;
        f3 d0, d1; uint32_t w0, w1, k0, k1, n0, n1;
        const bool a0 = ao_ray(p, i0, total, idle, d0, w0, k0, n0), a1 = ao_ray(p, i1, total, idle, d1, w1, k1, n1);
        HitRec r0, r1; ao_no_hit(r0); ao_no_hit(r1);
        int c0, c1;
        flat_closest2(sc.flat, sc.sweep, sc.prim_class, o, d0, o, d1, r0, r1, c0, c1);
        ao_store(sc, p, a, i0, total, a0, o, d0, r0, k0, n0, w0);
        ao_store(sc, p, a, i1, total, a1, o, d1, r1, k1, n1, w1);
    }
}
#endif
// one thread per owned pixel: the batch's hit distances added in sample order; last: divide by the hit count, into the map and channel 2
__global__ void __launch_bounds__(BLOCK) k_ao_depth_mean(Params p, AoQ a, float* accum, int last) {
    const uint32_t stride = gridDim.x * BLOCK;
    for (uint32_t lp = blockIdx.x * BLOCK + threadIdx.x; lp < (uint32_t)p.npix; lp += stride) {
        float sum = a.depth[lp]; int n = a.hits[lp];
        for (int k = 0; k < p.spp_batch; k++) {
            const float t = a.t[(size_t)k * (size_t)p.npix + lp];
            if (t != AO_MISS) { sum += t; n++; }
        }
        if (last) {
            if (n) sum = sum / (float)n;
            accum[3 * (size_t)lp + 2] = sum;
        }
        a.depth[lp] = sum; a.hits[lp] = n;
    }
}
// one thread per owned pixel: the batch's slots added in sample order into channel 0; whether the batch's last sample hit
__global__ void __launch_bounds__(BLOCK) k_ao_sum(Params p, AoQ a, float* accum) {
    const uint32_t stride = gridDim.x * BLOCK;
    for (uint32_t lp = blockIdx.x * BLOCK + threadIdx.x; lp < (uint32_t)p.npix; lp += stride) {
        float s0 = accum[3 * (size_t)lp];
        float2 r = make_float2(0.f, 0.f);
        for (int s = 0; s < p.spp_batch; s++) {
            r = a.rec[(size_t)s * (size_t)p.npix + lp];
            if (r.y != 0.f) s0 += r.x;
        }
        accum[3 * (size_t)lp] = s0;
        a.last_hit[lp] = (r.y != 0.f) ? 1 : 0;
    }
}
// `pixels` (ssao.py:129-130): channel 0 / cnt on all three channels where the last sample hit, else 0
__global__ void __launch_bounds__(256) k_ao_pixels(const float* accum, const int32_t* last_hit, float* out, uint32_t npix, float cnt) {
    const uint32_t lp = blockIdx.x * 256u + threadIdx.x;
    if (lp >= npix) return;
    const float v = last_hit[lp] ? accum[3 * (size_t)lp] / cnt : 0.f;
    out[3 * (size_t)lp] = v; out[3 * (size_t)lp + 1] = v; out[3 * (size_t)lp + 2] = v;
}
// apt_set_accum: channel 2 is the depth map;  apt_reset: channels 0 and 1 cleared, channel 2 put back from the map
__global__ void __launch_bounds__(256) k_ao_take_depth(const float* accum, float* depth, uint32_t npix) {
    const uint32_t lp = blockIdx.x * 256u + threadIdx.x;
    if (lp < npix) depth[lp] = accum[3 * (size_t)lp + 2];
}
__global__ void __launch_bounds__(256) k_ao_reset(float* accum, const float* depth, int32_t* last_hit, uint32_t npix) {
    const uint32_t lp = blockIdx.x * 256u + threadIdx.x;
    if (lp >= npix) return;
    accum[3 * (size_t)lp] = 0.f; accum[3 * (size_t)lp + 1] = 0.f; accum[3 * (size_t)lp + 2] = depth[lp];
    last_hit[lp] = 0;
}
