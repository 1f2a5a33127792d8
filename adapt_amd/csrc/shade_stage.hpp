// shade_stage.hpp - the shade stage of the wavefront path tracer (vanilla_renderer.py:36-117): what a path does at a vertex between two
// closest-hit queries - emission and its MIS weight, Russian roulette, one shadow ray per useful light sample, the continuation ray.
//
// Two kernels are made of the same three shading steps (open_vertex, sample_light, emit_and_scatter):
//   k_shade / k_shade_group  the STAGED kernel: reads what an extend kernel wrote (SoA queues, or the packed queue of one material
//                            class) and writes the next ray queue and the shadow queue (both builds, every trace mode);
//   k_shade_traced           the kernel that TRACES ITS OWN RAYS (product build, flat sweep, unsorted, one light sample per vertex -
//                            C1 / C2): continuation ray and light sample are swept against the scene's records in place, a bounce is
//                            one launch, and the path's radiance travels with its record.
#pragma once
#include "stages.hpp"

// ----------------------------------------------------------------- textures
// Taichi's float `a % b` is a - b * floor(a / b) (python/taichi/lang/ops.py, mod)
APT_D float ti_fmod(float a, float b) { float q = floorf(a / b); return a - b * q; }
APT_D f3 mix3(f3 a, f3 b, float t) { return a * (1.0f - t) + b * t; }          // taichi.math.mix: x * (1 - a) + y * a
// Texture.query, bxdf/texture.py:111-139: bilinear lookup inside the texture's rectangle of the atlas.
// Contract (the coordinates come straight from a scene file: OBJ `vt`, XML scale_u / scale_v):
//   * the wrapped coordinate lies in [0, w-1) and floor + 1 <= w-1: the reference's arithmetic, bit for bit - the clamps below are the identity;
//   * the float remainder comes out as w-1 itself (a tiny negative coordinate: a - b * floor(a / b) rounds to b): the last texel itself,
//     what the reference's formula gives when the neighbour it reads at weight 0 is finite;
//   * any other coordinate (the remainder of a large tile count leaves [0, w-1); an overflowing product or a non-finite coordinate gives
//     NaN): upstream reads an unchecked field there, nothing to be faithful to.  Here no texel outside the rectangle is ever read: the
//     floor is clamped to [0, w-1] in float before the cast, a NaN goes to 0 (fmaxf returns its other operand), the ceil texel is
//     min(floor + 1, w-1).  The ratios stay as computed (always in [0, 1] when they are numbers); a NaN ratio counts as 0.  So every
//     lookup is a convex combination of the rectangle's own texels: finite when they are.
APT_D f3 texture_query(const DevScene& sc, int map, int obj, float u, float v) {
    const int* ti_ = sc.tex_i + 15 * obj + 5 * map; const float* tf = sc.tex_f + 6 * obj + 2 * map;
    const float w = (float)ti_[3], h = (float)ti_[4];
    const float scaled_u = ti_fmod((u * tf[0]) * w, w - 1.f), scaled_v = ti_fmod((v * tf[1]) * h, h - 1.f);
    float floor_u = floorf(scaled_u), floor_v = floorf(scaled_v);
    const float ratio_u = fmaxf(scaled_u - floor_u, 0.f), ratio_v = fmaxf(scaled_v - floor_v, 0.f);
    floor_u = fminf(fmaxf(floor_u, 0.f), w - 1.f); floor_v = fminf(fmaxf(floor_v, 0.f), h - 1.f);
    const float ceil_u = fminf(floor_u + 1.f, w - 1.f), ceil_v = fminf(floor_v + 1.f, h - 1.f);
    const int fu = (int)(floor_u + (float)ti_[1]), fv = (int)(floor_v + (float)ti_[2]), cu = (int)(ceil_u + (float)ti_[1]), cv = (int)(ceil_v + (float)ti_[2]);
    const float* img = sc.atlas[map]; const int W = sc.atlas_w[map];
    const float* r0 = img + (size_t)fv * W * 3; const float* r1 = img + (size_t)cv * W * 3;
    const f3 q_ff = ld3(r0 + 3 * fu), q_cf = ld3(r0 + 3 * cu), q_fc = ld3(r1 + 3 * fu), q_cc = ld3(r1 + 3 * cu);
    return mix3(mix3(q_ff, q_cf, ratio_u), mix3(q_fc, q_cc, ratio_u), ratio_v);
}
// PathTracer.get_uv_item, path_tracer.py:276-289 (meshes only: textured spheres are refused at scene creation)
APT_D bool get_uv_item(const DevScene& sc, int map, int obj, int prim, float bu, float bv, f3& out) {
    if (sc.atlas[map] == nullptr || !(sc.tex_i[15 * obj + 5 * map] > -255)) return false;
    const float* uv = sc.uvs + 6 * prim;
    const float w0 = 1.f - bu - bv;
    const float gu = (uv[2] * bu + uv[4] * bv) + uv[0] * w0, gv = (uv[3] * bu + uv[5] * bv) + uv[1] * w0;
    out = texture_query(sc, map, obj, gu, gv);
    return true;
}
// The maps of a vertex on object it.obj_id, primitive `prim`, at barycentrics (bu, bv); returns which applied (1 albedo, 2 normal, 4 bump).
// What open_vertex does with the scene's textures, and what apt_surface_maps_probe runs on explicit inputs.
APT_D int surface_maps(const DevScene& sc, Hit& it, int prim, float bu, float bv, bool first_hit, f3& k_d) {
    int applied = 0; f3 tx;
    if (first_hit) {                                 // PathTracer.process_ns, applied to the camera ray's hit only (vanilla_renderer.py:42)
        if (get_uv_item(sc, 1, it.obj_id, prim, bu, bv, tx)) { m33 R; rotation_between(mk3(0.f, 1.f, 0.f), it.n_g, R); it.n_s = mul(R, tx); applied |= 2; }
        if (get_uv_item(sc, 2, it.obj_id, prim, bu, bv, tx)) { it.n_s = delocalize(it.n_s, tx); applied |= 4; }
    }
    // it.tex (vanilla_renderer.py:66): every surface model reads its diffuse colour as select(tex invalid, k_d, tex)
    // and nothing else reads k_d on the device, so a valid lookup simply replaces this path's copy of k_d
    if (get_uv_item(sc, 0, it.obj_id, prim, bu, bv, tx)) { k_d = tx; applied |= 1; }
    return applied;
}

// -------------------------------------------------------------------- shade
// AT: `o` is the hit point itself (the 56-byte path record carries it, stages.hpp TrRecord); d and t are not read
template <bool AT = false>
APT_D void build_hit_rec(const DevScene& sc, float4 ra, float4 rb, int prim, float t, float u, float v, f3 o, f3 d, Hit& it, int& hit_light, f3& k_d, bool with_vn = true);
APT_D void build_hit(const DevScene& sc, int prim, float t, float u, float v, f3 o, f3 d, Hit& it, int& hit_light, f3& k_d) {
    build_hit_rec(sc, sc.prim_shade[2 * prim], sc.prim_shade[2 * prim + 1], prim, t, u, v, o, d, it, hit_light, k_d);
}
template <bool AT>
APT_D void build_hit_rec(const DevScene& sc, float4 ra, float4 rb, int prim, float t, float u, float v, f3 o, f3 d, Hit& it, int& hit_light, f3& k_d, bool with_vn) {
    const int code = __float_as_int(ra.w);
    it.prim_id = prim; it.min_depth = t;
    it.obj_id = (code < 0) ? ~code : code;
    hit_light = __float_as_int(rb.x);
    k_d = mk3(rb.y, rb.z, rb.w);
    if (code < 0) {
        // sphere: the record holds the centre; normal from the hit point (tracer_base.py:217-223)
        it.n_g = normalize((AT ? o : (o + d * t)) - mk3(ra.x, ra.y, ra.z));
        it.n_s = it.n_g;
    } else {
        it.n_g = mk3(ra.x, ra.y, ra.z);
        if (with_vn && sc.has_vn) {
            const float4 v0 = sc.vnormals[3 * prim], v1 = sc.vnormals[3 * prim + 1], v2 = sc.vnormals[3 * prim + 2];
            // interpolated vertex normal, NOT re-normalised (tracer_base.py:228-230)
            it.n_s = (mk3(v0.x, v0.y, v0.z) * (1.f - u - v) + mk3(v1.x, v1.y, v1.z) * u) + mk3(v2.x, v2.y, v2.z) * v;
        } else it.n_s = it.n_g;
    }
}
APT_D void build_hit(const DevScene& sc, int prim, float t, float u, float v, f3 o, f3 d, Hit& it) {
    int light; f3 kd; build_hit(sc, prim, t, u, v, o, d, it, light, kd);
}

#if APT_FAST
// ---- rays traced in place (Params::traced; product build, flat sweep, unsorted, one light sample per vertex)
// The shade kernel sweeps its continuation ray against the scene's records itself (flat_closest1: one ray against two records per packed
// instruction), as it already does with its light sample, and k_generate does the same for the camera rays: a bounce is ONE launch
// instead of extend + fix-up + shade, the ray is never read back (24 + 8 bytes per segment), and a ray that hits nothing never enters a
// queue - its path ends where it was sampled (18 % of C2's continuation rays: no record written, no idle lane in the next launch).
// The rare rays that need the reference's own arithmetic (traverse.hpp flat_closest2: near-tied coplanar faces, directions for which
// upstream's slab cull is part of the result) are queued with a provisional record and listed, as before - but the lists are served by
// the NEXT launch itself instead of a fix-up launch per bounce (a launch boundary is a pipeline drain: ~20 us of a render lane each):
// a wave that finds its sub-queue's lists non-empty claims them (one atomic), serves them - one entry per lane, the full reference-order
// code - and publishes "done"; the sub-queue's other waves wait for that before they read a record.  The lists are empty in all but a few
// launches per render, where the whole protocol is two scalar loads per wave; the serving code sits in front of the kernel's main loop,
// where almost no register is live, so it costs the hot loop nothing (k_fix_flat alone allocates 84 VGPRs, the shade kernel 122).
// Nothing depends on how workgroups are placed: whichever wave claims a list is running, hence the waiters cannot starve it.
// C56: the launch's records are 56 bytes (stages.hpp TrRecord) - a staged ray's origin becomes the resolved record's hit point here.
template <bool C56 = false>
APT_D void fix_prologue(const DevScene& sc, const Params& p, const Queues& q, Counters* cnt, int cur, int sq, int bounce) {
    typedef TrRecord<C56> Rec;
    const uint32_t epoch = (uint32_t)bounce + 1u;
    const int ncls = q.tr_ncls;
    uint32_t* n_def_p = &cnt->n_tr[bounce % 3][ncls][sq * CNT_PAD]; uint32_t* n_sh_p = &cnt->n_fix_sh[cur ^ 1][sq * CNT_PAD];
    // Memory order.  The list lengths are read first (the claim word below is read AFTER them), then the claim word.  A wave that
    // finds this bounce claimed - by a running or a finished server - waits for "done" with an acquire load whatever lengths it saw, so
    // that everything the server appended or added (queue records, counters, radiance slots) happens-before this wave's reads; the
    // server resets the light-sample list BEFORE it publishes "done", and only after its claim, so lengths of zero seen together with an
    // unclaimed bounce are the lists' true lengths.
    // (relaxed loads performed at L2 and a WORKGROUP-scope fence - a wait for the loads, no cache invalidate - give the load-load order;
    // acquire loads at agent scope put a `buffer_inv` behind each of them in every wave of every launch: C1 4 709 -> 3 442 Msamples/s, C2's
    // shade kernel 18.2 -> 20.0 ms per 256 spp, measured.  The acquire that matters is the one on "done" below.)
    const uint32_t n_def = __hip_atomic_load(n_def_p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), n_sh = min(__hip_atomic_load(n_sh_p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), q.sh_subcap);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    uint32_t old = __hip_atomic_load(&cnt->fix_claim[sq * CNT_PAD], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old < epoch) {
        if ((n_def | n_sh) == 0u) return;                     // nothing listed, nobody serving
        if (lane_id() == 0) old = atomicMax(&cnt->fix_claim[sq * CNT_PAD], epoch);
        old = (uint32_t)__builtin_amdgcn_readlane((int)old, 0);
    }
    if (old >= epoch) {                                       // somebody else serves (or has served) the lists of this bounce
        while (__hip_atomic_load(&cnt->fix_done[sq * CNT_PAD], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < epoch) __builtin_amdgcn_s_sleep(16);
        return;
    }
    const uint32_t qbase = (uint32_t)sq * p.subcap, sh_qbase = (uint32_t)sq * q.sh_subcap;
    const bool need_uv = sc.has_vn || sc.tex_i != nullptr;
    for (uint32_t base = 0; base < n_def; base += 64u) {      // staged rays: closest hit by the reference-order code, then the record joins its class queue (or the path ends)
        const uint32_t li = base + lane_id(); const bool valid = li < n_def;
        // (staging at the top of the sub-queue's own region: served from its LOWEST slot upwards - a resolved record is appended at or below the
        // slot its ray was just read from, never onto a staged ray that is still to be served)
        const uint32_t lj = valid ? li : n_def - 1u;
        const uint32_t is = q.tr_stage_top ? qbase + p.subcap - n_def + lj : (uint32_t)ncls * p.cap + qbase + lj, io = is << 4;
        const float4 ra = ldq(q.tr[cur][0], io), rb = ldq(q.tr[cur][1], io), rc = ldq(q.tr[cur][2], io);
        float4 rd = make_float4(0.f, 0.f, 0.f, 0.f);      // (a 56-byte camera ray has no plane D)
        if (!C56 || bounce > 0) rd = Rec::load_d(q.tr[cur][3], is);
        const f3 o = mk3(ra.x, ra.y, ra.z), d = mk3(rb.x, rb.y, rb.z), lc = Rec::Lc(rc, rd);      // (staged: the three words of plane A hold the ray's origin in either form)
        HitRec r0, r1; r0.t = r1.t = 1e7f; r0.prim = r1.prim = -1; r0.u = r0.v = r1.u = r1.v = 0.f;
        int c0, c1;
        flat_closest2(sc.flat, sc.sweep, sc.prim_class, o, d, o, d, r0, r1, c0, c1);
        if (valid && r0.prim >= 0) {
            const int oc = ncls > 1 ? c0 : 0;
            const uint32_t pos = atomicAdd(&cnt->n_tr[bounce % 3][oc][sq * CNT_PAD], 1u);      // (one atomic per entry: this path is a handful of rays per million)
            const uint32_t slot = (uint32_t)oc * p.cap + qbase + pos;
            // (the 64-byte form's two stores stay as they were written: through put_a / put_b the hit record's fields are read in another order and
            // the parent's kernels come out with two registers swapped)
            if constexpr (C56) {
                auto pm = [pm0 = Rec::pm(ra, rb), prim = r0.prim] { return (pm0 & ~0xffu) | (uint32_t)prim; };
                Rec::put_a(q.tr[cur][0], slot, hit_point_of(o, d, r0.t), r0.t, pm); Rec::put_b(q.tr[cur][1], slot, d, pm, Rec::id(rb, rc));
            } else {
                stq(q.tr[cur][0], slot << 4, make_float4(ra.x, ra.y, ra.z, r0.t));
                stq(q.tr[cur][1], slot << 4, make_float4(rb.x, rb.y, rb.z, __uint_as_float((__float_as_uint(rb.w) & ~0xffu) | (uint32_t)r0.prim)));
            }
            Rec::copy_c(q.tr[cur][2], slot, rc); if (!C56 || bounce > 0) Rec::copy_d(q.tr[cur][3], slot, rd);      // (throughput, id, radiance, pdf: as they were staged)
            if (need_uv) { float2 uv_; uv_.x = r0.u; uv_.y = r0.v; stq(q.tr_uv[cur], slot << 3, uv_); }
        } else if (valid && !(lc.x == 0.f && lc.y == 0.f && lc.z == 0.f)) {      // nothing hit: the path ends, its radiance goes to its slot
            add_radiance(q.L, p.cap, radiance_slot(p, Rec::id(rb, rc)), lc, true);
        }
    }
    uint32_t t_lit = 0;
    for (uint32_t base = 0; base < n_sh; base += 64u) {       // light samples the previous bounce could not settle (shadow_flat_body<3>)
        const uint32_t li = base + lane_id(); const bool valid = li < n_sh;
        const uint32_t io = (sh_qbase + (valid ? li : n_sh - 1u)) << 2;
        const f3 o = ld3q(q.sh_o, q.sh_cap, io), d = ld3q(q.sh_d, q.sh_cap, io), c = ld3q(q.sh_c, q.sh_cap, io);
        const float dist = ldq(q.sh_tmax, io); const uint32_t slot = ldq(q.sh_id, io);
        bool occ, occ_b;
        const float lim = shadow_limit(dist);
        flat_any2(sc.flat, sc.sweep, o, d, o, d, lim, lim, occ, occ_b);
        // (several samples of one vertex may be listed - S > 1 - and share its slot: one entry at a time within the wave's 64)
        const bool weird = !(isfinite(c.x) && isfinite(c.y) && isfinite(c.z));
        const bool add = valid && (!occ || weird);
        for (unsigned long long m = __ballot(add); m != 0ull; m &= m - 1ull) {
            if ((int)lane_id() == __ffsll((long long)m) - 1) add_radiance(q.L, p.cap, slot, occ ? c * 0.f : c, true);      // (k_shadow: an occluded non-finite sample enters upstream's sum as 0 * contribution)
        }
        t_lit += (valid && !occ) ? 1u : 0u;
    }
    flush_stat(t_lit, &cnt->stats[sq][ST_LIT]);
    if (lane_id() == 0) __hip_atomic_store(n_sh_p, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // consumed - before "done" is published (the bounce after this one appends to this list again; the staging queue's counter rotates with the others)
    __threadfence();
    if (lane_id() == 0) __hip_atomic_store(&cnt->fix_done[sq * CNT_PAD], epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
#endif
// The shade kernels' scalar operands.  Scene, parameters and queues arrive by value in the kernel-argument segment - ~1.8 KB, of which a
// tile row touches ~165 dwords - and left alone the compiler loads every field it needs ONCE, in front of the row loop, where 102 scalar
// registers cannot hold them: the rest lives in lanes of two spill VGPRs and comes back through v_readlane at every use (242 of the 2 200
// VALU instructions of C2's row loop - on the unit this kernel is bound by).  So the arguments are read THROUGH THE SEGMENT POINTER, and
// the pointer is made opaque at the head of every phase of a row (an empty asm: APT_ARGS_PHASE): a field's load can then not be hoisted
// above the phase that uses it, it becomes an s_load (scalar memory, not a VALU issue slot; the segment stays in the scalar cache) next
// to its use, and its register is free again after the phase.
struct ShadeArgs3 { DevScene sc; Params p; Queues q; };          // the leading arguments of every shade kernel, laid out as the segment lays them out
typedef const __attribute__((address_space(4))) ShadeArgs3* args3_ptr;
APT_D args3_ptr kernel_args3() { return (args3_ptr)__builtin_amdgcn_kernarg_segment_ptr(); }
APT_D const ShadeArgs3* args_fresh(args3_ptr a) {
    asm volatile("" : "+s"(a));
    return (const ShadeArgs3*)a;
}
#define APT_ARGS_PHASE() (A_ = args_fresh(A0))
// ---- a vertex while it is shaded, and the three steps both shade kernels take with it (vanilla_renderer.py:36-120)
struct Vertex {
    f3 o, d, thr, hit_point; uint32_t id, l_off, draw0; float emission_weight;      // l_off: byte offset of the path's radiance slot; draw0: the path's draw index on entry
    Hit it; int hit_light; DevBxdf bx;
};
APT_D void vertex_reset(Vertex& vx) {
    vx.o = splat3(0.f); vx.d = mk3(0.f, 0.f, 1.f); vx.thr = splat3(0.f); vx.hit_point = splat3(0.f); vx.id = 0; vx.l_off = 0; vx.draw0 = 0; vx.emission_weight = 1.0f;
    vx.it.obj_id = -1; vx.it.prim_id = -1; vx.it.n_s = vx.it.n_g = mk3(1.f, 0.f, 0.f); vx.it.min_depth = 0.f; vx.hit_light = -1;
    vx.bx.type = 1; vx.bx.is_delta = 0; vx.bx.is_bsdf = 0; vx.bx.k_d = vx.bx.k_s = vx.bx.k_g = vx.bx.mean = splat3(0.f); vx.bx.ior = 1.f;
}
// Step 1, after the hit has been built (vx.it, vx.hit_light; rec_kd: the colour in the primitive's record): material and textures, the
// path's radiance slot and random stream, the emission MIS weight of this hit (the tail of the previous iteration, vanilla_renderer.py:
// 111-117) and the roulette (vanilla_renderer.py:50-57).  false: the path ends here.
// RNG: the vertex's generator (rng.hpp).  A DrawWindow is filled here, once, with every word the vertex will draw (jitter_tail: the camera-fed
// kernel's words 2 and 3 of block 0, left by the jitter's pass - camera_ray_dir - so that the block is not generated again; else null).
template <int BM, int SM, int TEX, typename RNG>
APT_D bool open_vertex(const ShadeArgs3* A_, Vertex& vx, RNG& rng, int prim, f3 rec_kd, uint32_t meta, float ray_pdf, float2 uv, int bounce, const uint32_t* jitter_tail = nullptr) {
    const bool was_spec = (meta >> 24) & 1u;
    if (BM == APT_BX_LAMBERTIAN) vx.bx.k_d = rec_kd;               // Lambertian-only scenes: type 1, not delta, not a BSDF (vertex_reset), colour from the record
    else vx.bx = ld_bxdf_lane((A_->sc).bxdf + vx.it.obj_id);
    if (TEX && (A_->sc).tex_i != nullptr) surface_maps((A_->sc), vx.it, prim, uv.x, uv.y, bounce == 0, vx.bx.k_d);      // the scene declares image textures (TEX kernels only)
    const uint32_t lp = vx.id & ((1u << (A_->p).pix_bits) - 1u), s = vx.id >> (A_->p).pix_bits;
    vx.l_off = radiance_slot((A_->p), vx.id);
    vx.draw0 = meta & 0xffffu;
    const uint32_t key0 = ((A_->p).world == 1) ? lp : ldq((A_->p).pix_key, lp << 2), ctr0 = (uint32_t)((A_->p).cnt_base + (int)s + 1);
    rng_init(rng, key0, (A_->p).seed, ctr0, vx.draw0);
    if (bounce > 0 && (A_->p).use_mis) {
        float e_pdf = 0.0f;
        if (vx.hit_light >= 0 && vx.bx.is_delta == 0 && !was_spec) e_pdf = emitter_solid_angle_pdf((A_->sc).src[vx.hit_light], vx.it, vx.d);
        vx.emission_weight = balance(ray_pdf, e_pdf);
    }
    if constexpr (std::is_same<RNG, DrawWindow>::value) {
        // every draw of this vertex is decided: the roulette by its throughput, a second emitter index by the surface it is on (sample_light)
        static_assert(BM == APT_BX_LAMBERTIAN && !(SM & APT_SRC_AREA), "a draw window serves [roulette] index [index] u1 u2: Lambertian surfaces, emitters that draw nothing");
        bool roulette = false; float mx = 0.f;
        if ((A_->p).use_rr) { mx = max3(vx.thr); roulette = mx < (A_->p).rr_threshold && bounce >= (A_->p).rr_bounce_th; }
        else if (max3(vx.thr) < 1e-4f) return false;
        const bool relight = vx.hit_light >= 0 && (A_->sc).n_sources > 1;
        const bool have_first = jitter_tail != nullptr && (A_->p).anti_alias != 0;      // (wave-uniform; the jitter drew two numbers: this vertex starts at word 2)
        uint32_t c[4] = {0u, 0u, have_first ? jitter_tail[0] : 0u, have_first ? jitter_tail[1] : 0u};
        if (!window_open(rng, key0, (A_->p).seed, ctr0, vx.draw0, roulette, mx, relight, c, have_first, [](bool v) { return __any(v) != 0; })) return false;
        if (roulette) vx.thr = vx.thr * srcp(mx + 1e-7f);
        return true;
    } else {
        if (!(SM & APT_SRC_AREA)) rng_open(rng);               // no area lights: a shade with one light sample draws at most five numbers (rng.hpp)
        if ((A_->p).use_rr) {
            float mx = max3(vx.thr);
            if (mx < (A_->p).rr_threshold && bounce >= (A_->p).rr_bounce_th) {
                if (rng_float(rng) > mx) return false;
                vx.thr = vx.thr * srcp(mx + 1e-7f);
            }
        } else if (max3(vx.thr) < 1e-4f) return false;
        return true;
    }
}
// Step 2, once per light sample (sample_light, path_tracer.py:537-554; vanilla_renderer.py:68-95): `want` - the sample is worth a shadow
// ray of direction `dir`, length `dist`, carrying `contrib`; `poisoned` - its MIS weight `mis_w` is NaN (the caller stores it: upstream
// the weight multiplies the sample even when the shadow ray is occluded, 0 * NaN, so it poisons the whole pixel-sample, which is zeroed
// at the end - reproduced without tracing).  LANE_SRC: whole-record emitter loads (the class kernels only: in C2's traced kernel their
// sixteen registers cost the fourth wave, 127 -> 132 VGPRs).
struct LightSample { bool want, sampled, poisoned; f3 dir, contrib; float dist, mis_w; int src; };      // src: the emitter sampled
template <int BM, int SM, bool LANE_SRC, typename R>
APT_D LightSample sample_light(const ShadeArgs3* A_, Vertex& vx, R& rng, const EmitterGeom& geom, const DevSrc src_only, bool active, bool& break_flag) {
    LightSample ls; ls.want = ls.sampled = ls.poisoned = false; ls.dir = ls.contrib = splat3(0.f); ls.dist = 0.f; ls.mis_w = 1.0f; ls.src = 0;
    if (!active || break_flag) return ls;
    const int ns = (A_->sc).n_sources;                    // wave-uniform: one light needs no modulo
    int sidx = rng_int(rng);                            // one int is always drawn
    sidx = (ns == 1) ? 0 : pymod(sidx, ns);
    float emitter_pdf = (A_->p).inv_ns;
    if (vx.hit_light >= 0) {
        if (ns <= 1) { break_flag = true; return ls; }
        sidx = rng_int(rng);
        sidx = (ns == 2) ? 0 : pymod(sidx, ns - 1);
        if (sidx >= vx.hit_light) sidx += 1;
        emitter_pdf = (A_->p).inv_ns1;
    }
    DevSrc src = src_only;
    if (ns != 1) src = LANE_SRC ? ld_src_lane((A_->sc).src + sidx) : (A_->sc).src[sidx];
    ls.src = sidx;
    f3 shadow_int; float direct_pdf;
    const f3 to_emitter = emitter_sample_hit<SM>(src, geom, vx.hit_point, rng, shadow_int, direct_pdf) - vx.hit_point;
    ls.dist = fnorm(to_emitter);
    ls.dir = fdiv3(to_emitter, ls.dist);
    ls.sampled = true;
    const f3 direct_spec = surface_eval<BM>(vx.bx, vx.it, vx.d, ls.dir, (A_->sc).world_ior, (A_->p).two_sides);
    if ((A_->p).use_mis && !(src.bool_bits & 0x01)) ls.mis_w = balance(emitter_pdf * direct_pdf, surface_pdf<BM>(vx.bx, vx.it, ls.dir, vx.d, (A_->sc).world_ior, (A_->p).two_sides));
    if (isnan(ls.mis_w)) { ls.poisoned = true; return ls; }
    f3 c = (direct_spec * shadow_int) * ls.mis_w;
    if (ns != 1) c = fdiv3(c, emitter_pdf);               // one light: the pdf is exactly 1 and x / 1 == x (wave-uniform branch)
    ls.contrib = (c * (A_->p).inv_S) * vx.thr;
    ls.want = !(ls.contrib.x == 0.f && ls.contrib.y == 0.f && ls.contrib.z == 0.f);
    return ls;
}
// Step 3: emission of the surface the vertex is on (vanilla_renderer.py:99-104; handed to `gather`), then the continuation direction and
// the throughput behind it (vanilla_renderer.py:106-110).  The emission has to stay AFTER the light sampling: with two-sided BRDFs the
// evaluation there flips it.n_s in place, upstream as here, and eval_le sees the flipped normal.
// (pdf == 0 - a cosine-hemisphere draw of exactly 0, one in 2^24 - makes the throughput spec / 0: +inf when the rounding residue of n_s . out is
// positive, NaN when it is not; upstream lets +inf through to the pixel and zeroes NaN.  The residue hangs on the last bits of the
// un-normalised interpolated vertex normal, i.e. of the barycentrics, which the product build's intersectors return to 1e-6 and not
// to the bit: DESIGN.md section 5 "non-finite pixels".  Re-sampling such a vertex here with the reference's own triangle test was
// measured: it costs the Lambertian kernel its fourth wave per SIMD, 122 -> 130 / 158 VGPRs inline / as a loop.)
template <int BM, int SM, typename R, typename Gather>
APT_D f3 emit_and_scatter(const ShadeArgs3* A_, Vertex& vx, R& rng, float& new_pdf, bool& is_spec, Gather&& gather) {
    if ((SM & APT_SRC_AREA) && vx.hit_light >= 0) {
        const f3 emit_int = emitter_eval_le((A_->sc).src[vx.hit_light], vx.hit_point - vx.o, vx.it.n_s);
        if (!(emit_int.x == 0.f && emit_int.y == 0.f && emit_int.z == 0.f)) gather((emit_int * vx.emission_weight) * vx.thr);
    }
    f3 spec;
    const f3 new_d = surface_sample<BM>(vx.bx, vx.it, vx.d, (A_->sc).world_ior, (A_->p).two_sides, rng, spec, new_pdf, is_spec);
    vx.thr = vx.thr * fdiv3(spec, new_pdf);
    return new_d;
}
// ---- the live-row forms of steps 1 and 2 (shade_traced, LIVE): every lane of a row holds a valid record - a lane past the queue's end the
// last entry's, a path the roulette ended its own - and computes on it straight-line; `alive` masks what a dead lane must not do: vote,
// count, append, store.  Written as `if (alive) {compute} else {defaults}` the steps make the compiler give every value a dead lane "has"
// a definition (v_mov of 0 / 1.0 / -1 and the phi copies behind them: a quarter of the moves of C2's row loop), because sweeps and stores
// behind read them unconditionally.  Per live lane the arithmetic is the parent's, operation for operation.
// Draw-window vertices only (Lambertian surfaces, emitters that draw nothing): the emission MIS weight has no reader there.
// -> the vertex is still alive; where the roulette or the throughput cut ended it, rng.draw - vx.draw0 is what it drew (one word or none).
template <int BM, int SM>
APT_D bool open_vertex_live(const ShadeArgs3* A_, Vertex& vx, DrawWindow& rng, f3 rec_kd, uint32_t pm, int bounce, bool alive, const uint32_t* jitter_tail = nullptr) {
    static_assert(BM == APT_BX_LAMBERTIAN && !(SM & APT_SRC_AREA), "a draw window serves [roulette] index [index] u1 u2: Lambertian surfaces, emitters that draw nothing");
    vx.bx.k_d = rec_kd;
    const uint32_t lp = vx.id & ((1u << (A_->p).pix_bits) - 1u), s = vx.id >> (A_->p).pix_bits;
    vx.l_off = radiance_slot((A_->p), vx.id);
    vx.draw0 = (pm >> 8) & 0xffffu;
    const uint32_t key0 = ((A_->p).world == 1) ? lp : ldq((A_->p).pix_key, lp << 2), ctr0 = (uint32_t)((A_->p).cnt_base + (int)s + 1);
    bool roulette = false; float mx = 0.f;
    if ((A_->p).use_rr) { mx = max3(vx.thr); roulette = mx < (A_->p).rr_threshold && bounce >= (A_->p).rr_bounce_th; }
    else alive = alive && !(max3(vx.thr) < 1e-4f);
    const bool relight = vx.hit_light >= 0 && (A_->sc).n_sources > 1;
    const bool have_first = jitter_tail != nullptr && (A_->p).anti_alias != 0;
    uint32_t c[4] = {0u, 0u, have_first ? jitter_tail[0] : 0u, have_first ? jitter_tail[1] : 0u};
    // (the second block's vote counts the lanes the parent's branch would hold)
    const bool live = window_open(rng, key0, (A_->p).seed, ctr0, vx.draw0, roulette, mx, relight, c, have_first, [alive](bool v) { return __any(v && alive) != 0; });
    if (roulette) vx.thr = vx.thr * srcp(mx + 1e-7f);
    return alive && live;
}
template <int BM, int SM, typename R>
APT_D LightSample sample_light_live(const ShadeArgs3* A_, Vertex& vx, R& rng, const EmitterGeom& geom, const DevSrc src_only, bool active) {
    LightSample ls;
    const int ns = (A_->sc).n_sources;
    int sidx = rng_int(rng);
    sidx = (ns == 1) ? 0 : pymod(sidx, ns);
    float emitter_pdf = (A_->p).inv_ns;
    if (ns <= 1) active = active && vx.hit_light < 0;        // on the scene's only light: one index drawn, nothing sampled
    else if (vx.hit_light >= 0) {
        sidx = rng_int(rng);
        sidx = (ns == 2) ? 0 : pymod(sidx, ns - 1);
        if (sidx >= vx.hit_light) sidx += 1;
        emitter_pdf = (A_->p).inv_ns1;
    }
    DevSrc src = src_only;
    if (ns != 1) src = (A_->sc).src[sidx];
    ls.src = sidx;
    f3 shadow_int; float direct_pdf;
    const f3 to_emitter = emitter_sample_hit<SM>(src, geom, vx.hit_point, rng, shadow_int, direct_pdf) - vx.hit_point;
    ls.dist = fnorm(to_emitter);
    ls.dir = fdiv3(to_emitter, ls.dist);
    ls.sampled = active;
    const f3 direct_spec = surface_eval<BM>(vx.bx, vx.it, vx.d, ls.dir, (A_->sc).world_ior, (A_->p).two_sides);
    ls.mis_w = 1.0f;
    if ((A_->p).use_mis && !(src.bool_bits & 0x01)) ls.mis_w = balance(emitter_pdf * direct_pdf, surface_pdf<BM>(vx.bx, vx.it, ls.dir, vx.d, (A_->sc).world_ior, (A_->p).two_sides));
    ls.poisoned = active && isnan(ls.mis_w);
    f3 c = (direct_spec * shadow_int) * ls.mis_w;
    if (ns != 1) c = fdiv3(c, emitter_pdf);
    ls.contrib = (c * (A_->p).inv_S) * vx.thr;
    ls.want = active && !ls.poisoned && !(ls.contrib.x == 0.f && ls.contrib.y == 0.f && ls.contrib.z == 0.f);
    return ls;
}
// a shadow-queue entry (k_shadow / shadow_flat_body read these planes)
APT_D void shadow_store(const Queues& q, uint32_t so, f3 o, f3 dir, float dist, f3 contrib) {
    st3q(q.sh_o, q.sh_cap, so, o); st3q(q.sh_d, q.sh_cap, so, dir); stq(q.sh_tmax, so, dist); st3q(q.sh_c, q.sh_cap, so, contrib);
}
struct ShadeTally { uint32_t shade, shadow, poison; };          // wave-uniform tallies (SGPRs); the RNG draws of a wave are tallied in LDS (s_draws): a per-lane tally would hold a VGPR for the whole kernel
APT_D void tally_flush(const ShadeTally& t, const uint32_t* s_draws, Counters* cnt, int sq) {
    flush_uniform(t.shade, &cnt->stats[sq][ST_SHADE]);
    flush_uniform(t.shadow, &cnt->stats[sq][ST_SHADOW]);
    if (lane_id() == 0 && s_draws[threadIdx.x >> 6]) atomicAdd(&cnt->stats[sq][ST_DRAWS], (unsigned long long)s_draws[threadIdx.x >> 6]);
    flush_uniform(t.poison, &cnt->stats[sq][ST_POISON]);
}
#if APT_FAST
// ---- the shade kernel that traces its own rays (Params::traced: "rays traced in place" above).  Input and output are the packed
// records of Queues::tr; the path's radiance travels with it (Lc) and reaches its slot of L once, when the path ends.
// For a scene of a few dozen records the any-hit sweep of a shadow ray costs fewer issue slots than the round trip of its 44-byte queue
// entry through HBM plus the scattered read-modify-write of the path's radiance slot behind it: the vertex's light sample is swept right
// here (one ray per lane against two records per packed instruction, traverse.hpp flat_any1), after the continuation has been sampled and
// traced, when little else is live.  The rare rays whose answer needs the reference-order sweep (flat_needs_cull) still leave as
// shadow-queue entries, counted by n_fix_sh[cur], and are served by the next launch's prologue.
// A row is a sequence of phases, each a function below, in the order shade_traced takes them; the forms of the kernel - CAM, STAGE, LIVE -
// differ in which function a phase is.  (Lane flags leave a phase as its return value: a bool behind a reference stays a byte in a lane
// register instead of a mask in scalar ones - measured: up to ten vector instructions of a lean kernel's row loop.)
//
// ROW HEAD, the queue-fed forms.  The record of the row at `b` that this lane reads: its own, or past the queue's end the last entry's
// (never used; LIVE: shaded with its effects masked) - no address leaves the sub-queue's region.
APT_D uint32_t row_lane(uint32_t b, uint32_t n) { return min(b + threadIdx.x, n - 1u); }
struct RecordPlanes { const float4 *a, *b, *c, *d; };             // planes A to D of the queue a launch reads (Queues::tr[cur])
// PFP: the next row's packed word - hit primitive, draw index, specular flag - is requested one row ahead (one register), so that a row's
// shading record can be requested together with its queue record instead of a round trip after it.  (Rounds 2-4 prefetched the Lambertian
// kernel's whole record: thirteen registers.  Without them the kernel allocates 91 VGPRs - five waves per SIMD instead of four - and three
// render lanes gain 6 %: C2 4 310 -> 4 560 Msamples/s on the same box.)
template <bool C56 = false>
APT_D uint32_t prefetch_prim(const RecordPlanes& tr, uint32_t qbase, uint32_t b, uint32_t n) { return ldq(TrRecord<C56>::pm_plane(tr.a, tr.b), ((qbase + row_lane(b, n)) << 4) + 12u); }
// STAGE, the staged record (queue-fed form only): a row's record - planes A to D, 64 entries of 16 bytes each: 1 KiB per
// plane and wave - is requested a row AHEAD, by loads that write LDS directly (global_load_lds_dwordx4: no register holds the data in
// flight), into 4 KiB that the wave owns; the scene's shading records (at most 96 x 32 bytes) sit in LDS too, one copy per workgroup.
// A row then opens with LDS reads only - its lane's four words into the registers the direct loads fill, the shading record of the hit
// primitive, which arrives with plane B (the word requested ahead on its own, PFP, and its register are gone) - and waits on no
// vector memory: the next row's loads are issued behind the light sample, in front of the two sweeps, and waited for at the end of
// the row, before its stores (a wait at the next row's top would also wait for those stores to be acknowledged: one in-order counter).
// Nothing is staged for an empty sub-queue or behind the last row.  STAGE = false is the kernel with the direct loads, instruction for instruction.
struct StagedRecord { rec4* rec; rec4* prim; };                   // plane k of this wave's row at rec[64 * k + lane]; the shading records (DevScene::prim_shade)
// (the 56-byte record, C56: 3.5 KiB per wave, laid out by thread - stages.hpp staged_read56 - and `rec` is the workgroup's area: plane k of
// the row of thread t at rec[BLOCK * k + t], plane D's two words as word planes behind plane C)
template <bool C56 = false>
APT_D StagedRecord staged_record_open(const ShadeArgs3* A_) {      // (before the prologue: every wave of the workgroup passes here, none has a staged load in flight)
    constexpr int WAVE_RECS = C56 ? 3 * 64 + 32 : 4 * 64;
    __shared__ rec4 s_stage[(BLOCK / 64) * WAVE_RECS]; __shared__ rec4 s_shade[2 * APT_FLAT_MAX_PRIMS];
    static_assert(2 * APT_FLAT_MAX_PRIMS <= BLOCK, "one shading-record word per thread");
    if ((int)threadIdx.x < 2 * min((A_->sc).n_prims, APT_FLAT_MAX_PRIMS)) { const float4 w_ = (A_->sc).prim_shade[threadIdx.x]; s_shade[threadIdx.x] = rec4{w_.x, w_.y, w_.z, w_.w}; }
    __syncthreads();
    return StagedRecord{s_stage + (C56 ? 0 : (threadIdx.x >> 6) * WAVE_RECS), s_shade};
}
template <bool C56 = false>
APT_D void stage_row(const StagedRecord& s, const RecordPlanes& tr, uint32_t qbase, uint32_t b, uint32_t n, int bounce) {      // (wave-uniform: b < n)
    const uint32_t off = (qbase + row_lane(b, n)) << 4;
    if constexpr (C56) {
        rec4* row = s.rec + (threadIdx.x >> 6) * 64;
        stage_plane(tr.a, off, row); stage_plane(tr.b, off, row + BLOCK); stage_plane(tr.c, off, row + 2 * BLOCK);
        // (plane D, 8 bytes per entry: its two words, 64 lanes of 4 bytes each)
        if (bounce > 0) { float* w_ = reinterpret_cast<float*>(s.rec + 3 * BLOCK) + (threadIdx.x >> 6) * 64; stage_word(reinterpret_cast<const float*>(tr.d), off >> 1, w_); stage_word(reinterpret_cast<const float*>(tr.d), (off >> 1) + 4u, w_ + BLOCK); }
        return;
    }
    stage_plane(tr.a, off, s.rec); stage_plane(tr.b, off, s.rec + 64); stage_plane(tr.c, off, s.rec + 128);
    if (bounce > 0) stage_plane(tr.d, off, s.rec + 192);
}
// this lane's words of the row's record and the shading record of its hit primitive (plane D's words are read at bounce 0 too, where
// nothing was staged into them: never used)
template <bool C56 = false>
APT_D void staged_row_read(const StagedRecord& s, float4& a, float4& b, float4& c, float4& d, float4& ra, float4& rb) {
    rec4 sa, sb, sc_, sd, pa, pb;
    if constexpr (C56) { float d0, d1; staged_read56(s.rec, sa, sb, sc_, d0, d1); sd = rec4{d0, d1, 0.f, 0.f}; }
    else staged_read(s.rec + lane_id(), sa, sb, sc_, sd);
    staged_read2(s.prim + 2 * max(tr_prim(__float_as_uint(C56 ? sa.w : sb.w)), 0), pa, pb);
    a = make_float4(sa.x, sa.y, sa.z, sa.w); b = make_float4(sb.x, sb.y, sb.z, sb.w); c = make_float4(sc_.x, sc_.y, sc_.z, sc_.w); d = make_float4(sd.x, sd.y, sd.z, sd.w);
    ra = make_float4(pa.x, pa.y, pa.z, pa.w); rb = make_float4(pb.x, pb.y, pb.z, pb.w);
}
// staged_wait; in the diagnostic build -DAPT_ROWTOP_STATS=1 between two stamps: per wave, the clock ticks spent waiting for its rows'
// records (stats[12]), those of the row loop (stats[13]) and the rows (stats[14])
struct RowTop { unsigned long long wait, rows, loop0; };
APT_D void staged_wait_stamped(RowTop& rt, bool row) {
#ifdef APT_ROWTOP_STATS
    const unsigned long long t0_ = __builtin_amdgcn_s_memtime(); staged_wait(); rt.wait += __builtin_amdgcn_s_memtime() - t0_; rt.rows += row ? 1u : 0u;
#else
    staged_wait();
#endif
}
// a vertex's draws into the wave's tally; UNORDERED (the kernels that stage their record): by an LDS add that waits for no staged load
template <bool UNORDERED> APT_D void tally_draws(uint32_t* s_draws, uint32_t n) { if constexpr (UNORDERED) lds_add_unordered(&s_draws[threadIdx.x >> 6], n); else atomicAdd(&s_draws[threadIdx.x >> 6], n); }
// planes A to C of a record -> the vertex's ray, throughput and path id (A.w, the hit distance, and B.w, the packed word, go to the hit)
// (the 56-byte record, C56: plane A's point is the vertex itself - vx.hit_point; the ray's origin did not travel and has no reader)
template <bool C56 = false>
APT_D void unpack_record(float4 a, float4 b, float4 c, Vertex& vx) {
    if constexpr (C56) vx.hit_point = mk3(a.x, a.y, a.z); else vx.o = mk3(a.x, a.y, a.z);
    vx.d = mk3(b.x, b.y, b.z); vx.thr = mk3(c.x, c.y, c.z); vx.id = TrRecord<C56>::id(b, c);
}
// a record's words -> its opened vertex; false: the path ends here.  pm: the packed word; REC: ra, rb hold the hit primitive's shading record
template <int BM, int SM, int TEX, bool REC, bool C56 = false, typename RNG>
APT_D bool open_record(const ShadeArgs3* A_, Vertex& vx, RNG& rng, float4 a, float4 b, float4 c, uint32_t pm, float4 ra, float4 rb, int cur, uint32_t idx, float ray_pdf, int bounce) {
    static_assert(!C56 || REC, "the 56-byte record's kernels hold the hit primitive's shading record");
    unpack_record<C56>(a, b, c, vx);
    const int prim = tr_prim(pm);
    if (prim < 0) return false;                              // nothing hit: path ends (vanilla_renderer.py:49)
    f3 rec_kd; float2 uv; uv.x = uv.y = 0.f;
    if ((A_->sc).has_vn || (TEX && (A_->sc).tex_i != nullptr)) uv = ldq((A_->q).tr_uv[cur], idx << 3);      // otherwise nobody reads the barycentrics (and nobody wrote them)
    if constexpr (C56) build_hit_rec<true>((A_->sc), ra, rb, prim, 0.f, uv.x, uv.y, vx.hit_point, vx.d, vx.it, vx.hit_light, rec_kd);
    else if (REC) build_hit_rec((A_->sc), ra, rb, prim, a.w, uv.x, uv.y, vx.o, vx.d, vx.it, vx.hit_light, rec_kd);
    else build_hit((A_->sc), prim, a.w, uv.x, uv.y, vx.o, vx.d, vx.it, vx.hit_light, rec_kd);
    return open_vertex<BM, SM, TEX>(A_, vx, rng, prim, rec_kd, tr_meta(pm, (uint32_t)bounce), ray_pdf, uv, bounce);
}
// LIVE, live rows (the staged and the camera-fed form of the lean kernels): every lane of a row shades a valid record
// straight-line - a lane past the queue's end the last entry's, which it staged; a lane past the id space's end the ray of its pixel; a
// path the roulette ended its own - and `alive` masks effects only: votes, tallies, appends, stores (open_vertex_live, sample_light_live
// above).  vertex_reset is no default provider there: what it writes is overwritten for every lane, or a constant of the Lambertian
// kernel.  At the last bounce the continuation is not sampled; `draw` moves on by its two words.  LIVE = false is the parent's kernel,
// instruction for instruction.
template <int BM, int SM, bool C56 = false, typename RNG>
APT_D bool open_record_live(const ShadeArgs3* A_, Vertex& vx, RNG& rng, float4 a, float4 b, float4 c, float4 d, float4 ra, float4 rb, int cur, uint32_t idx, int bounce, bool alive, uint32_t* s_draws, f3& Lc) {
    if (bounce > 0) Lc = TrRecord<C56>::Lc(c, d);
    unpack_record<C56>(a, b, c, vx);
    const uint32_t pm = TrRecord<C56>::pm(a, b); const int prim = tr_prim(pm);
    alive = alive && prim >= 0;                              // nothing hit: path ends (vanilla_renderer.py:49)
    f3 rec_kd; float2 uv; uv.x = uv.y = 0.f;
    if ((A_->sc).has_vn) { if (alive) uv = ldq((A_->q).tr_uv[cur], idx << 3); }
    if constexpr (C56) build_hit_rec<true>((A_->sc), ra, rb, max(prim, 0), 0.f, uv.x, uv.y, vx.hit_point, vx.d, vx.it, vx.hit_light, rec_kd);
    else build_hit_rec((A_->sc), ra, rb, max(prim, 0), a.w, uv.x, uv.y, vx.o, vx.d, vx.it, vx.hit_light, rec_kd);
    const bool opened = alive; alive = open_vertex_live<BM, SM>(A_, vx, rng, rec_kd, pm, bounce, alive);
    if (opened && !alive && rng.draw != vx.draw0) tally_draws<true>(s_draws, rng.draw - vx.draw0);      // the roulette's word of a path it ended
    return alive;
}
// CAM, the camera-fed form (steady full-film batches): bounce 0 with no queue in front of it.  Every slot of the id space is
// a live camera ray then, so a row MAKES its 64 records instead of loading them - pixel, jitter, direction, the slot's radiance zeroed, the
// sweep against the strip's records, all as k_generate_trace does them (stages.hpp camera_ray_dir / camera_strip_mask) - and shades the hits
// in the same registers: the camera ray's 64-byte record is neither written nor read back, and k_generate_trace's launch is gone.  Row `pos`
// of sub-queue q is id-space wave (pos / 64) * nq + q, the mapping of generate_body, so a wave holds 64 consecutive local pixels and the
// strip-mask rule holds as it stands; the row count is a closed form, no counter is read.  Camera rays the sweep cannot settle are staged
// exactly as k_generate_trace stages them (top of the sub-queue's region of tr[0], n_tr[0][ncls]); the ordinary bounce-0 launch that
// follows resolves them in its prologue and shades that handful.  This kernel runs no prologue: nothing is listed before it.
// Its light samples all leave from what the wave's strip sees: where the wave's emitter is uniform they are swept against the pairs of
// its occluder list that the strip's mask keeps (flat_build.cpp light_strips; the masks lie behind the strip lists in `strips`).
APT_D uint32_t cam_wave(const ShadeArgs3* A_, uint32_t pos, int q) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)(pos >> 6)) * (uint32_t)(A_->p).nq + (uint32_t)q; }      // (wave-uniform: scalar registers)
// slot `id_` of the id space -> its sample and pixel, the path's id word; `zero`: the slot's radiance is zeroed
APT_D uint32_t cam_path(const ShadeArgs3* A_, uint32_t id_, bool zero, uint32_t& s, int& i, int& j) {
    const uint32_t lp = id_ % (uint32_t)(A_->p).npix; s = id_ / (uint32_t)(A_->p).npix;
    local_to_global((A_->p), lp, i, j);
    if (zero) for (int pl = 0; pl < (A_->p).l_planes; pl++) stL((A_->q).L, (A_->p).cap, (id_ << 2) | (uint32_t)pl, splat3(0.f));
    return (s << (A_->p).pix_bits) | lp;
}
// the camera ray against the records of its strip (id-space wave w) -> c_idx, c_t; true: the ray is left to the reference-order code
APT_D bool cam_sweep(const ShadeArgs3* A_, const unsigned long long* strips, uint32_t w, bool valid, f3 cam_o, f3 dir, float& c_t, int& c_idx) {
    int c_run = -1; c_t = 0.f; c_idx = -1;
    if (__any(valid)) c_idx = flat_closest1<true>((A_->sc).flat, cam_o, dir, 1e7f, c_t, c_run, camera_strip_mask((A_->p), strips, w));
    return valid && (c_run >= 0 || flat_needs_cull((A_->sc).flat, dir));
}
// a camera ray left to the reference-order code is staged.  The words the two callers store differently come from `words`, called in the
// rare branch, where their register notes want them made: A.w; B.w's primitive; the barycentrics; planes C (one, one, one, id) and D (zero, zero, zero, one_d)
struct StagedRayWords { float t; int prim; float u, v, one, zero, one_d; };
template <bool C56 = false, typename Words>
APT_D void stage_camera_ray(const ShadeArgs3* A_, Counters* cnt, int q, uint32_t qbase, bool c_defer, f3 cam_o, f3 dir, uint32_t draws, uint32_t id, Words&& words) {
    if (!__any(c_defer)) return;
    const int ncls = (A_->q).tr_ncls; const uint32_t dpos = wave_append(c_defer, &cnt->n_tr[0][ncls][q * CNT_PAD]);
    if (c_defer) {
        const uint32_t slot = (A_->q).tr_stage_top ? qbase + (A_->p).subcap - 1u - dpos : (uint32_t)ncls * (A_->p).cap + qbase + dpos;
        const StagedRayWords w = words();
        typedef TrRecord<C56> Rec;
        auto pm = [&] { return tr_pack(w.prim, draws, false); };
        Rec::put_a((A_->q).tr[0][0], slot, cam_o, w.t, pm);
        Rec::put_b((A_->q).tr[0][1], slot, dir, pm, id);
        Rec::put_c((A_->q).tr[0][2], slot, mk3(w.one, w.one, w.one), id, mk3(w.zero, w.zero, w.zero));
        if constexpr (!C56) Rec::put_d((A_->q).tr[0][3], slot, mk3(w.zero, w.zero, w.zero), w.one_d);      // (56 bytes: a camera ray has no plane D, stages.hpp TrRecord)
        if ((A_->sc).has_vn || (A_->sc).tex_i != nullptr) { float2 uv_; uv_.x = w.u; uv_.y = w.v; stq((A_->q).tr_uv[0], slot << 3, uv_); }
    }
}
// the camera vertex: the ray is made, swept against its strip's records and, where that settles it, shaded right here.
// -> alive; entry: the lane holds a path this launch shades (valid, not left to the reference-order code)
template <int BM, int SM, int TEX, bool WINDOW, bool C56 = false, typename RNG>
APT_D bool camera_vertex(const ShadeArgs3* A_, Counters* cnt, int q, uint32_t qbase, uint32_t pos, bool in_row, uint32_t cam_total, const unsigned long long* strips, Vertex& vx, RNG& rng, uint32_t* s_draws, uint32_t& t_samples, uint32_t& t_extend, bool& entry) {
    const uint32_t w = cam_wave(A_, pos, q), id_ = w * 64u + lane_id(); const bool valid = in_row && id_ < cam_total;
    f3 dir = mk3(0.f, 0.f, 1.f); uint32_t draws = 0, jitter_tail[2] = {0u, 0u};
    if (valid) { uint32_t s; int i, j; vx.id = cam_path(A_, id_, true, s, i, j); dir = camera_ray_dir((A_->p), i, j, s, draws, WINDOW ? jitter_tail : nullptr); }
    if (draws) atomicAdd(&s_draws[threadIdx.x >> 6], draws);      // (the jitter's draws: k_generate_trace's share of ST_DRAWS)
    const f3 cam_o = mk3((A_->p).cam_t[0], (A_->p).cam_t[1], (A_->p).cam_t[2]);
    float c_t; int c_idx, hit_cls = 0;
    const bool c_defer = cam_sweep(A_, strips, w, valid, cam_o, dir, c_t, c_idx);
    HitRec hr; hr.t = 1e7f; hr.prim = -1; hr.u = hr.v = 0.f;
    if (valid && !c_defer && c_idx >= 0) flat_resolve((A_->sc).flat, c_idx, c_t, cam_o, dir, hr, hit_cls);
    { const uint32_t nv = wave_count(valid); t_samples += nv; t_extend += nv; }
    stage_camera_ray<C56>(A_, cnt, q, qbase, c_defer, cam_o, dir, draws, vx.id, [&] {
        float one = 1.f;
        if (WINDOW && !C56) asm volatile("" : "+v"(one));      // (made here, in the rare branch: as a constant, (0, 0, 0, 1) is hoisted in front of the row loop, where the draw-window kernel has no four registers for it - 72 VGPRs and a 16-byte spill)
        float zero = 0.f;
        if constexpr (C56) { if (WINDOW) asm volatile("" : "+v"(zero)); }      // (the 56-byte record's plane D is (zero, zero): hoisted and spilled likewise)
        return StagedRayWords{hr.t, C56 ? -1 : hr.prim, hr.u, hr.v, 1.f, zero, one};      // (a staged ray was not resolved: its hit record is the empty one)
    });
    entry = valid && !c_defer; bool alive = entry && hr.prim >= 0;                       // nothing hit: the path ends where it began, nothing gathered
    if (alive) {
        vx.o = cam_o; vx.d = dir; vx.thr = splat3(1.f);
        f3 rec_kd; float2 uv; uv.x = hr.u; uv.y = hr.v;
        build_hit((A_->sc), hr.prim, hr.t, uv.x, uv.y, vx.o, vx.d, vx.it, vx.hit_light, rec_kd);
        alive = open_vertex<BM, SM, TEX>(A_, vx, rng, hr.prim, rec_kd, tr_meta(tr_pack(hr.prim, draws, false), 0u), 1.f, uv, 0, WINDOW ? jitter_tail : nullptr);
    }
    return alive;
}
// ... live rows: a lane past the id space's end makes the ray of its pixel (a pixel of the film all the same, a sample no batch holds), and
// a ray that hit nothing or is left to the reference-order code is shaded on whatever record the resolve gives it; `valid`, `c_defer`, `alive` mask the effects
template <int BM, int SM, bool WINDOW, bool C56 = false, typename RNG>
APT_D bool camera_vertex_live(const ShadeArgs3* A_, Counters* cnt, int q, uint32_t qbase, uint32_t pos, bool in_row, uint32_t cam_total, const unsigned long long* strips, Vertex& vx, RNG& rng, uint32_t* s_draws, uint32_t& t_samples, uint32_t& t_extend, bool& entry) {
    const uint32_t w = cam_wave(A_, pos, q), id_ = w * 64u + lane_id(); const bool valid = in_row && id_ < cam_total;
    uint32_t draws = 0, jitter_tail[2] = {0u, 0u}, s; int i, j;
    vx.id = cam_path(A_, id_, valid, s, i, j);
    const f3 dir = camera_ray_dir((A_->p), i, j, s, draws, WINDOW ? jitter_tail : nullptr);
    if (valid && draws) atomicAdd(&s_draws[threadIdx.x >> 6], draws);      // (the jitter's draws: k_generate_trace's share of ST_DRAWS)
    const f3 cam_o = mk3((A_->p).cam_t[0], (A_->p).cam_t[1], (A_->p).cam_t[2]);
    float c_t; int c_idx, hit_cls = 0;
    const bool c_defer = cam_sweep(A_, strips, w, valid, cam_o, dir, c_t, c_idx);
    HitRec hr;
    flat_resolve((A_->sc).flat, max(c_idx, 0), c_t, cam_o, dir, hr, hit_cls);
    { const uint32_t nv = wave_count(valid); t_samples += nv; t_extend += nv; }
    stage_camera_ray<C56>(A_, cnt, q, qbase, c_defer, cam_o, dir, draws, vx.id, [&] {      // with an empty hit record
        float one = 1.f, far_ = 1e7f, zero = 0.f;
        if constexpr (C56) asm volatile("" : "+v"(one), "+v"(zero));      // (the 56-byte record carries no hit distance)
        else asm volatile("" : "+v"(one), "+v"(far_), "+v"(zero));      // (made here, in the rare branch: as constants the words are hoisted in front of the row loop and spilled there, see camera_vertex)
        return StagedRayWords{far_, -1, zero, zero, one, zero, one};
    });
    entry = valid && !c_defer; bool alive = entry && c_idx >= 0 && hr.prim >= 0;          // nothing hit: the path ends where it began, nothing gathered
    vx.o = cam_o; vx.d = dir; vx.thr = splat3(1.f);
    f3 rec_kd; build_hit((A_->sc), max(hr.prim, 0), hr.t, hr.u, hr.v, vx.o, vx.d, vx.it, vx.hit_light, rec_kd);
    const bool opened = alive; alive = open_vertex_live<BM, SM>(A_, vx, rng, rec_kd, tr_pack(hr.prim, draws, false), 0, alive, WINDOW ? jitter_tail : nullptr);
    if (opened && !alive && rng.draw != vx.draw0) tally_draws<false>(s_draws, rng.draw - vx.draw0);      // the roulette's word of a path it ended
    return alive;
}
// ROW TAIL.  Emission of the surface the vertex is on, then the continuation (emit_and_scatter): new_d, its direction; -> a continuation
// ray leaves.  The vertex's draws join the wave's tally (LDS_TALLY: tally_draws' unordered form).
template <int BM, int SM, bool LDS_TALLY, typename RNG>
APT_D bool scatter(const ShadeArgs3* A_, Vertex& vx, RNG& rng, bool alive, int bounce, uint32_t* s_draws, f3& Lc, f3& new_d, float& new_pdf, bool& is_spec) {
    bool cont = false;
    if (alive) { new_d = emit_and_scatter<BM, SM>(A_, vx, rng, new_pdf, is_spec, [&](f3 add) { Lc = Lc + add; }); cont = (bounce + 1) < (A_->p).max_bounce; }
    if (rng.draw != vx.draw0) tally_draws<LDS_TALLY>(s_draws, rng.draw - vx.draw0);      // also paths that died in the roulette
    return cont;
}
// ... live rows: the last bounce's continuation has no reader, its two words are passed over (wave-uniform)
template <int BM, int SM, bool LDS_TALLY, typename RNG>
APT_D bool scatter_live(const ShadeArgs3* A_, Vertex& vx, RNG& rng, bool alive, int bounce, uint32_t* s_draws, f3& Lc, f3& new_d, float& new_pdf, bool& is_spec) {
    bool cont = false;
    if ((bounce + 1) < (A_->p).max_bounce) { new_d = emit_and_scatter<BM, SM>(A_, vx, rng, new_pdf, is_spec, [&](f3 add) { Lc = Lc + add; }); cont = alive; }
    else rng.draw += 2u;
    if (alive) tally_draws<LDS_TALLY>(s_draws, rng.draw - vx.draw0);
    return cont;
}
// The records the row's light samples are swept against (traverse.hpp flat_occ_list): the occluder list of the emitter that every lane of
// the wave that wants a sample has sampled - the only one in a single-emitter scene - else the full stream (-1).  Decided before the
// continuation, wave-uniform (scalar registers), so that the emitter index is not held in a lane register until the sweep.
APT_D int pick_occluder_list(const ShadeArgs3* A_, const LightSample& f) {
    int occ_e = 0;
    if ((A_->sc).n_sources != 1) {
        const unsigned long long wm = __ballot(f.want);
        occ_e = -1;
        if (wm != 0ull) { const int e0 = __builtin_amdgcn_readlane(f.src, __ffsll((long long)wm) - 1); if (!__any(f.want && f.src != e0)) occ_e = e0; }
    }
    return occ_e;
}
// The continuation ray meets the scene's records.  Only rays that hit something (or whose answer is left to the reference-order code:
// listed, with a provisional record) enter the next queue (-> true); the tail atomic is on its way while the light sample is swept.
struct Continuation { float t, u, v; int hit, q; TrAppend app; };      // hit distance, barycentrics, primitive; q: the queue the record joins (0; 1: the staging area at the top of its sub-queue's region; -1: none); its append ticket
APT_D bool trace_continuation(const ShadeArgs3* A_, const Vertex& vx, f3 new_d, bool cont, uint32_t* next_counter, uint32_t& t_extend, Continuation& ct) {
    ct.t = 0.f; ct.hit = -1; ct.u = ct.v = 0.f; int tr_idx = -1, tr_run = -1, hit_cls = 0;
    if (__any(cont)) tr_idx = flat_closest1((A_->sc).flat, vx.hit_point, new_d, 1e7f, ct.t, tr_run);
    const bool tr_defer = cont && (tr_run >= 0 || flat_needs_cull((A_->sc).flat, new_d));
    t_extend += wave_count(cont);
    cont = cont && (tr_idx >= 0 || tr_defer);
    if (cont && !tr_defer) { HitRec hr; flat_resolve((A_->sc).flat, tr_idx, ct.t, vx.hit_point, new_d, hr, hit_cls); ct.hit = hr.prim; ct.u = hr.u; ct.v = hr.v; }
    ct.q = !cont ? -1 : (tr_defer ? 1 : 0);
    const Append a_ = append_issue(ct.q == 0, next_counter); ct.app.raw = a_.raw; ct.app.rank = rank_in(a_.m);      // (a staged ray - rare - moves the staging queue's tail by itself: append_record)
    return cont;
}
// The row's light sample, swept in place against the list pick_occluder_list chose and added to Lc; a ray that needs the reference-order
// sweep leaves as a shadow-queue entry for the next launch's prologue.  CAM: the pairs of the emitter's list that cannot lie between the
// patch of surfaces the strip sees and the light are skipped (the mask is fetched here, scalar loads).
template <bool CAM>
APT_D void sweep_light_sample(const ShadeArgs3* A_, Counters* cnt, const Vertex& vx, const LightSample& f, int occ_e, int cur, int q, uint32_t sh_qbase, uint32_t pos, const unsigned long long* strips, f3& Lc, uint32_t& t_traced, uint32_t& t_lit) {
    const bool defer = f.want && flat_needs_cull((A_->sc).flat, f.dir); bool occ = false;
    if (__any(f.want && !defer)) {
        const FlatList ls = (occ_e >= 0) ? flat_occ_list((A_->sc).flat, occ_e) : flat_full_list((A_->sc).flat);
        if constexpr (CAM) {
            unsigned long long lmask = ~0ull;
            if (occ_e >= 0 && occ_e < APT_LIGHT_STRIP_EMITTERS) lmask = light_strip_mask((A_->p), strips, cam_wave(A_, pos, q), occ_e);
            occ = flat_any1<true>(ls, vx.hit_point, f.dir, shadow_limit(f.dist), lmask);
        } else occ = flat_any1(ls, vx.hit_point, f.dir, shadow_limit(f.dist));
    }
    if (__any(defer)) {
        const uint32_t spos = wave_append(defer, &cnt->n_fix_sh[cur][q * CNT_PAD]);
        if (defer && spos < (A_->q).sh_subcap) { const uint32_t so = (sh_qbase + spos) << 2; shadow_store((A_->q), so, vx.hit_point, f.dir, f.dist, f.contrib); stq((A_->q).sh_id, so, vx.l_off); }
    }
    const bool traced = f.want && !defer;
    if (traced) {
        // (an occluded sample still enters upstream's sum as 0 * contribution: NaN for a non-finite one, see k_shadow)
        const bool weird = !(isfinite(f.contrib.x) && isfinite(f.contrib.y) && isfinite(f.contrib.z));
        if (!occ || weird) Lc = Lc + (occ ? f.contrib * 0.f : f.contrib);
    }
    t_traced += wave_count(f.want); t_lit += wave_count(traced && !occ);
}
// the continuation's record joins the next queue; the path's radiance so far (Lc) travels with it
// (the 56-byte record, C56: the NEXT vertex - this ray's hit point, made here from what the reader would have loaded; a staged ray keeps its origin)
// TURN (56 bytes): a staged ray's position is turned round in its rare branch and the row has one slot expression, instead of a select in
// the row.  Which of the two the compiler makes the shorter row loop of differs by kernel (the scalar registers it keeps in lanes move):
// the camera-fed form without live rows takes this one, the other four the select (tests/test_kernel_record_compact.py holds all five).
template <bool C56 = false, bool TURN = false>
APT_D void append_record(const ShadeArgs3* A_, int nxt, uint32_t qbase, uint32_t* next_counter, const Continuation& ct, bool cont, const Vertex& vx, f3 new_d, uint32_t draw, bool is_spec, f3 Lc, float new_pdf) {
    uint32_t npos = (uint32_t)__builtin_amdgcn_readlane((int)ct.app.raw, 0) + ct.app.rank;
    auto pm = [&] { return tr_pack(ct.hit, draw, is_spec); };
    if constexpr (C56) {
        // a staged ray's plane A - its origin - is stored in the rare branch, whole; behind it the vertex's own position has no reader left
        typedef TrRecord<true> Rec;
        if (__any(ct.q == 1)) {
            const uint32_t dpos = wave_append(ct.q == 1, next_counter + APT_MAX_NQ * CNT_PAD);
            if (ct.q == 1) { npos = TURN ? (A_->p).subcap - 1u - dpos : dpos; Rec::put_a((A_->q).tr[nxt][0], qbase + (A_->p).subcap - 1u - dpos, vx.hit_point, ct.t, [&] { return tr_pack(-1, draw, is_spec); }); }      // (no hit yet)
        }
        const uint32_t slot = (!TURN && ct.q == 1) ? qbase + (A_->p).subcap - 1u - npos : qbase + npos;      // (staged rays grow down from the top of the sub-queue's region)
        float t_hit = ct.t;
        asm volatile("" : "+v"(t_hit));      // (the point is made HERE, into the registers of the vertex's own: made ahead of the light sample's sweep it costs three registers the budget does not have)
        // (a resolved ray has its primitive: the packed word needs no "nothing hit" test here - the staged rays' word was made above)
        if (ct.q == 0) Rec::put_a((A_->q).tr[nxt][0], slot, hit_point_of(vx.hit_point, new_d, t_hit), t_hit, [&] { return (uint32_t)ct.hit | ((draw & 0xffffu) << 8) | (is_spec ? (1u << 24) : 0u); });
        if (cont) {
            Rec::put_b((A_->q).tr[nxt][1], slot, new_d, pm, vx.id);
            Rec::put_c((A_->q).tr[nxt][2], slot, vx.thr, vx.id, Lc); Rec::put_d((A_->q).tr[nxt][3], slot, Lc, new_pdf);
            if ((A_->sc).has_vn || (A_->sc).tex_i != nullptr) { float2 uv_; uv_.x = ct.u; uv_.y = ct.v; stq((A_->q).tr_uv[nxt], slot << 3, uv_); }
        }
        return;
    }
    if (__any(ct.q == 1)) { const uint32_t dpos = wave_append(ct.q == 1, next_counter + APT_MAX_NQ * CNT_PAD); if (ct.q == 1) npos = dpos; }
    if (cont) {
        const uint32_t slot = (ct.q == 1) ? qbase + (A_->p).subcap - 1u - npos : qbase + npos;      // (staged rays grow down from the top of the sub-queue's region)
        typedef TrRecord<false> Rec;
        Rec::put_a((A_->q).tr[nxt][0], slot, vx.hit_point, ct.t, pm); Rec::put_b((A_->q).tr[nxt][1], slot, new_d, pm, vx.id);
        Rec::put_c((A_->q).tr[nxt][2], slot, vx.thr, vx.id, Lc); Rec::put_d((A_->q).tr[nxt][3], slot, Lc, new_pdf);
        if ((A_->sc).has_vn || (A_->sc).tex_i != nullptr) { float2 uv_; uv_.x = ct.u; uv_.y = ct.v; stq((A_->q).tr_uv[nxt], slot << 3, uv_); }
    }
}
// the path ends here (nothing hit, roulette, last bounce): its radiance goes to its slot - added, not stored: the prologue may have put a deferred sample's share there already
APT_D void end_path(const ShadeArgs3* A_, bool ended, uint32_t id, f3 Lc) { if (ended && !(Lc.x == 0.f && Lc.y == 0.f && Lc.z == 0.f)) add_radiance((A_->q).L, (A_->p).cap, radiance_slot((A_->p), id), Lc, true); }
// C56: the launch reads and writes the 56-byte record (stages.hpp TrRecord: the hit point travels, origin, distance and pdf do not); C56 =
// false is the kernel with the 64-byte record, instruction for instruction.
template <int BM, int SM, int TEX, bool CAM = false, bool STAGE = false, bool LIVE_ = false, bool C56 = false>
APT_D void shade_traced(args3_ptr A0, Counters* cnt, int cur_, int bounce_, const unsigned long long* strips = nullptr) {
    static_assert(!(CAM && STAGE), "a camera-fed row loads no record");
    static_assert(!C56 || (TEX == 0 && BM == APT_BX_LAMBERTIAN && !(SM & APT_SRC_AREA)), "the 56-byte record: Lambertian surfaces, no area light - nobody reads the ray's origin, its hit distance or its pdf");
    typedef TrRecord<C56> Rec;
    static_assert(!LIVE_ || ((CAM || STAGE) && TEX == 0), "live rows: the staged and the camera-fed form of the lean kernels");
    constexpr bool LIVE = LIVE_ && APT_DRAW_WINDOW != 0;      // (live rows are written for the draw window: a build without it, -DAPT_DRAW_WINDOW=0, keeps the parent's form under the live kernels' names)
    const ShadeArgs3* A_ = args_fresh(A0);                      // scene, parameters, queues: read through the kernel-argument segment, re-fetched per phase (APT_ARGS_PHASE)
    const int cur = CAM ? 0 : cur_, bounce = CAM ? 0 : bounce_, nxt = cur ^ 1;
    const SubLoop sl = sub_loop((A_->p).nq);
    const uint32_t qbase = (uint32_t)sl.q * (A_->p).subcap, sh_qbase = (uint32_t)sl.q * (A_->q).sh_subcap;
    uint32_t* next_counter = &cnt->n_tr[(bounce + 1) % 3][0][sl.q * CNT_PAD];      // (the first queue's tail)
    if (sl.first == 0 && threadIdx.x == 0) { cnt->n_tr[(bounce + 2) % 3][0][sl.q * CNT_PAD] = 0; cnt->n_tr[(bounce + 2) % 3][(A_->q).tr_ncls][sl.q * CNT_PAD] = 0; }      // (read by the previous bounce, appended to by the next one; the second: the staging queue's tail)
    const EmitterGeom geom = {(A_->sc).precom, (A_->sc).normals, (A_->sc).obj_info};
    __shared__ uint32_t s_draws[BLOCK / 64];
    if (lane_id() == 0) s_draws[threadIdx.x >> 6] = 0;
    ShadeTally tl = {0u, 0u, 0u}; uint32_t t_traced = 0, t_lit = 0, t_extend = 0, t_samples = 0;
#ifdef APT_NEAR_STATS
    uint32_t t_near = 0;
#endif
    RowTop rt = {0ull, 0ull, 0ull};
    // the generator: without area lights a Lambertian vertex's draws are all decided when it is opened, and it reads them from a draw window (rng.hpp)
    constexpr bool WINDOW = APT_DRAW_WINDOW != 0 && BM == APT_BX_LAMBERTIAN && !(SM & APT_SRC_AREA);
    typedef typename std::conditional<WINDOW, DrawWindow, Philox>::type Rng;
    constexpr bool PFP = TEX == 0 && !CAM && !STAGE;          // (a camera-fed row knows its primitive when it has traced its ray: nothing to request ahead; a staged row's arrives with its plane B)
    static_assert(APT_FLAT_MAX_PRIMS < (int)TR_NO_PRIM, "the packed record keeps the hit primitive in 8 bits");
    const RecordPlanes tr = {(A_->q).tr[cur][0], (A_->q).tr[cur][1], (A_->q).tr[cur][2], (A_->q).tr[cur][3]};
    StagedRecord stage = {nullptr, nullptr};
    if constexpr (STAGE) stage = staged_record_open<C56>(A_);
    uint32_t n, cam_total = 0;
    if constexpr (CAM) {
        // rows of this sub-queue: 64 per id-space wave w with w % nq == q
        cam_total = (uint32_t)(A_->p).npix * (uint32_t)(A_->p).spp_batch;
        const uint32_t n_waves = (cam_total + 63u) / 64u, nq_ = (uint32_t)(A_->p).nq;
        n = n_waves > (uint32_t)sl.q ? ((n_waves - (uint32_t)sl.q + nq_ - 1u) / nq_) * 64u : 0u;
    } else {
        fix_prologue<C56>((A_->sc), (A_->p), (A_->q), cnt, cur, sl.q, bounce);       // before the queue's length is read: the prologue may append to it
        n = __hip_atomic_load(&cnt->n_tr[bounce % 3][0][sl.q * CNT_PAD], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    uint32_t pf_pm = 0;                                        // (PFP: the next row's packed word)
    if (PFP && n > 0) pf_pm = prefetch_prim<C56>(tr, qbase, sl.first, n);
    if (STAGE && sl.first < n) { stage_row<C56>(stage, tr, qbase, sl.first, n, bounce); staged_wait_stamped(rt, false); }      // (the first row's record: the only one whose round trip the wave sits out)
#ifdef APT_ROWTOP_STATS
    rt.loop0 = __builtin_amdgcn_s_memtime();
#endif
    for (uint32_t base = sl.first; base < n; base += sl.stride) {
        APT_ARGS_PHASE();
        const uint32_t pos = base + threadIdx.x, idx = qbase + pos;                    // (unsorted renders: one queue for the scene)
        bool alive = pos < n;
        const uint32_t cu_pm = pf_pm; float4 cu_ra = make_float4(0.f, 0.f, 0.f, 0.f), cu_rb = cu_ra;
        if (PFP) { const int rp = max(tr_prim(cu_pm), 0); cu_ra = (A_->sc).prim_shade[2 * rp]; cu_rb = (A_->sc).prim_shade[2 * rp + 1]; pf_pm = prefetch_prim<C56>(tr, qbase, base + sl.stride, n); }
        Vertex vx; vertex_reset(vx); Rng rng; rng_init(rng, 0u, 0u, 0u, 0u);
        f3 Lc = splat3(0.f);                                   // the radiance the path has gathered so far (camera rays carry none: nothing is read at bounce 0)
        bool entry = alive; float ray_pdf = 1.f;
        // ---- the row's head: its opened vertex
        if constexpr (CAM && LIVE) alive = camera_vertex_live<BM, SM, WINDOW, C56>(A_, cnt, sl.q, qbase, pos, alive, cam_total, strips, vx, rng, s_draws, t_samples, t_extend, entry);
        else if constexpr (CAM) alive = camera_vertex<BM, SM, TEX, WINDOW, C56>(A_, cnt, sl.q, qbase, pos, alive, cam_total, strips, vx, rng, s_draws, t_samples, t_extend, entry);
        else if constexpr (STAGE) {
            float4 a, b_, c, d;                                // this lane's words of the row's record
            staged_row_read<C56>(stage, a, b_, c, d, cu_ra, cu_rb);
            if constexpr (LIVE) alive = open_record_live<BM, SM, C56>(A_, vx, rng, a, b_, c, d, cu_ra, cu_rb, cur, idx, bounce, alive, s_draws, Lc);
            else if (alive) {
                if (bounce > 0) { Lc = Rec::Lc(c, d); if (SM & APT_SRC_AREA) ray_pdf = d.w; }
                alive = open_record<BM, SM, TEX, true, C56>(A_, vx, rng, a, b_, c, Rec::pm(a, b_), cu_ra, cu_rb, cur, idx, ray_pdf, bounce);
            }
        } else {                                               // the direct loads: plane D has a reader behind the first bounce only
            if constexpr (!C56) if (alive && bounce > 0) { const float4 d = Rec::load_d(tr.d, idx); Lc = Rec::Lc(d, d); if (SM & APT_SRC_AREA) ray_pdf = d.w; }
            if (alive) {
                const float4 a = ldq(tr.a, idx << 4), b_ = ldq(tr.b, idx << 4), c = ldq(tr.c, idx << 4);
                if constexpr (C56) if (bounce > 0) Lc = Rec::Lc(c, Rec::load_d(tr.d, idx));      // (the 56-byte record's radiance lies in planes C and D)
#ifdef APT_ROWTOP_STATS      // (direct loads: everything the row has requested - record, shading record - is waited for between two stamps; the staged form's wait is stamped where it stands)
                staged_wait_stamped(rt, true);
#endif
                alive = open_record<BM, SM, TEX, PFP, C56>(A_, vx, rng, a, b_, c, PFP ? cu_pm : Rec::pm(a, b_), cu_ra, cu_rb, cur, idx, ray_pdf, bounce);
            }
        }
        tl.shade += wave_count(alive);
#ifdef APT_NEAR_STATS      // diagnostic build (tools/gpu_near_probe.py): shaded vertices that sit within 2e-3 of the vertex before them - rays that re-hit the surface they left
        if constexpr (!C56) t_near += wave_count(alive && bounce > 0 && vx.it.min_depth < 2e-3f);      // (56-byte record: the hit distance does not travel - counted where the record is appended, below)
#endif
        // the vertex's position (a 56-byte record carried it: unpack_record)
        if constexpr (!C56 || CAM) {
            if constexpr (LIVE) vx.hit_point = hit_point_of(vx.o, vx.d, vx.it.min_depth);
            else if (alive) vx.hit_point = hit_point_of(vx.o, vx.d, vx.it.min_depth);
        }
        APT_ARGS_PHASE();
        // ---- next-event estimation: the vertex's light sample waits in registers and is swept at the end of the row, when little else is live
        bool break_flag = false; DevSrc src_only;             // the scene's only light, read once through the scalar path
        if ((A_->sc).n_sources == 1) src_only = ld_src_uniform((A_->sc).src);
        LightSample f;                                         // (one light sample per vertex: api.hip pick_shading, PIPE_TRACED)
        if constexpr (LIVE) f = sample_light_live<BM, SM>(A_, vx, rng, geom, src_only, alive);
        else f = sample_light<BM, SM, false>(A_, vx, rng, geom, src_only, alive, break_flag);
        if (f.poisoned) Lc = splat3(f.mis_w);
        tl.shadow += wave_count(f.sampled); tl.poison += wave_count(f.poisoned);
        const int occ_e = pick_occluder_list(A_, f);
        // The next row's record starts on its way HERE, behind the last load that the row's shading waits for: loads come back in the order
        // they were issued, so the wait for any load issued behind the staged ones is a wait for them - the round trip this form takes out
        // of the row.  In front of them lie the continuation's sample and its sweep: time enough to land.
        if constexpr (STAGE) if (base + sl.stride < n) stage_row<C56>(stage, tr, qbase, base + sl.stride, n, bounce);
        APT_ARGS_PHASE();
        // ---- emission of the surface we are on, then the continuation, which meets the scene's records
        bool cont, is_spec = false; float new_pdf = 1.f; f3 new_d = mk3(0.f, 1.f, 0.f);
        if constexpr (LIVE) cont = scatter_live<BM, SM, STAGE>(A_, vx, rng, alive, bounce, s_draws, Lc, new_d, new_pdf, is_spec);
        else cont = scatter<BM, SM, STAGE>(A_, vx, rng, alive, bounce, s_draws, Lc, new_d, new_pdf, is_spec);
        APT_ARGS_PHASE();
        Continuation ct; cont = trace_continuation(A_, vx, new_d, cont, next_counter, t_extend, ct);
        APT_ARGS_PHASE();
        sweep_light_sample<CAM>(A_, cnt, vx, f, occ_e, cur, sl.q, sh_qbase, pos, strips, Lc, t_traced, t_lit);
        // the next row's record has landed - it has had both sweeps - before this row's stores are issued: a wait at the next row's top
        // would be a wait for these stores to be acknowledged as well (one counter, in order)
        if constexpr (STAGE) staged_wait_stamped(rt, true);
#ifdef APT_NEAR_STATS
        if constexpr (C56) t_near += wave_count(cont && ct.q == 0 && ct.t < 2e-3f);
#endif
        append_record<C56, C56 && CAM && !LIVE>(A_, nxt, qbase, next_counter, ct, cont, vx, new_d, rng.draw, is_spec, Lc, new_pdf);
        end_path(A_, !cont && entry, vx.id, Lc);
    }
    flush_uniform(t_traced, &cnt->stats[sl.q][ST_SHADOW_TRACED]); flush_uniform(t_lit, &cnt->stats[sl.q][ST_LIT]); flush_uniform(t_extend, &cnt->stats[sl.q][ST_EXTEND]);
    if (CAM) flush_uniform(t_samples, &cnt->stats[sl.q][ST_SAMPLES]);
    tally_flush(tl, s_draws, cnt, sl.q);
#ifdef APT_NEAR_STATS
    flush_uniform(t_near, &cnt->stats[sl.q][14]);
#endif
#ifdef APT_ROWTOP_STATS
    if (!CAM && lane_id() == 0 && rt.rows) { atomicAdd(&cnt->stats[sl.q][12], rt.wait); atomicAdd(&cnt->stats[sl.q][13], (unsigned long long)__builtin_amdgcn_s_memtime() - rt.loop0); atomicAdd(&cnt->stats[sl.q][14], rt.rows); }
#endif
}
#endif
// ---- the staged shade kernel: reads the extend stage's output - the SoA queues (unsorted renders: ShadeIn) or one packed class queue
// (CQ: Queues::cq, class in.cls) - and writes the next bounce's SoA queue and one shadow-queue entry per useful light sample.
// BM / SM: material and emitter masks of the scene (shading.hpp); code for absent models is compiled out.
// TEX: image-texture lookups.  Only the all-models kernel is instantiated with TEX = 1 (textured scenes run unsorted through
// it): inlined into the specialised kernels the lookup costs e.g. the mod-Phong class kernel its fourth wave per SIMD
// (126 -> 129 VGPRs) in every scene WITHOUT textures, and out of line it costs a call frame in scratch.
// TR: transient render (stages.hpp TransQ): the vertex's optical length is carried by slot, each light sample's time is kept next to its
// radiance plane, and the emitter-hit contribution goes to the slot's record with its time instead of into L.  TR = false is the steady
// kernel, unchanged.  In a light-group render (TransQ::by_light, wave-uniform) the two stored words name the emitter - LightSample::src,
// Vertex::hit_light, as floats: exact below 2^24 - where a transient render stores a time; every other word is the transient twin's.
template <int BM, int SM, int TEX, bool CQ, bool TR = false>
APT_D void shade_staged(args3_ptr A0, Counters* cnt, const ShadeIn& in, int cur, int bounce, TransQ tq = TransQ{}) {
    const ShadeArgs3* A_ = args_fresh(A0);                      // scene, parameters, queues: read through the kernel-argument segment, re-fetched per phase (APT_ARGS_PHASE)
    const int nxt = cur ^ 1;
    const SubLoop sl = sub_loop((A_->p).nq);
    const uint32_t n = in.counts[sl.q * CNT_PAD];
    const uint32_t qbase = (uint32_t)sl.q * (A_->p).subcap, sh_qbase = (uint32_t)sl.q * (A_->q).sh_subcap;
    uint32_t* next_counter = &cnt->n_active[nxt][sl.q * CNT_PAD];
    uint32_t* shadow_counter = &cnt->n_shadow[sl.q * CNT_PAD];
    const EmitterGeom geom = {(A_->sc).precom, (A_->sc).normals, (A_->sc).obj_info};
    __shared__ uint32_t s_draws[BLOCK / 64];
    if (lane_id() == 0) s_draws[threadIdx.x >> 6] = 0;
    ShadeTally tl = {0u, 0u, 0u};
#ifdef APT_NEAR_STATS
    uint32_t t_near = 0;
#endif
    constexpr bool PFP = TEX == 0;                            // the next row's hit primitive is requested one row ahead, as in shade_traced
    const uint32_t in_base = CQ ? (uint32_t)in.cls * (A_->p).cap + qbase : qbase;      // first slot of the queue this workgroup reads
    const float4* cqA = CQ ? (A_->q).cq[0] : nullptr; const float4* cqB = CQ ? (A_->q).cq[1] : nullptr; const float4* cqC = CQ ? (A_->q).cq[2] : nullptr; const float4* cqD = CQ ? (A_->q).cq[3] : nullptr;
    int pf_prim = -1;
    auto prefetch_prim = [&](uint32_t b) {
        const uint32_t ps = in_base + min(b + threadIdx.x, n - 1u);
        pf_prim = CQ ? ldq(reinterpret_cast<const int*>(cqB), (ps << 4) + 12u) : ldq(in.prim, ps << 2);
    };
    if (PFP && n > 0) prefetch_prim(sl.first);
    for (uint32_t base = sl.first; base < n; base += sl.stride) {
        APT_ARGS_PHASE();
        const uint32_t pos = base + threadIdx.x, idx = in_base + pos;
        bool alive = pos < n;
        const int cu_prim = pf_prim;
        float4 cu_ra = make_float4(0.f, 0.f, 0.f, 0.f), cu_rb = cu_ra;
        if (PFP) { const int rp = max(cu_prim, 0); cu_ra = (A_->sc).prim_shade[2 * rp]; cu_rb = (A_->sc).prim_shade[2 * rp + 1]; prefetch_prim(base + sl.stride); }
        Vertex vx; vertex_reset(vx);
        Philox rng; rng_init(rng, 0u, 0u, 0u, 0u);
        if (alive) {
            const uint32_t io = idx << 2;
            const int prim = PFP ? cu_prim : (CQ ? ldq(reinterpret_cast<const int*>(cqB), (idx << 4) + 12u) : ldq(in.prim, io));
            if (prim < 0) alive = false;                         // nothing hit: path ends (vanilla_renderer.py:49)
            else {
                uint32_t meta; float t_in, ray_pdf = 1.f; float2 uv; uv.x = uv.y = 0.f;
                if (CQ) {
                    const float4 a = ldq(cqA, idx << 4), b_ = ldq(cqB, idx << 4), c = ldq(cqC, idx << 4), dd = ldq(cqD, idx << 4);
                    vx.o = mk3(a.x, a.y, a.z); t_in = a.w; vx.d = mk3(b_.x, b_.y, b_.z); vx.thr = mk3(c.x, c.y, c.z); vx.id = __float_as_uint(c.w);
                    meta = __float_as_uint(dd.x); if (SM & APT_SRC_AREA) ray_pdf = dd.y; uv.x = dd.z; uv.y = dd.w;
                } else {
                    vx.o = ld3q(in.ray_o, (A_->p).cap, io); vx.d = ld3q(in.ray_d, (A_->p).cap, io); vx.thr = ld3q(in.thr, (A_->p).cap, io);
                    vx.id = ldq(in.id, io); meta = ldq(in.meta, io); t_in = ldq(in.t, io);
                    if (SM & APT_SRC_AREA) ray_pdf = ldq(in.pdf, io);          // (its only reader is the emission MIS weight: scenes without area lights never look at it)
                    if ((A_->sc).has_vn || (TEX && (A_->sc).tex_i != nullptr)) { uv.x = ldq(in.u, io); uv.y = ldq(in.v, io); }      // otherwise nobody reads the barycentrics (and the flat extend kernel does not write them)
                }
                f3 rec_kd;
                if (PFP) build_hit_rec((A_->sc), cu_ra, cu_rb, prim, t_in, uv.x, uv.y, vx.o, vx.d, vx.it, vx.hit_light, rec_kd);
                else build_hit((A_->sc), prim, t_in, uv.x, uv.y, vx.o, vx.d, vx.it, vx.hit_light, rec_kd);
                alive = open_vertex<BM, SM, TEX>(A_, vx, rng, prim, rec_kd, meta, ray_pdf, uv, bounce);
            }
        }
        tl.shade += wave_count(alive);
#ifdef APT_NEAR_STATS      // diagnostic build (tools/gpu_near_probe.py): shaded vertices that sit within 2e-3 of the vertex before them - rays that re-hit the surface they left
        t_near += wave_count(alive && bounce > 0 && vx.it.min_depth < 2e-3f);
#endif
        if (alive) vx.hit_point = vx.d * vx.it.min_depth + vx.o;
        // the vertex's time: the segment that ends here adds length * ior, the ior of the world's medium when the ray arrives from outside
        // (n_g . d < 0), else that of the hit object's medium (path_tracer.py get_ior, accumulated as in bdpt.py:253); the camera is at 0
        float t_vx = 0.f;
        if constexpr (TR) if (alive) {
            const float ior = (dot(vx.it.n_g, vx.d) < 0.f) ? (A_->sc).world_ior : (A_->sc).med[vx.it.obj_id].ior;
            t_vx = ((bounce == 0) ? 0.f : tq.t_path[vx.l_off >> 2]) + vx.it.min_depth * ior;
        }

        APT_ARGS_PHASE();
        // ---- next-event estimation: one shadow-queue entry per useful light sample
        bool break_flag = false;
        DevSrc src_only;                                      // the scene's only light, read once through the scalar path
        if ((A_->sc).n_sources == 1) src_only = ld_src_uniform((A_->sc).src);
        // light samples by vertex: ONE queue-tail atomic per tile row for all S samples of every vertex
        uint32_t vbase = 0;
        if ((A_->p).nee_vm) vbase = wave_append(alive, shadow_counter);
        for (int s = 0; s < (A_->p).S; s++) {
            const LightSample ls = sample_light<BM, SM, CQ>(A_, vx, rng, geom, src_only, alive, break_flag);
            if (ls.poisoned) stL((A_->q).L, (A_->p).cap, vx.l_off, splat3(ls.mis_w));
            tl.shadow += wave_count(ls.sampled); tl.poison += wave_count(ls.poisoned);
            if ((A_->p).nee_vm) {
                const uint32_t so = (sh_qbase + (uint32_t)s * (A_->p).subcap + vbase) << 2;        // plane s of the sub-queue's region: consecutive lanes, consecutive entries
                if (ls.want) { st3q((A_->q).sh_d, (A_->q).sh_cap, so, ls.dir); stq((A_->q).sh_tmax, so, ls.dist); st3q((A_->q).sh_c, (A_->q).sh_cap, so, ls.contrib); }
                else if (alive) stq((A_->q).sh_tmax, so, -1.0f);                   // the vertex has no sample s worth tracing
                if (alive && s == 0) { stq((A_->q).sh_id, so, vx.l_off); st3q((A_->q).sh_o, (A_->q).sh_cap, so, vx.hit_point); }      // one radiance slot and ONE origin per vertex, kept with its first entry (the S samples leave from the same point: 12 bytes written and read once instead of S times)
            } else {
                const uint32_t spos = wave_append(ls.want, shadow_counter);
                if (ls.want && spos < (A_->q).sh_subcap) {
                    const uint32_t so = (sh_qbase + spos) << 2;
                    shadow_store((A_->q), so, vx.hit_point, ls.dir, ls.dist, ls.contrib);
                    stq((A_->q).sh_id, so, vx.l_off | (((A_->p).l_planes > 1) ? (uint32_t)s : 0u));
                    // its time: the vertex's plus the connection segment's length in the world's medium (an unoccluded segment crosses no
                    // surface: bdpt.py:372,397 with vpt.py track_ray); kept by radiance plane, which only this sample adds into this bounce
                    if constexpr (TR) tq.t_light[(size_t)(((A_->p).l_planes > 1) ? s : 0) * (A_->p).cap + (vx.l_off >> 2)] = tq.by_light ? (float)ls.src : t_vx + ls.dist * (A_->sc).world_ior;      // (a light-group render: the emitter sampled, k_bin_lights)
                }
            }
        }
        APT_ARGS_PHASE();
        // ---- emission of the surface we are on, then the continuation
        bool cont = false, is_spec = false;
        f3 new_d = mk3(0.f, 1.f, 0.f);
        float new_pdf = 1.f;
        if (alive) {
            if constexpr (TR) new_d = emit_and_scatter<BM, SM>(A_, vx, rng, new_pdf, is_spec, [&](f3 add) { tq.emit[vx.l_off >> 2] = make_float4(add.x, add.y, add.z, tq.by_light ? (float)vx.hit_light : t_vx); });      // binned at the vertex's time (k_bin_transient), or by the emitter hit (k_bin_lights)
            else new_d = emit_and_scatter<BM, SM>(A_, vx, rng, new_pdf, is_spec, [&](f3 add) { add_radiance((A_->q).L, (A_->p).cap, vx.l_off, add, true); });      // (nothing else touches the path's slot while its shade kernel runs)
            cont = (bounce + 1) < (A_->p).max_bounce;
            if constexpr (TR) if (cont) tq.t_path[vx.l_off >> 2] = t_vx;
        }
        if (rng.draw != vx.draw0) atomicAdd(&s_draws[threadIdx.x >> 6], rng.draw - vx.draw0);      // also paths that died in the roulette
        APT_ARGS_PHASE();
        const uint32_t npos = wave_append(cont, next_counter);
        if (cont) {
            const uint32_t so = (qbase + npos) << 2;
            st3q((A_->q).ray_o[nxt], (A_->p).cap, so, vx.hit_point);
            st3q((A_->q).ray_d[nxt], (A_->p).cap, so, new_d);
            st3q((A_->q).thr[nxt], (A_->p).cap, so, vx.thr);
            stq((A_->q).id[nxt], so, vx.id);
            stq((A_->q).meta[nxt], so, pack_meta(rng.draw, (uint32_t)(bounce + 1), is_spec));
            if (SM & APT_SRC_AREA) stq((A_->q).pdf[nxt], so, new_pdf);
        }
    }
    tally_flush(tl, s_draws, cnt, sl.q);
#ifdef APT_NEAR_STATS
    flush_uniform(t_near, &cnt->stats[sl.q][14]);
#endif
}
template <int BM, int SM, int TEX = 0>
__global__ void __launch_bounds__(BLOCK) k_shade(DevScene sc, Params p, Queues q, Counters* cnt, ShadeIn in, int cur, int bounce) {
    shade_staged<BM, SM, TEX, false>(kernel_args3(), cnt, in, cur, bounce);
}
template <int BM, int SM, int TEX = 0>
__global__ void __launch_bounds__(BLOCK) k_shade_tr(DevScene sc, Params p, Queues q, Counters* cnt, ShadeIn in, int cur, int bounce, TransQ tq) {
    shade_staged<BM, SM, TEX, false, true>(kernel_args3(), cnt, in, cur, bounce, tq);
}
#if APT_FAST
template <int BM, int SM, int TEX = 0>
__global__ void __launch_bounds__(BLOCK) k_shade_traced(DevScene sc, Params p, Queues q, Counters* cnt, int cur, int bounce) {
    shade_traced<BM, SM, TEX>(kernel_args3(), cnt, cur, bounce);
}
// The Lambertian / point-light specialisation (C1 / C2) under a register bound: with round 6's float transcendentals it allocates 77 VGPRs
// (six waves per SIMD); asked for seven the allocator finds 72 without a spill (eight: 64 and 24 bytes of scratch).
#ifndef APT_TRACED_WAVES
#define APT_TRACED_WAVES 7
#endif
template <int BM, int SM>
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(APT_TRACED_WAVES, APT_TRACED_WAVES))) k_shade_traced_lean(DevScene sc, Params p, Queues q, Counters* cnt, int cur, int bounce) {
    shade_traced<BM, SM, 0>(kernel_args3(), cnt, cur, bounce);
}
// ... with the record staged in LDS a row ahead (shade_traced, STAGE); APT_RECORD_STAGE=0 selects the kernel above
template <int BM, int SM>
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(APT_TRACED_WAVES, APT_TRACED_WAVES))) k_shade_traced_lean_staged(DevScene sc, Params p, Queues q, Counters* cnt, int cur, int bounce) {
    shade_traced<BM, SM, 0, false, true>(kernel_args3(), cnt, cur, bounce);
}
// ... and the staged kernel with live rows (shade_traced, LIVE); APT_LIVE_ROWS=0 selects the kernel above
template <int BM, int SM>
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(APT_TRACED_WAVES, APT_TRACED_WAVES))) k_shade_traced_lean_staged_live(DevScene sc, Params p, Queues q, Counters* cnt, int cur, int bounce) {
    shade_traced<BM, SM, 0, false, true, true>(kernel_args3(), cnt, cur, bounce);
}
// ... and their camera-fed twins (shade_traced, CAM): bounce 0 of a steady full-film batch, in place of k_generate_trace + the first launch above
template <int BM, int SM, int TEX = 0>
__global__ void __launch_bounds__(BLOCK) k_shade_traced_cam(DevScene sc, Params p, Queues q, Counters* cnt, const unsigned long long* strips) {
    shade_traced<BM, SM, TEX, true>(kernel_args3(), cnt, 0, 0, strips);
}
#ifndef APT_TRACED_CAM_WAVES
#define APT_TRACED_CAM_WAVES 7
#endif
template <int BM, int SM>
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(APT_TRACED_CAM_WAVES, APT_TRACED_CAM_WAVES))) k_shade_traced_lean_cam(DevScene sc, Params p, Queues q, Counters* cnt, const unsigned long long* strips) {
    shade_traced<BM, SM, 0, true>(kernel_args3(), cnt, 0, 0, strips);
}
template <int BM, int SM>
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(APT_TRACED_CAM_WAVES, APT_TRACED_CAM_WAVES))) k_shade_traced_lean_cam_live(DevScene sc, Params p, Queues q, Counters* cnt, const unsigned long long* strips) {
    shade_traced<BM, SM, 0, true, false, true>(kernel_args3(), cnt, 0, 0, strips);
}
// ... and the five lean forms on the 56-byte record (shade_traced, C56; stages.hpp TrRecord): what a Lambertian / point-light render runs
// unless APT_RECORD_COMPACT=0.  A renderer runs one record form in every launch of a batch (k_generate_trace56 feeds these).
#define APT_LEAN56_KERNEL(NAME, WAVES) template <int BM, int SM> __global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) NAME
APT_LEAN56_KERNEL(k_shade_traced_lean56, APT_TRACED_WAVES)(DevScene sc, Params p, Queues q, Counters* cnt, int cur, int bounce) { shade_traced<BM, SM, 0, false, false, false, true>(kernel_args3(), cnt, cur, bounce); }
APT_LEAN56_KERNEL(k_shade_traced_lean56_staged, APT_TRACED_WAVES)(DevScene sc, Params p, Queues q, Counters* cnt, int cur, int bounce) { shade_traced<BM, SM, 0, false, true, false, true>(kernel_args3(), cnt, cur, bounce); }
APT_LEAN56_KERNEL(k_shade_traced_lean56_staged_live, APT_TRACED_WAVES)(DevScene sc, Params p, Queues q, Counters* cnt, int cur, int bounce) { shade_traced<BM, SM, 0, false, true, true, true>(kernel_args3(), cnt, cur, bounce); }
APT_LEAN56_KERNEL(k_shade_traced_lean56_cam, APT_TRACED_CAM_WAVES)(DevScene sc, Params p, Queues q, Counters* cnt, const unsigned long long* strips) { shade_traced<BM, SM, 0, true, false, false, true>(kernel_args3(), cnt, 0, 0, strips); }
APT_LEAN56_KERNEL(k_shade_traced_lean56_cam_live, APT_TRACED_CAM_WAVES)(DevScene sc, Params p, Queues q, Counters* cnt, const unsigned long long* strips) { shade_traced<BM, SM, 0, true, false, true, true>(kernel_args3(), cnt, 0, 0, strips); }
#endif

// ---- class kernels in groups: ONE launch shades several material classes.
// A class-sorted bounce was one launch per class (C5: 8 x 16 per batch), and a launch costs its lane 15-30 us however short its queue -
// the pipeline drains, the next grid is dispatched, 1024 workgroups read their queue lengths: most of C5's shade time, a tenth of C3's.
// The classes of a bounce are independent, so a group kernel walks the class queues of its members one after the other - every workgroup
// its sub-queue of class A, then of class B, ... with no barrier in between: a workgroup that runs out of A entries starts on B while
// others still shade A - and the launch boundary between them is gone.  A kernel's register allocation is the maximum over its members',
// so the groups follow the footprints (api.hip kClass).  Round 5 had three - up to 128 VGPRs / four waves per SIMD, up to 168 / three,
// beyond / two (modified Phong and Fresnel blend with their double-precision pow: 201-217).  With the product build's float transcendentals
// and 1-ulp divisions (round 6) no class kernel allocates more than 125, so there are TWO: the lean classes - Lambertian, delta, lobe-free
// Blinn-Phong, Lambertian transmission: 93-96 VGPRs, held to FIVE waves per SIMD - and everything else (Blinn-Phong, Oren-Nayar, thin coat,
// microfacet, modified Phong, Fresnel blend: 111-125, four waves).
// Members absent from the scene are skipped by a wave-uniform test (GroupIn::cls < 0).  Per vertex nothing changes: same class code, same
// queues, same order inside a queue - images and statistics are those of the one-launch-per-class schedule bit for bit (GPU test).
#define APT_GROUP_SLOTS 6
struct GroupIn { const uint32_t* counts[APT_GROUP_SLOTS]; int cls[APT_GROUP_SLOTS]; };     // per member: the class queue's per-sub-queue entry counts, its compact class id (-1: not in this scene)
template <int SM, int WAVES, int B0, int B1, int B2, int B3, int B4 = 0, int B5 = 0>
__global__ void __launch_bounds__(BLOCK, WAVES) k_shade_group(DevScene sc, Params p, Queues q, Counters* cnt, GroupIn g, int cur, int bounce) {
    ShadeIn in = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    if constexpr (B0 != 0) if (g.cls[0] >= 0) { in.counts = g.counts[0]; in.cls = g.cls[0]; shade_staged<B0, SM, 0, true>(kernel_args3(), cnt, in, cur, bounce); }
    if constexpr (B1 != 0) if (g.cls[1] >= 0) { in.counts = g.counts[1]; in.cls = g.cls[1]; shade_staged<B1, SM, 0, true>(kernel_args3(), cnt, in, cur, bounce); }
    if constexpr (B2 != 0) if (g.cls[2] >= 0) { in.counts = g.counts[2]; in.cls = g.cls[2]; shade_staged<B2, SM, 0, true>(kernel_args3(), cnt, in, cur, bounce); }
    if constexpr (B4 != 0) if (g.cls[4] >= 0) { in.counts = g.counts[4]; in.cls = g.cls[4]; shade_staged<B4, SM, 0, true>(kernel_args3(), cnt, in, cur, bounce); }
    if constexpr (B5 != 0) if (g.cls[5] >= 0) { in.counts = g.counts[5]; in.cls = g.cls[5]; shade_staged<B5, SM, 0, true>(kernel_args3(), cnt, in, cur, bounce); }
    if constexpr (B3 != 0) if (g.cls[3] >= 0) { in.counts = g.counts[3]; in.cls = g.cls[3]; shade_staged<B3, SM, 0, true>(kernel_args3(), cnt, in, cur, bounce); }
}
// ... and their transient twins (no occupancy bound: the time words cost a few registers and this mode sets no speed target)
template <int SM, int B0, int B1, int B2, int B3, int B4 = 0, int B5 = 0>
__global__ void __launch_bounds__(BLOCK) k_shade_group_tr(DevScene sc, Params p, Queues q, Counters* cnt, GroupIn g, int cur, int bounce, TransQ tq) {
    ShadeIn in = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    if constexpr (B0 != 0) if (g.cls[0] >= 0) { in.counts = g.counts[0]; in.cls = g.cls[0]; shade_staged<B0, SM, 0, true, true>(kernel_args3(), cnt, in, cur, bounce, tq); }
    if constexpr (B1 != 0) if (g.cls[1] >= 0) { in.counts = g.counts[1]; in.cls = g.cls[1]; shade_staged<B1, SM, 0, true, true>(kernel_args3(), cnt, in, cur, bounce, tq); }
    if constexpr (B2 != 0) if (g.cls[2] >= 0) { in.counts = g.counts[2]; in.cls = g.cls[2]; shade_staged<B2, SM, 0, true, true>(kernel_args3(), cnt, in, cur, bounce, tq); }
    if constexpr (B4 != 0) if (g.cls[4] >= 0) { in.counts = g.counts[4]; in.cls = g.cls[4]; shade_staged<B4, SM, 0, true, true>(kernel_args3(), cnt, in, cur, bounce, tq); }
    if constexpr (B5 != 0) if (g.cls[5] >= 0) { in.counts = g.counts[5]; in.cls = g.cls[5]; shade_staged<B5, SM, 0, true, true>(kernel_args3(), cnt, in, cur, bounce, tq); }
    if constexpr (B3 != 0) if (g.cls[3] >= 0) { in.counts = g.counts[3]; in.cls = g.cls[3]; shade_staged<B3, SM, 0, true, true>(kernel_args3(), cnt, in, cur, bounce, tq); }
}
