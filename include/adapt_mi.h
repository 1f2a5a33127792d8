/*
 * adapt_mi.h — C-ABI of libadapt_mi.so: the MI355X (gfx950) wavefront path tracer that
 * stands in for AdaPT's Taichi `pt` renderer (Renderer, renderer/vanilla_renderer.py) and, with apt_render_cfg.volumetric = 1,
 * for its `vpt` renderer (VolumeRenderer, renderer/vpt.py: homogeneous media, null surfaces, one grid volume).
 *
 * What each entry point replaces in the reference (paths under /root/reference):
 *   apt_bvh_build_linear / apt_linear_bvh_*   tracer/bvh/bvh.cpp:274-296  bvh_cpp.bvh_build(...) (pybind11 module), called from
 *                                   tracer/path_tracer.py:143-179 (bvh_process): the same four arrays in the same layout
 *   apt_bvh_build / apt_bvh_*      the same builder's role for this library's own kernels (binary SAH tree -> 8-wide quantised tree)
 *   apt_bvh_build_device           (no upstream counterpart) the same handle filled by the device builders (LBVH, PLOC), for the tree tests
 *   apt_flat_records               tracer/tracer_base.py:117-134,184-212: the data of the brute-force intersector, as the flat sweep wants it
 *   apt_flat_occluders             (no upstream counterpart) per emitter, the flat records that can block its light samples
 *   apt_camera_strips              (no upstream counterpart) per 64 local pixels, the flat record pairs a camera ray can hit
 *   apt_light_strips               (no upstream counterpart) per 64 local pixels and emitter, the occluder pairs a camera vertex's light sample can meet
 *   apt_scene_create               tracer/tracer_base.py:117-134 (load_primitives) +
 *                                   tracer/path_tracer.py:245-274 (initialze): numpy -> device fields
 *   apt_renderer_create            renderer/vanilla_renderer.py:26-30 / tracer_base.py:36-102 (film, crop, camera,
 *                                   sampling flags) — the constructor half that is not scene data
 *   apt_render                     renderer/vanilla_renderer.py:32-120  Renderer.render, or renderer/vpt.py:145-258
 *                                   VolumeRenderer.render (one launch == one spp there; here `n_spp` samples per call, cnt += n_spp)
 *   apt_read_pixels                `rdr.pixels.to_numpy()` (utils/watermark.py:23): color / cnt, layout [x][y][rgb]
 *   apt_get_accum / apt_set_accum  tracer/path_tracer.py:181-211  get_check_point / load_check_point
 *   apt_read_transient             renderer/bdpt.py:57-58,164-166  time_bins / time_cnts (TRANSIENT_CAM), for the `pt` renderer
 *   apt_read_path_lengths / apt_set_path_lengths   (none; the `pt` render split by path length - emission, direct, n-bounce -)
 *   apt_read_light_groups / apt_set_light_groups / apt_relight   (none; the `pt` render split by emitter - light groups - and relit on the device)
 *   apt_read_sample_counts / apt_read_moments / apt_set_adaptive_state   (none; adaptive sampling)
 *   apt_render_aov / apt_read_aov / apt_set_aov / apt_clear_aov   (none; per-pixel albedo, normal and depth of the camera rays' first hits)
 *   apt_renderer_create with ao = 1, apt_read_ao_depth   renderer/ssao.py:31-130  SSAORenderer (`--type ao`): depth map at creation, screen-space occlusion per sample
 *   apt_renderer_create with direct = 1, apt_render_direct, apt_read_direct_maps   renderer/direct_render.py:26-88  BlinnPhongTracer: hits at creation, one point light per call
 *   apt_denoise                    post_processing.py:15-32 (the firefly filter: stage 1) + an edge-avoiding a-trous filter guided by those buffers (stage 2; none upstream)
 *   apt_get_stats                  (none; the reference only has ti.profiler, render.py:154-160)
 *   apt_device_ptr                 (none; hands the tile framebuffer to RCCL for the multi-GPU gather)
 *
 * Conventions: every function returns 0 on success, a negative APT_E_* code on failure, and
 * apt_last_error() then returns a thread-local message.  Input pointers are borrowed for the
 * duration of the call and copied; outputs are caller-allocated; handles are opaque; one host
 * thread per handle.  All floats are IEEE binary32, ints are 32-bit.  There is no CPU fallback:
 * without a HIP device apt_scene_create / apt_renderer_create fail with APT_E_NO_DEVICE.
 */
#ifndef ADAPT_MI_H
#define ADAPT_MI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define APT_OK            0
#define APT_E_INVALID    -1   /* bad argument */
#define APT_E_NO_DEVICE  -2   /* no usable HIP device */
#define APT_E_HIP        -3   /* HIP runtime error (message has the hipError string) */
#define APT_E_NOMEM      -4
#define APT_E_STATE      -5   /* call not valid in this state */

typedef struct apt_bvh apt_bvh;
typedef struct apt_scene apt_scene;
typedef struct apt_renderer apt_renderer;

/* Flat scene description — the arrays of SURVEY.md §A.2 (what the reference keeps in Taichi fields). */
typedef struct apt_scene_desc {
    int32_t n_prims, n_objects, n_sources, has_vertex_normal;
    const float*   prims;       /* n_prims*9   triangle (v0,v1,v2) | sphere (centre, r r r, 0 0 0) */
    const float*   normals;     /* n_prims*3   geometric normals */
    const float*   v_normals;   /* n_prims*9   per-vertex shading normals (zeros when a mesh has none) */
    const int32_t* obj_info;    /* n_objects*3 first prim, prim count, 0 = mesh | 1 = sphere */
    const float*   obj_aabb;    /* n_objects*6 min xyz, max xyz */
    const int32_t* emitter_id;  /* n_objects   attached emitter index or -1 */
    const int32_t* bxdf_i;      /* n_objects*4 type, is_delta, is_bsdf, 0     (bxdf/brdf.py:152-158, bsdf.py:68-73).  BRDF type 3 (microfacet) shades as the
                                 * reference's Trowbridge-Reitz model, i.e. as the reference does with `__ENABLE_MICROFACET__ = True` (brdf.py:8,428-484); with its
                                 * default False the reference's parser never emits type 3 (it rewrites such a BRDF to Lambertian, brdf.py:60-65): so does the host side here */
    const float*   bxdf_f;      /* n_objects*13 k_d k_s k_g mean, medium ior */
    const int32_t* src_i;       /* n_sources*4 type, bool_bits, obj_ref_id, 0 (emitters/abtract_source.py:44-54) */
    const float*   src_f;       /* n_sources*11 intensity dir pos inv_area r */
    float          world_ior;   /* free-space medium ior */
    /* Image textures on meshes (bxdf/texture.py:99-139, tracer/path_tracer.py:84-126,261-307): all NULL / 0 when the scene has
     * none.  Maps: 0 albedo (replaces k_d, vanilla_renderer.py:66), 1 normal and 2 bump (camera-ray hit only, vanilla_renderer.py:42). */
    const float*   uvs;         /* n_prims*6     per-vertex (u, v) of every triangle */
    const int32_t* tex_i;       /* n_objects*3*5 per object and map: type (-255 = none, 0 = image), off_x, off_y, w, h inside the atlas */
    const float*   tex_f;       /* n_objects*3*2 scale_u, scale_v */
    const float*   atlas[3];    /* per map: atlas_h * atlas_w * 3 floats, row-major [y][x][rgb], or NULL */
    int32_t        atlas_w[3], atlas_h[3];
    /* Participating media for the volumetric path tracer (bxdf/medium.py:24-125, parsers/world.py): both NULL when the scene has
     * none.  Row o < n_objects is the medium attached to object o's BSDF, row n_objects the world's. */
    const int32_t* med_i;       /* (n_objects+1)    type: -1 transparent, 0 hg, 1 multi-hg, 2 rayleigh, 3 mie */
    const float*   med_f;       /* (n_objects+1)*16 ior, u_s rgb, u_a rgb, u_e rgb, par[3], pdf[3] */
    /* Grid volume for the volumetric path tracer (bxdf/volume.py:36-246; what GridVolume_np.export() hands to the kernels): all NULL
     * when the scene declares none. */
    const int32_t* vol_i;       /* 5   type (2 = RGB; the only kind the reference can export), xres, yres, zres, phase-function type */
    const float*   vol_f;       /* 33  albedo rgb, inv_T[9] row-major, trans, mini, maxi (world box), majorant rgb, majorant pdf rgb, phase par[3], lobe weights[3] */
    const float*   vol_grid;    /* zres*yres*xres*3 extinction per channel, [z][y][x][rgb] */
} apt_scene_desc;

/* Per-renderer configuration: film, camera, sampling flags, tile ownership, batching. */
typedef struct apt_render_cfg {
    int32_t width, height;                        /* full film size */
    int32_t do_crop, start_x, end_x, start_y, end_y;
    int32_t max_bounce, num_shadow_ray;
    int32_t use_rr, use_mis, anti_alias, stratified, brdf_two_sides;
    int32_t rr_bounce_th;
    float   rr_threshold;
    float   cam_r[9];                             /* row-major camera rotation */
    float   cam_t[3];
    float   inv_focal, half_w, half_h;
    uint32_t seed;                                /* Philox key word 1 (key word 0 = global pixel index x*H+y) */
    /* tile ownership: columns x with (x / band_width) % world_size == rank belong to this renderer */
    int32_t band_width, rank, world_size;
    int32_t spp_per_batch;                        /* samples per pixel in flight per wavefront batch; 0 = auto: ~32 Mi paths per render lane,
                                                     fitted under the class queues' 32-bit slot addressing and a third of the free device memory.
                                                     A render call splits its samples into equal batches of at most this size, a whole number
                                                     per lane; the image does not depend on the split */
    int32_t device;                               /* HIP device ordinal */
    int32_t profile;                              /* 1 = time every kernel launch with HIP events */
    /* Direct-light viewer: direct = 1 makes the handle upstream's BlinnPhongTracer (renderer/direct_render.py) instead of a
       path tracer.  apt_renderer_create traces the ray through the CENTRE of every pixel of the WHOLE film - anti_alias, stratified and the
       crop window are not read, no random number is drawn - and keeps each pixel's hit distance, shading normal and object
       (apt_read_direct_maps).  apt_render_direct then shades the film for one or more positions of ONE point light of intensity
       direct_intensity: a Blinn-Phong highlight pow(max(dot(h, n_s), 0), k_g) per channel, times min(1 / (1e-5 + d^2), 1e5), times 0.1 where
       the light is occluded, times the intensity and the material's k_d; a miss is 0.  There is no accumulation: apt_render, apt_get_accum,
       apt_set_accum and apt_device_ptr return APT_E_STATE, apt_reset does nothing, apt_read_pixels hands out the last frame shaded.
       Needs volumetric = 0, ao = 0, light_groups = path_lengths = transient_bins = 0, adaptive_threshold = 0 and world_size = 1; max_bounce,
       num_shadow_ray, the roulette and the jitter flags are not read.  (These two sit before the blocks that were there when they were added
       and before `volumetric`, which tests/test_ao_host.py pins as the ao block's neighbour.) */
    int32_t direct;                               /* 0 = off, 1 = direct-light viewer */
    float   direct_intensity[3];                  /* finite; the point source's rgb intensity (upstream's emit_int) */
    int32_t volumetric;                           /* 0 = Renderer.render (renderer/vanilla_renderer.py:32-120); 1 = VolumeRenderer.render
                                                     (renderer/vpt.py:145-258): free-path sampling in homogeneous media, null surfaces,
                                                     transmittance-tracked light samples */
    /* Ambient occlusion: ao = 1 makes the handle upstream's SSAORenderer (renderer/ssao.py, `--type ao`) instead of a path
       tracer.  apt_renderer_create renders the depth map - ao_depth_samples camera rays per pixel at sample counter 0, the mean distance of
       those that hit - and every sample of apt_render traces the camera ray, draws ao_smp_hemisphere directions about the hit's shading normal,
       re-projects the points ao_sample_extent along them onto the film and holds their distance against the depth map there.  The accumulation
       has upstream's layout: channel 0 the sum of (1 - occlusion), channel 1 zero, channel 2 the depth map (apt_set_accum takes it back from
       there; apt_reset keeps it); apt_read_pixels hands out channel 0 / cnt on all three channels where the LAST sample's ray hit, else 0.
       Needs volumetric = 0, light_groups = path_lengths = transient_bins = 0, adaptive_threshold = 0 and world_size = 1 (a sample's depth
       lookups cross the column shards); max_bounce, num_shadow_ray and the roulette are not read.  (These four sit before the blocks that were
       there when they were added.) */
    int32_t ao;                                   /* 0 = off, 1 = ambient occlusion */
    int32_t ao_smp_hemisphere;                    /* > 0; the sensor's smp_hemisphere (upstream's default 32) */
    int32_t ao_depth_samples;                     /* >= 0; the sensor's depth_samples (64) */
    float   ao_sample_extent;                     /* > 0, finite; the sensor's sample_extent (0.1) */
    /* Light groups, surface renderer only: every path contribution is also added to the plane of the emitter its light came
       from - emitter e is row e of apt_scene_desc.src_f - and, within it, to the part that says how the emitter was reached (0: by a sampled
       ray, 1: by a light sample).  Needs volumetric = 0, num_shadow_ray <= 4, world_size = 1, path_lengths = 0, transient_bins = 0 and
       adaptive_threshold = 0; runs the staged pipeline on one render lane.  The planes take n_sources * 2 * owned pixels * 16 bytes.  (It sits
       before the blocks that were there when it was added: they keep their places at the end.) */
    int32_t light_groups;                         /* 0 = off, 1 = keep the n_sources x 2 planes (apt_read_light_groups, apt_relight) */
    /* Path-length images, surface renderer only: every path contribution is also added to the plane of its length - its
       number of segments, camera to emitter - and, within it, to the part that says how the emitter was reached (0: by a sampled ray,
       1: by a light sample).  Needs volumetric = 0, num_shadow_ray <= 4, world_size = 1, transient_bins = 0 and adaptive_threshold = 0;
       runs the staged pipeline on one render lane.  (Like the adaptive block it sits before the two blocks that were there when it was
       added: they keep their places at the end.) */
    int32_t path_lengths;                         /* 0 = off, 1 = keep the max_bounce + 1 planes (apt_read_path_lengths) */
    /* Adaptive sampling: a pixel stops sampling once its relative error e_p (max over channels of the standard error of
       its mean / (mean + 1e-3)) is <= adaptive_threshold.  Decisions are made only at global sample numbers that are multiples of
       adaptive_step and >= adaptive_min_spp; an active pixel takes every sample of a round, with the steady renderer's sample numbers, so
       a pixel with n_p samples holds the steady renderer's accumulation after n_p spp bit for bit.  0 = off (steady state).  Not with
       transient_bins > 0.  (These three sit before the transient block, which keeps the
       last place it had when it was added.) */
    float   adaptive_threshold;                   /* > 0 turns the mode on (finite) */
    int32_t adaptive_min_spp, adaptive_step;      /* both > 0 when the mode is on (the Python layer's defaults: 64, 32) */
    /* Transient (time-resolved) rendering, surface renderer only (DESIGN.md "Transient rendering"): every path contribution is also
       added to a time bin by its optical length, camera to emitter (bdpt.py:164-165, TRANSIENT_CAM).  0 = off (steady state).  Needs
       volumetric = 0, num_shadow_ray <= 4 and world_size = 1; runs the staged pipeline on one render lane. */
    int32_t transient_bins;                       /* number of bins (upstream's sample_count) */
    float   transient_min_time;                   /* a contribution at time t counts when min_time < t < min_time + interval * bins ... */
    float   transient_interval;                   /* ... in bin int((t - min_time) / interval); must be > 0 */
} apt_render_cfg;

/* The stages a launch is filed under: index of apt_stats.launches[] / kernel_ms[] (adapt_amd/_lib.py KERNEL_NAMES lists them in this order) */
enum { APT_K_GENERATE = 0, APT_K_EXTEND = 1, APT_K_SHADE = 2, APT_K_SHADOW = 3, APT_K_FINALIZE = 4 };
#define APT_N_KERNELS 5
typedef struct apt_stats {
    int64_t n_samples;        /* pixel-samples generated */
    int64_t n_extend;         /* closest-hit rays traced */
    int64_t n_shade;          /* bounce-loop iterations that reached shading (after miss / RR / cut-off) */
    int64_t n_shadow;         /* shadow rays the reference would cast (valid emitter sample) */
    int64_t n_shadow_traced;  /* of those, rays with a non-zero contribution that were actually traced */
    int64_t n_lit;            /* traced shadow rays found unoccluded */
    int64_t n_draws;          /* RNG draws consumed */
    int64_t n_poisoned;       /* light samples whose MIS weight was NaN (sample zeroed, as upstream) */
    int64_t launches[APT_N_KERNELS];
    double  kernel_ms[APT_N_KERNELS];   /* summed HIP-event time per kernel (profile=1 only) */
    double  render_ms;                  /* HIP-event time of all apt_render calls so far */
    int64_t n_track;                    /* volumetric: closest-hit queries made by the transmittance walk of the light samples */
    int64_t n_stray_light;              /* light-group renders: non-zero records that named no emitter of the scene and went to no plane (0 unless something is broken) */
} apt_stats;

/* Denoiser settings.  Stage 1, the firefly filter, is upstream's rule (post_processing.py:15-32): on the zero-padded film a pixel
   keeps its value if any of its 8 neighbours lies within Euclidean rgb distance < firefly_threshold of it, else it becomes the float32 sum of the 8
   (first index outermost) / 8; non-finite input components count as 0.  Stage 2 is the a-trous wavelet filter of Dammertz et al. 2010: iteration
   k = 0 .. iterations-1 has 5x5 taps 2^k pixels apart with h = (1/16, 1/4, 3/8, 1/4, 1/16) per axis and tap weight h(dx) h(dy) w_n w_z w_a w_c w_hit:
     w_n = max(0, n_p . n_q)^sigma_n            w_z = exp(-|z_p - z_q| / (sigma_z max(z_p, 1e-6)))
     w_a = exp(-|a_p - a_q|^2 / sigma_a^2)      w_c = exp(-|c_p - c_q|^2 / (sigma_c 2^-k)^2)   (sigma_c <= 0: no colour term)
     w_hit = 1 when p and q agree on hit_fraction > 0, else 0; between two pixels that hit nothing w_n = w_z = w_a = 1
   with n, z, a the feature buffers' means (unit normal, depth, albedo) and c the iteration's input colour.  Taps outside the film or the crop window are
   skipped, the centre tap always counts with h(0)^2, output = weighted sum / weight sum.  demodulate: where hit_fraction > 0 the filter runs on
   c / max(a, 1e-3) and the albedo is multiplied back at the end. */
typedef struct apt_denoise_cfg {
    float   firefly_threshold;                    /* > 0: stage 1 runs (upstream's THRESHOLD is 0.4); 0: off */
    int32_t firefly_only;                         /* 1: stage 1 alone (needs firefly_threshold > 0; the fields below are not read) */
    int32_t iterations;                           /* K, 1..24 (default 3) */
    float   sigma_n, sigma_z, sigma_a, sigma_c;   /* defaults 128, 0.1, 0.1, 1.0: chosen on a measured grid, DESIGN.md §4.7 */
    int32_t demodulate;                           /* default 1 */
} apt_denoise_cfg;

/* ---- BVH build (host, own layout; replaces bvh_cpp.bvh_build) */
int apt_bvh_build(const float* prims /* n_prims*9 */, int32_t n_prims,
                  const int32_t* obj_info /* n_objects*3 */, int32_t n_objects, apt_bvh** out);
int apt_bvh_counts(const apt_bvh*, int32_t* n_nodes, int32_t* n_leaf_prims, int32_t* max_depth);
/* nodes: n_nodes*16 floats (two child boxes + two child links); prim_order: n_prims ints (BVH order -> original prim) */
int apt_bvh_export(const apt_bvh*, float* nodes, int32_t* prim_order);
/* The tree the traversal kernels walk: the binary tree (rebuilt with single-primitive leaves) collapsed to 8-wide nodes with
 * 8-bit quantised child boxes, 64 bytes = 16 dwords per node, breadth-first, node 0 = root (layout: csrc/bvh_wide.cpp);
 * prim_order: leaf-order slot -> original primitive.  n_levels = depth in 8-wide nodes.  apt_bvh_wide_frame: the global grid the
 * 16-bit node corners live on (world = gmin + gstep * grid, power-of-two steps). */
int apt_bvh_wide_counts(const apt_bvh*, int32_t* n_nodes, int32_t* n_levels);
int apt_bvh_wide_export(const apt_bvh*, uint32_t* nodes /* n_nodes*16 */, int32_t* prim_order /* n_prims */);
int apt_bvh_wide_frame(const apt_bvh*, float gmin[3], float gstep[3]);
void apt_bvh_free(apt_bvh*);
/* The device builders on their own (csrc/bvh_gpu.hip; algo 0 = LBVH, 1 = PLOC): the handle apt_bvh_build fills, holding the device-built
 * binary tree with single-primitive leaves (apt_bvh_counts / apt_bvh_export; max_depth is the tree's real depth) and its 8-wide collapse
 * (apt_bvh_wide_*).  Needs n_prims >= 2.  Never falls back to the host builder: a failed device build is an error.  *algo_used: the
 * algorithm that produced the tree (a PLOC build that gives up is retried as LBVH and reports 0).  Arguments are checked before the device
 * is looked for; a device ordinal outside 0..count-1 is APT_E_INVALID, "apt_bvh_build_device: device ordinal out of range". */
int apt_bvh_build_device(const float* prims /* n_prims*9 */, int32_t n_prims, const int32_t* obj_info /* n_objects*3 */, int32_t n_objects,
                         int32_t device, int32_t algo, apt_bvh** out, int32_t* algo_used);

/* ---- records of the flat sweep (host; csrc/flat_build.cpp).  What the product build's small-scene intersector reads instead of the
 * reference's `prims` / `precom_vec` (tracer/tracer_base.py:117-134,184-212): per planar primitive its corner and the rows of
 * [e1 e2 n]^-1; two coplanar triangles of an object that share an edge and have a convex outline are one record.  apt_scene_create
 * builds them internally; this entry exposes the builder so that it can be checked without a device.
 * counts[7]: parallelograms, parallelograms in coplanar groups, convex quads, convex quads in groups, triangles, triangles in groups,
 * spheres.  stream (may be NULL): counts-ordered records, 12 floats each (corner p0, rows U, V, T), 18 for convex quads (+ the two far
 * edges as a u + b v + c), 4 per sphere (centre, r^2); tab (may be NULL): 28 floats per record (U, p0.x | V, p0.y | prim_a prim_b
 * class_a class_b as int32 | map_a[6] | map_b[6] | p0.z ...).  n_stream / n_tab: floats needed (always written). */
int apt_flat_records(const float* prims /* n_prims*9 */, int32_t n_prims, const int32_t* obj_info /* n_objects*3 */, int32_t n_objects,
                     int32_t counts[7], float* stream, int32_t stream_cap, float* tab, int32_t tab_cap, int32_t* n_stream, int32_t* n_tab);
/* Occluder lists of the light samples (csrc/flat_build.cpp flat_occluders): per emitter, the flat records a segment from
 * the scene to a point the emitter can be sampled at may block - what the product build's traced shade kernel sweeps a light sample
 * against.  src_i / src_f as in apt_scene_desc.  cull = 0: every list is the full stream.  table (may be NULL): 8 int32 per emitter (offset
 * into pairs in floats, records per section: parallelograms, convex quads, triangles, spheres; 0 0 0); keep (may be NULL): n_records
 * flags per emitter, 1 = in the list, records in apt_flat_records' stream order; pairs (may be NULL): the lists two records at a time
 * (the layout of the flat sweep's paired stream).  n_records / n_pairs: always written. */
int apt_flat_occluders(const float* prims /* n_prims*9 */, int32_t n_prims, const int32_t* obj_info /* n_objects*3 */, int32_t n_objects,
                       const int32_t* src_i, const float* src_f, int32_t n_sources, int32_t cull, int32_t* table, int32_t* keep, int32_t keep_cap,
                       float* pairs, int32_t pairs_cap, int32_t* n_records, int32_t* n_pairs);

/* Strip lists of the camera rays (host only): for the film, camera, crop-independent band plan (band_width, rank, world_size)
 * of cfg, one 64-bit word per block of 64 consecutive local pixels (ceil(owned columns * height / 64) words): bit k set = a camera ray of
 * the block can hit a record of pair k of the flat sweep's paired stream (pairs counted in stream order across the sections).  cull = 0:
 * every bit of every word set (what APT_CAMERA_CULL=0 gives a renderer).  masks may be NULL; n_strips / n_pairs: always written. */
int apt_camera_strips(const float* prims /* n_prims*9 */, int32_t n_prims, const int32_t* obj_info /* n_objects*3 */, int32_t n_objects,
                      const apt_render_cfg* cfg, int32_t cull, uint64_t* masks, int32_t masks_cap, int32_t* n_strips, int32_t* n_pairs);

/* Strip masks of the camera vertex's light samples (host only): per emitter e < min(n_sources, 16) and block b of 64
 * consecutive local pixels, masks[e * n_strips + b]: bit k set = a record of pair k of emitter e's occluder list (apt_flat_occluders with
 * cull = 1, its order and pairing) may block a light sample taken at a camera hit point of the block.  cull = 0: every bit set (what
 * APT_LIGHT_STRIPS=0 gives a renderer).  n_pairs (n_sources entries): pairs per list; origin_slack: how far off the strip's clipped
 * outlines the rule lets a shadow-ray origin lie.  masks, n_pairs, origin_slack may be NULL. */
int apt_light_strips(const float* prims /* n_prims*9 */, int32_t n_prims, const int32_t* obj_info /* n_objects*3 */, int32_t n_objects,
                     const int32_t* src_i, const float* src_f, int32_t n_sources, const apt_render_cfg* cfg, int32_t cull,
                     uint64_t* masks, int32_t masks_cap, int32_t* n_strips, int32_t* n_pairs, float* origin_slack);

/* ---- BVH build, reference layout: the drop-in for the pybind11 module itself.
 * Replaces bvh_cpp.bvh_build(obj_array, obj_info, world_min, world_max) (tracer/bvh/bvh.cpp:274-296), whose four flat arrays
 * PathTracer.bvh_process reshapes and loads into the LinearBVH / LinearNode fields (tracer/path_tracer.py:155-170,
 * tracer/ti_bvh.py:10-53) for AdaPT's own stackless preorder walk.  obj_prim_cnt / obj_is_sphere are the two rows of the
 * reference's (2, n_obj) obj_info table (tracer/path_tracer.py:222-230).  Outputs of apt_linear_bvh_export, caller-allocated:
 *   bvh_minmax  n_prims*6  per-primitive box (min xyz, max xyz) in tree order      node_minmax n_nodes*6  per-node box
 *   bvh_info    n_prims*2  (object, original primitive)                            node_info   n_nodes*3  (first, count, subtree size)
 * Nodes are in preorder; node 0 is the root with box = the world box and subtree size = n_nodes; a leaf has subtree size 1.
 * Host only (no device needed).  adapt_amd/bvh_cpp.py wraps these three calls as a module named like the reference's. */
typedef struct apt_linear_bvh apt_linear_bvh;
int apt_bvh_build_linear(const float* prims /* n_prims*9 */, int32_t n_prims, const int32_t* obj_prim_cnt, const int32_t* obj_is_sphere,
                         int32_t n_objects, const float* world_min /* 3 */, const float* world_max /* 3 */, apt_linear_bvh** out);
int apt_linear_bvh_counts(const apt_linear_bvh*, int32_t* n_nodes, int32_t* n_prims);
int apt_linear_bvh_export(const apt_linear_bvh*, float* bvh_minmax, float* node_minmax, int32_t* bvh_info, int32_t* node_info);
void apt_linear_bvh_free(apt_linear_bvh*);

/* ---- scene / renderer lifetime */
int apt_scene_create(const apt_scene_desc* desc, int32_t device, apt_scene** out);
void apt_scene_destroy(apt_scene*);
/* What built the binary tree under the scene's 8-wide tree, after any fallback: 0 = binned SAH on the host, 1 = LBVH, 2 = PLOC on the device
 * (the default from a million primitives up; env APT_BVH_BUILDER=sah|lbvh|ploc, read at apt_scene_create, overrides). */
int apt_scene_bvh_builder(const apt_scene*, int32_t* builder);
int apt_renderer_create(const apt_scene*, const apt_render_cfg* cfg, apt_renderer** out);
void apt_renderer_destroy(apt_renderer*);

/* ---- rendering */
int apt_render(apt_renderer*, int32_t n_spp);             /* accumulates n_spp more samples per owned pixel */
int apt_synchronize(apt_renderer*);
int apt_tile_shape(const apt_renderer*, int32_t* n_cols, int32_t* height);   /* owned framebuffer = n_cols*height*3 */
int apt_read_pixels(apt_renderer*, float* out);           /* owned tile, [local col][y][rgb], color / cnt (adaptive: color / n_p, 0 where n_p = 0) */
int apt_get_accum(apt_renderer*, float* out, int32_t* cnt);
int apt_set_accum(apt_renderer*, const float* in, int32_t cnt);
int apt_reset(apt_renderer*);                             /* color = 0, cnt = 0, stats = 0, transient bins = 0, path-length planes = 0, light-group planes = 0, adaptive state = start, feature buffers = 0 */
/* transient renders: the owned tile's bins, [bin][local col][y][rgba] - summed r, g, b (divide by cnt for radiance, as pixels) and the
   number of contributions (a); transient_bins * n_cols * height * 4 floats.  apt_set_transient restores them (checkpoints). */
int apt_read_transient(apt_renderer*, float* out);
int apt_set_transient(apt_renderer*, const float* in);
/* path-length renders (path_lengths = 1; APT_E_STATE otherwise): the owned tile's planes, [length - 1][part][local col][y][rgba] - summed
   r, g, b (divide by cnt for radiance, as pixels) and the number of contributions (a); (max_bounce + 1) * 2 * n_cols * height * 4 floats.
   Summed over lengths and parts they are the accumulation.  apt_set_path_lengths restores them (checkpoints). */
int apt_read_path_lengths(apt_renderer*, float* out);
int apt_set_path_lengths(apt_renderer*, const float* in);
/* light-group renders (light_groups = 1; APT_E_STATE otherwise): the owned tile's planes, [emitter][part][local col][y][rgba] - summed r, g, b
   (divide by cnt for radiance, as pixels) and the number of contributions (a); n_sources * 2 * n_cols * height * 4 floats.  Summed over emitters
   and parts they are the accumulation.  apt_set_light_groups restores them (checkpoints).  apt_relight: out = the owned tile, [local col][y][rgb],
   with emitter e's share multiplied by gains[3e .. 3e+2] (rgb): sum over e, part 0 then part 1, of gain * plane, / cnt - what apt_read_pixels would
   hand out had emitter e's intensity been scaled by its gain, on the same random stream.  A channel with gain 0 is skipped (no 0 * inf). */
int apt_read_light_groups(apt_renderer*, float* out);
int apt_set_light_groups(apt_renderer*, const float* in);
int apt_relight(apt_renderer*, const float* gains /* n_sources*3 */, float* out /* n_cols*height*3 */);
/* adaptive renders (adaptive_threshold > 0; APT_E_STATE otherwise), owned tile in [local col][y] order: the per-pixel sample counts n_p and
   (active may be NULL) whether each pixel still samples; the float64 sums of squared sample values, 3 per pixel (S2; S1 is the accumulation).
   apt_set_adaptive_state restores all three (checkpoints; after apt_set_accum). */
int apt_read_sample_counts(apt_renderer*, int32_t* counts, uint8_t* active);
int apt_read_moments(apt_renderer*, double* s2);
int apt_set_adaptive_state(apt_renderer*, const int32_t* counts, const double* s2, const uint8_t* active);
/* Feature buffers of the surface renderer on one rank (volumetric = 1 and world_size > 1: APT_E_INVALID).  apt_render_aov adds the camera rays of
   samples first_sample+1 .. first_sample+n_spp - the rays apt_render traces for those sample numbers, met with the renderer's own traversal - to the
   per-pixel sums: a ray that hits contributes the albedo the shade stage would read (k_d or the albedo map), the shading normal after the maps
   (world space, not flipped) and the hit distance; a miss nothing.  The caller keeps track of which samples are in.  apt_read_aov: owned pixels in
   [local col][y] order, 8 floats each: sum albedo rgb, sum depth, sum normal xyz, hit count (all 0 outside a crop window).  Sums are added in sample
   order by one thread per pixel: repeated runs and other call splits give the same bits.  apt_set_aov restores them (checkpoints). */
int apt_render_aov(apt_renderer*, int32_t first_sample, int32_t n_spp);
int apt_read_aov(apt_renderer*, float* out);
int apt_set_aov(apt_renderer*, const float* in);
int apt_clear_aov(apt_renderer*);
/* Denoise colour_in ([x][y][rgb], width*height*3 floats; NULL: the renderer's current pixels, as apt_read_pixels hands them out) into out, guided by
   the feature buffers as they stand.  The settings are checked before the handle and the device.  Same refusals as the feature buffers. */
int apt_denoise(apt_renderer*, const apt_denoise_cfg* cfg, const float* colour_in, float* out);
/* ambient-occlusion renders (ao = 1; APT_E_STATE otherwise): the depth map, [local col][y], n_cols * height floats - the mean hit distance of the
   pixel's ao_depth_samples camera rays, 0 where none hit or outside a crop window */
int apt_read_ao_depth(apt_renderer*, float* out);
/* direct-light viewers (direct = 1; APT_E_STATE otherwise).  apt_render_direct shades the film once per light position: emit_pos holds n >= 1
   positions (n * 3 floats, every one finite: n <= 0, NULL or a non-finite coordinate is APT_E_INVALID); out, where not NULL, takes the n frames,
   [frame][x][y][rgb], n * width * height * 3 floats.  The per-pixel hits are read once per launch, whatever n is; a sweep too large for the
   frame buffer runs in several launches.  apt_read_pixels hands out the last frame afterwards.  apt_read_direct_maps copies out what the
   creation's hit pass kept: depth ([x][y], width * height floats: the hit distance, 0 for a miss) and normal ([x][y][xyz]: the shading normal,
   not normalised where it is a mix of vertex normals; zero for a miss); either pointer may be NULL. */
int apt_render_direct(apt_renderer*, const float* emit_pos, int32_t n, float* out);
int apt_read_direct_maps(apt_renderer*, float* depth, float* normal);
int apt_get_stats(apt_renderer*, apt_stats* out);
int apt_device_ptr(apt_renderer*, void** accum_dev, int32_t* cnt); /* device float[n_cols*height*3] accumulation buffer */
int apt_stream(apt_renderer*, void** hip_stream);         /* the hipStream_t every kernel of this renderer runs on */

/* ---- unit entry points used by the parity tests (same device code paths as apt_render)
 * The ones from apt_rng_stream on check their arguments before they look for a device, so a bad call is APT_E_INVALID with or without
 * one; a device ordinal outside 0..count-1 is APT_E_INVALID, "<name>: device ordinal out of range"; apt_emitter_probe refuses a row whose
 * source index is not an integer in 0..n_sources-1 (NaN included) with APT_E_INVALID, "apt_emitter_probe: no such emitter". */
int apt_intersect(apt_renderer*, int32_t n, const float* o, const float* d,
                  int32_t* prim_out, float* t_out, float* uv_out);
int apt_occluded(apt_renderer*, int32_t n, const float* o, const float* d, const float* tmax, int32_t* occ_out);
int apt_rng_stream(int32_t device, uint32_t pixel, uint32_t seed, uint32_t sample, int32_t n, uint32_t* out);
/* Surface-model probe: test k uses material (bxdf_i[4k..], bxdf_f[13k..]) and dirs12[12k..] = n_s, n_g, incid, out.
 * do_sample = 0: out[4k..] = eval rgb (f*cos), pdf(out | incid).   [BRDF.eval/get_pdf, BSDF.eval_surf/get_pdf]
 * do_sample = 1: out[9k..] = dir xyz, f*cos rgb, pdf, is_specular, draws; RNG = Philox(key=(k, seed), sample 1). */
int apt_bxdf_probe(int32_t device, int32_t n, const int32_t* bxdf_i, const float* bxdf_f, const float* dirs12,
                   float world_ior, int32_t do_sample, uint32_t seed, float* out);
/* Texture probe: map_obj[2k..] = map (0 albedo, 1 normal, 2 bump), object; uv[2k..]; out3[3k..] = Texture.query.  Any coordinate may be
 * asked for: no texel outside the texture's rectangle is read (the contract is stated at texture_query, csrc/shade_stage.hpp). */
int apt_texture_probe(const apt_scene*, int32_t n, const int32_t* map_obj, const float* uv, float* out3);
/* Surface-maps probe: the normal, bump and albedo maps of a vertex as the shade kernels apply them.  Row k: primitive prim_first[2k],
 * prim_first[2k+1] != 0 for a camera ray's hit (the only one whose shading normal the maps touch), barycentrics bary[2k..].
 * out7[7k..] = k_d, n_s, the maps that applied (1 albedo | 2 normal | 4 bump).  A primitive outside 0..n_prims-1 is APT_E_INVALID,
 * "apt_surface_maps_probe: no such primitive". */
int apt_surface_maps_probe(const apt_scene*, int32_t n, const int32_t* prim_first, const float* bary, float* out7);
/* Medium probe (volumetric tracer; bxdf/medium.py:84-125, bxdf/phase.py): test k uses medium (med_i[k], med_f[16k..]) and in7[7k..].
 * mode 0: Medium.sample_mfp, in = max_depth            -> out8[8k..] = is_mi, t, beta rgb, draws
 * mode 1: Medium.sample_new_rays, in = incid xyz       -> dir xyz, phase value x3, pdf, draws
 * mode 2: Medium.eval + transmittance, in = incid xyz, out xyz, depth -> phase value, transmittance rgb.  RNG as above. */
int apt_medium_probe(int32_t device, int32_t n, const int32_t* med_i, const float* med_f, int32_t mode, const float* in7,
                     uint32_t seed, float* out8);
/* Grid-volume probe (volumetric tracer; bxdf/volume.py:268-463): one volume, packed as apt_scene_desc carries it (vol_i[5], vol_f[33],
 * vol_grid), test k uses in10[10k..] and the Philox stream keyed (k, seed), sample 1.  The volume is checked as apt_scene_create checks it.
 * mode 0: GridVolume.intersect_volume, in = o xyz, d xyz, -, -, -, max_t   -> out8[8k..] = hit, near_t, far_t
 * mode 1: density_lookup_3d + channel, in = index xyz, u xyz, channel      -> the voxel value (0 outside the grid)
 * mode 2: GridVolume.sample_mfp,       in = o xyz, d xyz, thp rgb, max_t   -> hit_t (-1: none), beta rgb, draws
 * mode 3: GridVolume.transmittance,    in = o xyz, d xyz, thp rgb, max_t   -> transmittance rgb, draws */
int apt_volume_probe(int32_t device, int32_t n, const int32_t* vol_i, const float* vol_f, const float* vol_grid, int32_t mode,
                     const float* in10, uint32_t seed, float* out8);
/* Emitter probe: in11[11k..] = source index, hit_pos, normal, ray_d, min_depth;
 * out12[12k..] = sampled pos, intensity (/pdf), pdf, draws, eval_le rgb, solid_angle_pdf; RNG as above. */
int apt_emitter_probe(const apt_scene*, int32_t n, const float* in11, uint32_t seed, float* out12);
/* Transient binning probe: out[k] = the time bin the transient renderer puts a contribution at time t[k] into (-1: outside the window),
 * for the window of n_bins bins of width interval from min_time, set up as apt_renderer_create sets it up. */
int apt_transient_bin_probe(int32_t device, int32_t n, const float* t, float min_time, float interval, int32_t n_bins, int32_t* out);
/* trace_mode: 0 = BVH traversal, 1 = wave-uniform sweep (scenes of <= 96 primitives with object boxes), 2 = tiled sweep (of those, the
 * scenes with an object large enough to be worth skipping per ray), 3 = flat sweep (product build: every scene small enough to have flat
 * records).  env APT_TRAVERSAL=bvh|sweep|tile|flat, read at apt_renderer_create, overrides where the scene allows the mode asked for. */
int apt_renderer_info(const apt_renderer*, int32_t* spp_batch, int32_t* n_subqueues, int64_t* queue_bytes,
                      int32_t* lds_bytes, const char** shade_variant, int32_t* trace_mode);
/* Rays traced in place: *fused = 1 when the renderer shades the camera vertex in the kernel that traces the camera ray (steady full-film
 * renders with max_bounce >= 1; env APT_CAMERA_FUSE=0, read at apt_renderer_create, selects generate + a queue-fed bounce 0), else 0. */
int apt_renderer_camera_fused(const apt_renderer*, int32_t* fused);
/* ... and *in_use = 1 when that kernel sweeps the camera vertex's light samples against strip masks that leave some pair of an occluder
 * list out (apt_light_strips; env APT_LIGHT_STRIPS=0, read at apt_renderer_create, sets every bit), else 0 - always 0 without the fusion. */
int apt_renderer_light_strips(const apt_renderer*, int32_t* in_use);
/* Rays traced in place: *staged = 1 when the queue-fed shade kernel stages each row's path record in LDS a row ahead (the Lambertian /
 * point-light kernel; env APT_RECORD_STAGE=0, read at apt_renderer_create, selects the kernel that loads the record where it is used), else 0. */
int apt_renderer_record_staged(const apt_renderer*, int32_t* staged);
/* Rays traced in place: *live = 1 when the staged and the camera-fed shade kernel run their live-row form - every lane of a row computes on a
 * valid record, a dead lane's effects are masked (the Lambertian / point-light kernels; env APT_LIVE_ROWS=0, read at apt_renderer_create,
 * selects the kernels that give dead lanes default values), else 0. */
int apt_renderer_live_rows(const apt_renderer*, int32_t* live);
/* Rays traced in place: *compact = 1 when every launch of a batch reads and writes the 56-byte path record - the hit point instead of the
 * ray's origin and hit distance, no pdf of the ray (the Lambertian / point-light kernels, which read neither; env APT_RECORD_COMPACT=0,
 * read at apt_renderer_create, keeps the 64-byte record), else 0. */
int apt_renderer_record_compact(const apt_renderer*, int32_t* compact);

/* Shader clock (MHz) with every CU busy: cycle counter against the 100 MHz wall clock over a full-grid FMA chain (~1 ms).
 * bench.py prices the VALU roofline of the trace kernels with it.  (No reference counterpart.) */
int apt_measure_sclk_mhz(int32_t device, float* mhz);

const char* apt_last_error(void);
const char* apt_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ADAPT_MI_H */
