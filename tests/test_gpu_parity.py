"""HIP path (through the C-ABI) vs the CPU oracle and the golden fixtures — the parity tests proper, on the EXACT build.

The library exists in two builds of the same sources (adapt_amd/build.py): `exact` (libadapt_mi_exact.so: every intersector is the
reference's loop operation for operation) and `fast` (libadapt_mi.so: the product, what bench.py and smoke() run; small scenes take
the flat sweep of traverse.hpp, inside SURVEY 8(d)'s stated tolerances).  This module pins the exact build - bit-exact hits, draw
counts and images wherever the arithmetic is deterministic; tests/test_gpu_fast.py holds the product build to the stated tolerances
on the same scenes and ties the two builds together where they run the same code.

Tolerances (float32 path tracing):
  * integer / index work (RNG words, hit primitive ids, occlusion flags, path statistics): exact;
  * per-call float outputs of the shading models: <= 4 ulp-ish (rel 3e-6): the device evaluates
    cos/sin/pow in double and rounds once, the CPU side calls glibc's float functions;
  * images, HIP vs oracle with the SAME Philox stream: >= 99.5 % of pixels within 1e-3*(1+|x|) per channel and
    relMSE <= 1e-4 (an ulp-level difference can flip a branch and re-draw a path; nothing else may differ).
"""
import os

import numpy as np
import pytest

import gpu_cases as GC
from conftest import SCENES, golden, image_metrics, scene_from_golden
from gpu_cases import counters_within, image_within
from parity_bounds import EXACT, REFERENCE_RUN
from adapt_amd.scene_pack import make_config

pytestmark = pytest.mark.gpu

F = golden("functions.npz")


@pytest.fixture(autouse=True, scope="module")
def _exact_build():
    """every renderer / scene / probe of this module lives in libadapt_mi_exact.so"""
    from adapt_amd import _lib
    prev = _lib.use("exact")
    yield
    _lib.use(prev)


def close(a, b, rel=3e-6, abs_=1e-7):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    both_nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(both_nan | (np.abs(a - b) <= abs_ + rel * np.abs(b))))


@pytest.fixture
def renderer(parsed):
    """tests/gpu_cases.py renderer_factory: every renderer a test makes is closed when that test ends"""
    with GC.renderer_factory(parsed) as make:
        yield make


def test_native_library_is_the_one_in_tree():
    import os
    from adapt_amd import _lib
    _lib.load()
    maps = open("/proc/self/maps").read()
    assert os.path.realpath(_lib.LIB_PATH) in maps


def test_rng_stream_bit_exact():
    from adapt_amd.renderer import rng_stream
    from oracle import binding as ob
    for pixel, seed, sample in ((0, 0, 1), (262143, 0, 1024), (12345, 99, 7), (2 ** 32 - 1, 2 ** 32 - 1, 2 ** 31)):
        assert np.array_equal(rng_stream(pixel, seed, sample, 37), ob.rng_stream(pixel, seed, sample, 37))
    assert rng_stream(0, 0, 0, 4).tolist() == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]      # Random123 known answer


# microfacet_functions.npz: the reference's Trowbridge-Reitz BRDF (type 3), recorded with its `__ENABLE_MICROFACET__` switch on
@pytest.mark.parametrize("fixture", ["functions.npz", "microfacet_functions.npz"])
def test_bxdf_eval_pdf_vs_reference_vectors(fixture):
    from adapt_amd.renderer import bxdf_probe
    F = golden(fixture)
    x = F["eval_in"]
    m = x[:, 0].astype(int)
    out = bxdf_probe(F["mat_i"][m], F["mat_f"][m], x[:, 1:13], world_ior=1.0, sample=False)
    y = F["eval_out"]
    bad = [k for k in range(len(x)) if not close(out[k], y[k])]
    assert not bad, [(k, int(m[k]), out[k], y[k]) for k in bad[:5]]
    assert np.isnan(y).any() or fixture != "functions.npz"          # the fresnel-blend NaN-pdf quirk is part of the vectors


@pytest.mark.parametrize("fixture", ["functions.npz", "microfacet_functions.npz"])
def test_bxdf_sample_vs_reference_vectors(fixture):
    from adapt_amd.renderer import bxdf_probe
    F = golden(fixture)
    x = F["sample_in"]
    m = x[:, 0].astype(int)
    dirs = np.concatenate([x[:, 1:10], np.zeros((len(x), 3), np.float32)], axis=1)
    out = bxdf_probe(F["mat_i"][m], F["mat_f"][m], dirs, world_ior=1.0, sample=True, seed=777)
    y = F["sample_out"]
    assert np.array_equal(out[:, 7], y[:, 7]) and np.array_equal(out[:, 8], y[:, 8])     # is_specular flag, draws consumed
    bad = [k for k in range(len(x)) if not close(out[k, :7], y[k, :7], rel=2e-5, abs_=2e-6)]
    assert not bad, [(k, int(m[k]), out[k], y[k]) for k in bad[:5]]


@pytest.mark.parametrize("tag", ["cbox", "balls_mono", "glass_box", "features_a"])
def test_intersection_vs_reference_vectors(tag, renderer):
    g = golden(f"scene_{SCENES[tag][2]}.npz")
    r = renderer(tag, width=64, height=64)
    prim, t, uv = r.intersect(g["ray_o"], g["ray_d"])
    h = g["ray_hit"]
    assert np.array_equal(prim, h[:, 1].astype(np.int32))                  # same primitive (or -1)
    hit = prim >= 0
    assert np.array_equal(t[hit], h[hit, 2])                               # same operations -> same bits
    tri = hit & (r.flat.obj_info[np.maximum(h[:, 0].astype(int), 0), 2] == 0)
    assert np.array_equal(uv[tri], h[tri, 3:5])
    assert np.all(t[~hit] == np.float32(1e7))
    assert np.array_equal(r.occluded(g["ray_o"], g["ray_d"], g["ray_tmax"]), g["ray_occ"])


@pytest.mark.parametrize("tag", ["cbox", "balls_mono", "glass_box", "features_a"])
def test_intersection_vs_oracle_random_rays(tag, renderer, oracle_scene):
    rs = np.random.RandomState(7)
    n = 20000
    o = rs.uniform([0.1, 0.1, 0.1], [5.4, 5.3, 5.4], size=(n, 3)).astype(np.float32)
    d = rs.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:50, 0] = 0.0                                                        # axis-parallel components (inf slabs)
    d[:50] /= np.linalg.norm(d[:50], axis=1, keepdims=True)
    tmax = rs.uniform(0.2, 8.0, n).astype(np.float32)
    r = renderer(tag, width=192, height=192)
    sc = oracle_scene(tag)
    prim, t, uv = r.intersect(o, d)
    obj_o, prim_o, t_o, uv_o, _ = sc.intersect(o, d)
    same = prim == prim_o
    # a different primitive is only acceptable as an exact tie in t (shared edge): SURVEY §7 "traversal order parity"
    assert np.all(t[~same] == t_o[~same]) and (~same).mean() < 2e-2
    assert np.array_equal(t[same], t_o[same])
    assert np.array_equal(r.occluded(o, d, tmax), sc.occluded(o, d, tmax))


@pytest.mark.parametrize("mode", ["bvh", "sweep", "tile"])
def test_every_traversal_mode_gives_the_same_hits_and_image(mode, parsed, oracle_scene, monkeypatch):
    """The three intersectors (per-lane BVH walk, wave sweep, tiled sweep) are interchangeable: same closest hit,
    same occlusion answer, same image.  APT_TRAVERSAL is read when the renderer is created."""
    from adapt_amd.renderer import Renderer
    monkeypatch.setenv("APT_TRAVERSAL", mode)
    tag = "features_a"                                                      # spheres + two-triangle quads + a 12-triangle box
    r = Renderer(*parsed(tag), width=64, height=48)
    try:
        assert r.info()["traversal"] == mode
        rs = np.random.RandomState(11)
        n = 30000
        o = rs.uniform([0.1, 0.1, 0.1], [5.4, 5.3, 5.4], size=(n, 3)).astype(np.float32)
        d = rs.normal(size=(n, 3)).astype(np.float32)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        d[:64, 1] = 0.0; d[64:128, 0] = 0.0; d[64:128, 2] = 0.0              # zero components: infinite / NaN slabs
        o[64:96, 0] = 0.0                                                   # ... starting exactly on a wall plane
        d[:128] /= np.linalg.norm(d[:128], axis=1, keepdims=True)
        tmax = rs.uniform(0.2, 8.0, n).astype(np.float32)
        sc = oracle_scene(tag)
        prim, t, uv = r.intersect(o, d)
        _, prim_o, t_o, uv_o, _ = sc.intersect(o, d)
        if mode == "bvh":
            # own tree: the same primitive, exact ties included (lowest index among equal t, as the brute-force loop keeps it); only
            # the per-object slab cull - whose NaN / inf behaviour decides the degenerate rays 0..127 - belongs to the brute-force
            # intersector alone
            g = slice(128, None)
            assert np.array_equal(prim[g], prim_o[g]) and np.array_equal(t[g], t_o[g])
            assert np.array_equal(r.occluded(o[g], d[g], tmax[g]), sc.occluded(o[g], d[g], tmax[g]))
        else:                                                                # reference iteration order: identical, uv included
            assert np.array_equal(prim, prim_o) and np.array_equal(t, t_o)
            from adapt_amd.scene_pack import pack_scene
            fs = pack_scene(*parsed(tag))
            is_sphere_prim = np.zeros(fs.n_prims, bool)
            for first, count, kind in fs.obj_info:
                is_sphere_prim[first:first + count] = kind != 0
            tri_hit = (prim >= 0) & ~is_sphere_prim[np.maximum(prim, 0)]    # barycentrics are only defined (and used) for triangles
            assert np.array_equal(uv[tri_hit], uv_o[tri_hit])
            assert np.array_equal(r.occluded(o, d, tmax), sc.occluded(o, d, tmax))
        if mode == "bvh":
            return      # this scene's mod-Phong wall emits axis-parallel rays from points ON a wall plane, which upstream's slab cull drops
                        # (NaN slabs) and a tree does not; image parity of the BVH walk is test_bvh_mode_matches_oracle_on_mesh_scene's job
        r.render(n_spp=8)
        rc = make_config(parsed(tag)[3], width=64, height=48)
        ref, _, ost = sc.render(rc, 8)
        image_within(r.color.to_numpy(), ref, 8, EXACT.within, EXACT.rel, label=mode)
        counters_within(r.stats(), ost, EXACT.counters, 0, label=mode)
    finally:
        r.close()


@pytest.mark.parametrize("tag", ["balls_mono", "glass_box", "features_a", "features_c"])      # features_a: all five emitter types
def test_emitters_vs_reference_vectors(tag, renderer):
    g = golden(f"scene_{SCENES[tag][2]}.npz")
    r = renderer(tag, width=64, height=64)
    out = r.emitter_probe(g["emit_in"], seed=778)
    y = g["emit_out"]
    assert np.array_equal(out[:, 7], y[:, 7])                              # draws
    assert close(out[:, :7], y[:, :7], rel=2e-5, abs_=2e-6) and close(out[:, 8:], y[:, 8:], rel=2e-5, abs_=2e-6)


def test_point_emitter_vs_reference_vectors(renderer):
    g = golden("scene_cbox.npz")
    out = renderer("cbox", width=64, height=64).emitter_probe(g["emit_in"], seed=778)
    assert np.array_equal(out[:, 7], g["emit_out"][:, 7]) and close(out[:, :7], g["emit_out"][:, :7])


IMAGE_CASES = [
    # tag, width, height, spp, overrides        (C1 = cbox 256^2 / 64 spp / 4 bounces: BASELINE configs[0])
    ("cbox", 256, 256, 64, {"max_bounce": 4}),
    ("cbox", 96, 96, 16, {}),
    ("balls_mono", 96, 96, 8, {}),
    ("glass_box", 96, 96, 8, {}),
    # feature coverage: five emitter types + every remaining surface model; no RR / no MIS / two-sided / uniform jitter;
    # single sphere emitter with pixel-centre rays and aggressive RR
    ("features_a", 64, 48, 16, {}),
    ("features_b", 64, 48, 16, {}),
    ("features_c", 64, 48, 16, {}),
    ("textured", 64, 48, 16, {}),
    ("microfacet", 64, 48, 16, {}),           # Trowbridge-Reitz BRDFs (the reference's opt-in model), sorted into a class of their own
]


@pytest.mark.parametrize("tag,w,h,spp,ov", IMAGE_CASES)
def test_image_matches_oracle_same_stream(tag, w, h, spp, ov, renderer, parsed, oracle_scene):
    """tests/gpu_cases.py image_vs_oracle_same_stream on the exact build: SURVEY 8(d) verbatim, and the exact path structure"""
    info = GC.image_vs_oracle_same_stream(renderer, parsed, oracle_scene, tag, w, h, spp, ov, *EXACT, exact_structure=True)
    assert info["arithmetic"] == "exact"


@pytest.mark.parametrize("tag", ["cbox", "balls_mono", "glass_box", "features_a", "features_b", "features_c", "textured", "microfacet"])
def test_image_matches_reference_run(tag, renderer):
    """Directly against the fixture recorded from the reference's own kernel (same Philox stream), the first sample alone too."""
    assert GC.image_vs_reference_run(renderer, tag, *REFERENCE_RUN, first_sample=True)["arithmetic"] == "exact"


@pytest.mark.parametrize("tag", ["cbox", "balls_mono"])
def test_statistical_cross_check_other_seed(tag, renderer, parsed, oracle_scene):
    """the HIP estimator is the same estimator, not merely the same stream -- against a CPU render with ANOTHER seed its
    relMSE stays within 1.5x of the relMSE between two CPU renders with different seeds."""
    hip, cpu, info = GC.other_seed_images(renderer, parsed, oracle_scene, tag)
    GC.other_seed_criterion_exact(tag, hip, cpu)
    assert info["arithmetic"] == "exact"


def test_cbox_is_bit_reproducible_and_batch_invariant(renderer):
    """One shadow ray per bounce => every float is added in a fixed order: bitwise reproducible, and
    independent of how samples are batched or the render call is split."""
    a = renderer("cbox", width=128, height=128, spp_per_batch=8)
    a.render(n_spp=24)
    img = a.color.to_numpy()
    b = renderer("cbox", width=128, height=128, spp_per_batch=3)
    b.render(n_spp=10); b.render(n_spp=14)
    assert np.array_equal(img, b.color.to_numpy())
    c = renderer("cbox", width=128, height=128, spp_per_batch=1)
    c.render(n_spp=24)
    assert np.array_equal(img, c.color.to_numpy())
    assert a.stats()["n_shade"] == b.stats()["n_shade"] == c.stats()["n_shade"]
    # the library's own split (no batch size given: equal lane-batches, a whole number per render lane - api.hip lane_batch)
    d = renderer("cbox", width=128, height=128)
    d.render(n_spp=24)
    assert np.array_equal(img, d.color.to_numpy()) and d.stats()["n_shade"] == a.stats()["n_shade"]


@pytest.mark.parametrize("tag", ["cbox", "features_b"])          # one shadow ray per hit: no two float atomics ever meet on a radiance slot
def test_render_lanes_do_not_change_the_image(tag, parsed, monkeypatch):
    """Batches run concurrently on 1..4 HIP streams (APT_LANES); the finalize kernels are chained so that every pixel still
    receives its samples in sample order: the accumulated image and the statistics are bit-identical for any lane count.
    (With several shadow rays per hit the order of the atomic adds into a path's radiance is free, lanes or not.)"""
    from adapt_amd.renderer import Renderer
    out = {}
    for lanes in (1, 2, 3, 4):
        monkeypatch.setenv("APT_LANES", str(lanes))
        r = Renderer(*parsed(tag), width=96, height=64, spp_per_batch=2)
        try:
            r.render(n_spp=7); r.render(n_spp=6)          # 7 batches (the last one short), then a second call that starts on lane 0 again
            out[lanes] = (r.color.to_numpy().copy(), {k: v for k, v in r.stats().items() if k.startswith("n_")})
        finally:
            r.close()
    for lanes in (2, 3, 4):
        assert np.array_equal(out[lanes][0].view(np.uint32), out[1][0].view(np.uint32)), lanes
        assert out[lanes][1] == out[1][1], (lanes, out[lanes][1], out[1][1])


def test_tile_partition_invariance_on_one_gpu(renderer):
    """4 'ranks' rendered one after the other on the same device assemble to the single-renderer image."""
    from adapt_amd.tiles import assemble
    full = renderer("cbox", width=160, height=96)
    full.render(n_spp=6)
    ref = full.color.to_numpy()
    tiles = []
    for rank in range(4):
        r = renderer("cbox", width=160, height=96, rank=rank, world_size=4, band_width=16)
        r.render(n_spp=6)
        tiles.append(r.tile_accum())
        assert r.tile_accum().shape == (len(r.plan.columns(rank)), 96, 3)
    assert np.array_equal(assemble(full.plan.__class__(160, 96, 16, 4), tiles), ref)


def test_checkpoint_round_trip_and_crop(renderer, parsed):
    a = renderer("cbox", width=64, height=64)
    a.render(n_spp=4)
    ck = a.get_check_point()
    assert set(ck) >= {"w", "h", "crop_x", "crop_y", "crop_rx", "crop_ry", "focal", "num_objects", "num_prims", "cam_orient", "src_num",
                       "cam_t", "accumulation", "counter"} and ck["counter"] == 4 and ck["accumulation"].shape == (64, 64, 3)
    a.render(n_spp=4)
    b = renderer("cbox", width=64, height=64)
    b.load_check_point(ck)
    assert b.cnt[None] == 4
    b.render(n_spp=4)
    assert np.array_equal(a.color.to_numpy(), b.color.to_numpy())           # resume == uninterrupted
    ck["w"] = 65
    with pytest.raises(ValueError):
        b.load_check_point(ck)
    # crop: pixels outside the window are never touched (vanilla_renderer.py:37-38)
    from adapt_amd.renderer import Renderer
    em, arr, objs, cfg = parsed("cbox")
    cfg = dict(cfg); cfg["film"] = {"width": 64, "height": 64, "crop_x": 30, "crop_y": 20, "crop_rx": 10, "crop_ry": 6}
    c = Renderer(em, arr, objs, cfg)
    c.render(n_spp=8)
    img = c.color.to_numpy()
    assert np.array_equal(img[20:40, 14:26], a.color.to_numpy()[20:40, 14:26])
    mask = np.ones((64, 64), bool); mask[20:40, 14:26] = False
    assert not img[mask].any() and c.stats()["n_samples"] == 8 * 20 * 12
    c.close()


def test_full_size_properties_c2(renderer):
    """BASELINE configs[1] shape (cbox 512x512, 8 bounces) at a reduced sample count: properties that do not
    need the oracle at this size — statistics identities, energy bounds, left/right colour bleeding."""
    r = renderer("cbox")
    assert (r.w, r.h, r.max_bounce) == (512, 512, 8)
    r.render(n_spp=32)
    st = r.stats()
    img = r.pixels.to_numpy()
    n = 512 * 512 * 32
    assert st["n_samples"] == n and st["n_shadow"] == st["n_shade"]          # S = 1: one light sample per shaded bounce
    assert st["n_samples"] < st["n_extend"] <= st["n_samples"] + st["n_shade"]
    assert st["n_lit"] <= st["n_shadow_traced"] <= st["n_shadow"] and st["n_poisoned"] == 0
    assert 3.0 < st["n_shade"] / n < 4.2 and 12.0 < st["n_draws"] / n < 14.0   # 3.63 shades, 13 draws per sample
    assert np.isfinite(img).all() and img.min() >= 0 and 0.1 < img.mean() < 0.6
    # red wall (x ~ 5.5) shows at small i, green (x = 0) at large i: x decreases with i (tracer_base.py:156)
    red, green = img[12:72, 200:300].mean(axis=(0, 1)), img[440:500, 200:300].mean(axis=(0, 1))
    assert red[0] > 2 * red[1] and green[1] > 2 * green[0]


FULL_SIZE = os.environ.get("APT_FULL_SIZE_PARITY") == "1"


@pytest.mark.skipif(not FULL_SIZE, reason="minutes of host time for the oracle: APT_FULL_SIZE_PARITY=1 (the run of record is profiles/r0N_full_size_parity.log)")
@pytest.mark.parametrize("tag,spp", [("cbox", 1024), ("balls_mono", 1024)])
def test_full_size_parity_c2_c3(tag, spp, renderer, parsed, oracle_scene, capsys):
    """BASELINE configs[1] and [2] at their FULL size - 512x512, 1024 samples per pixel, 8 / 16 bounces - HIP against the oracle on the
    same Philox stream, every pixel: the per-pixel tolerance of the small cases holds at 268 M samples, and the path statistics agree."""
    # "identical": the one inf pixel of C2 (vanilla_renderer.py:119 zeroes NaN only) coincides
    info = GC.full_size_parity(renderer, parsed, oracle_scene, capsys, tag, spp, 0.9999, 1e-7, 1e-5, non_finite="identical", print_l2=True)
    assert info["arithmetic"] == "exact"


# ---------------------------------------------------------------- large scenes: BVH traversal path
@pytest.mark.parametrize("tag,scene", [("c2", "cbox"), ("c3", "balls_mono")])
def test_full_frame_c2_c3_against_the_oracle_statistics(tag, scene, renderer):
    """BASELINE configs[1] / [2] at their FULL film size (512 x 512, all bounces; 64 of the 1024 spp) against the oracle's render of the
    same samples (tests/golden/fullsize_*.npz, generated by tests/golden/gen/gen_fullsize_stats.py): path statistics, the 8 x 8 grid of
    tile means, the image at 1/8 resolution.  Un-gated twin of test_full_size_parity_c2_c3, which compares every pixel at 1024 spp."""
    # counters 2e-6: an ulp in a transcendental can flip a branch: 81 of 1.2e9 vertices at 1024 spp
    info = GC.full_frame_vs_oracle_statistics(renderer, tag, scene, counters=2e-6, tiles=2e-5, within=0.9999, rel=1e-9)
    assert info["arithmetic"] == "exact"


@pytest.fixture(scope="module")
def bunnies_small():
    from adapt_amd.synth import three_bunnies
    return three_bunnies(levels=1)                 # 5 950 triangles: the oracle's brute force still finishes in seconds


@pytest.mark.parametrize("levels,dyn", [(4, "1"), (4, "0"), (64, "1")])
def test_bvh_stack_spill_and_fetch_modes_agree(levels, dyn, bunnies_small, monkeypatch):
    """The traversal stack keeps its first levels in LDS and spills deeper ones to global columns; with only 4 LDS levels nearly every
    ray spills.  Closest hits, occlusion flags and the image must not depend on where the stack lives nor on whether rays are assigned
    to lanes statically or fetched dynamically (same per-ray arithmetic): compared with the default configuration bit for bit."""
    from adapt_amd.renderer import Renderer
    rs = np.random.RandomState(5)
    n = 4000
    o = rs.uniform([0.3, 0.2, 0.3], [5.2, 5.2, 5.2], size=(n, 3)).astype(np.float32)
    d = rs.normal(size=(n, 3)).astype(np.float32); d /= np.linalg.norm(d, axis=1, keepdims=True)
    tmax = rs.uniform(0.2, 6.0, n).astype(np.float32)
    ref = Renderer(*bunnies_small, width=64, height=64)
    ref_hit, ref_occ = ref.intersect(o, d), ref.occluded(o, d, tmax)
    ref.render(n_spp=3); ref_img = ref.color.to_numpy(); ref.close()
    monkeypatch.setenv("APT_BVH_LDS_LEVELS", str(levels)); monkeypatch.setenv("APT_DYN_FETCH", dyn)
    r = Renderer(*bunnies_small, width=64, height=64)
    try:
        prim, t, uv = r.intersect(o, d)
        assert np.array_equal(prim, ref_hit[0]) and np.array_equal(t, ref_hit[1]) and np.array_equal(uv, ref_hit[2])
        assert np.array_equal(r.occluded(o, d, tmax), ref_occ)
        r.render(n_spp=3)
        a, b = r.color.to_numpy(), ref_img
        # three-bunnies takes two light samples per vertex: their float atomics may land in either order, nothing else may differ
        assert np.mean(np.all(np.abs(a - b) <= 1e-5 * (1 + np.abs(b)), axis=2)) >= 0.999
    finally:
        r.close()


def test_bvh_mode_matches_oracle_on_mesh_scene(bunnies_small):
    """> 96 primitives => BVH traversal (own tree).  Against the oracle's BRUTE-FORCE intersector: same closest hits,
    same occlusion, same image, spot lights + glass + fresnel-blend."""
    from adapt_amd.renderer import Renderer
    from adapt_amd.scene_pack import pack_scene
    from oracle import binding as ob
    r = Renderer(*bunnies_small, width=96, height=96)
    assert r.info()["traversal"] == "bvh" and r.flat.n_prims == 10 + 3 * 495 * 4
    rc = make_config(bunnies_small[3], width=96, height=96)
    rc.use_bvh = False
    sc = ob.OracleScene(pack_scene(*bunnies_small), rc.cam_t, build_bvh=True)
    rs = np.random.RandomState(3)
    n = 6000
    o = rs.uniform([0.3, 0.2, 0.3], [5.2, 5.2, 5.2], size=(n, 3)).astype(np.float32)
    d = rs.normal(size=(n, 3)).astype(np.float32); d /= np.linalg.norm(d, axis=1, keepdims=True)
    # rays through shared edges and vertices of the mesh as well (exact ties between two or more triangles): both intersectors keep
    # the lowest primitive index among equal t - the walk by an explicit tie-break, whatever order its tree visits them in
    tri = r.flat.prims.reshape(-1, 3, 3)[10:10 + 400]
    mids = np.concatenate([(tri[:, 0] + tri[:, 1]) * np.float32(0.5), tri[:, 2]]).astype(np.float32)
    eo = np.tile(np.float32([2.78, 2.73, -3.0]), (mids.shape[0], 1))
    ed = mids - eo; ed /= np.linalg.norm(ed, axis=1, keepdims=True).astype(np.float32)
    o, d = np.concatenate([o, eo]), np.concatenate([d, ed.astype(np.float32)])
    prim, t, uv = r.intersect(o, d)
    _, prim_o, t_o, uv_o, _ = sc.intersect(o, d)
    assert np.array_equal(prim, prim_o) and np.array_equal(t, t_o) and np.array_equal(uv[prim >= 0], uv_o[prim >= 0])
    n = 6000
    tmax = rs.uniform(0.2, 6.0, o.shape[0]).astype(np.float32)
    assert np.array_equal(r.occluded(o, d, tmax), sc.occluded(o, d, tmax))
    r.render(n_spp=4)
    ref, cnt, ost = sc.render(rc, 4)
    m = image_metrics(r.pixels.to_numpy(), ref / np.float32(cnt))
    st = r.stats()
    assert m["frac_within"] >= 0.99 and m["relMSE"] <= 2e-4, m
    assert abs(st["n_shade"] - ost["n_shade"]) <= 1e-3 * ost["n_shade"] and abs(st["n_draws"] - ost["n_draws"]) <= 1e-3 * ost["n_draws"]
    # the oracle's restated reference BVH gives the oracle's brute-force image bit for bit
    rc.use_bvh = True
    ref_bvh, _, _ = sc.render(rc, 4)
    assert np.array_equal(ref, ref_bvh)
    r.close()


def test_full_size_c4_scene_properties():
    """BASELINE configs[3] stand-in at full geometry (95 050 triangles, 800x800) with few samples: checks that do
    not need the CPU at this size — the tree covers every primitive, statistics identities, finite image, and a
    cropped window equals the same window of the full render (RNG keyed by global pixel)."""
    from adapt_amd.renderer import Renderer
    from adapt_amd.synth import three_bunnies
    em, arr, objs, cfg = three_bunnies()
    r = Renderer(em, arr, objs, cfg)
    assert (r.w, r.h, r.num_prims, r.max_bounce, r.num_shadow_ray) == (800, 800, 95050, 8, 2) and r.info()["traversal"] == "bvh"
    r.render(n_spp=2)
    st, img = r.stats(), r.pixels.to_numpy()
    assert st["n_samples"] == 800 * 800 * 2 and st["n_shadow"] == 2 * st["n_shade"] and st["n_lit"] <= st["n_shadow_traced"] <= st["n_shadow"]
    assert np.isfinite(img).all() and img.mean() > 0.05          # (fresnel-blend's diffuse lobe can go slightly negative, upstream too)
    cfg2 = dict(cfg); cfg2["film"] = {"width": 800, "height": 800, "crop_x": 400, "crop_y": 300, "crop_rx": 48, "crop_ry": 32}
    c = Renderer(em, arr, objs, cfg2)
    c.render(n_spp=2)
    win = c.pixels.to_numpy()[352:448, 268:332]
    m = image_metrics(win, img[352:448, 268:332])
    assert m["frac_within"] >= 0.995, m           # two shadow rays per bounce: float atomics may reorder, nothing else differs
    r.close(); c.close()


def test_rccl_gather_path_on_one_gpu(renderer):
    """The multi-GPU readback path with a world of one: torch.distributed backend "nccl" (= RCCL), the zero-copy view of the
    renderer's device framebuffer, all_gather_into_tensor, tile assembly.  (N > 1 is covered by the gloo test on CPU.)"""
    import os
    import socket
    import torch
    import torch.distributed as dist
    from adapt_amd.tiles import device_tile, gather_image
    r = renderer("cbox", width=96, height=64)
    r.render(n_spp=3)
    local = r.color.to_numpy()
    t = device_tile(r)
    assert t.is_cuda and tuple(t.shape) == (96, 64, 3) and np.array_equal(t.cpu().numpy(), local)
    sock = socket.socket(); sock.bind(("127.0.0.1", 0)); port = sock.getsockname()[1]; sock.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        img = gather_image(r, normalised=False, force_collective=True)
        assert np.array_equal(img, local)
        img = gather_image(r, normalised=True, force_collective=True)
        assert np.array_equal(img, local / np.float32(3))
    finally:
        dist.destroy_process_group()


def test_full_size_c4_crop_matches_brute_force_oracle():
    """tests/gpu_cases.py c4_crop_vs_brute_force_oracle on the exact build"""
    from gpu_cases import c4_crop_vs_brute_force_oracle
    assert c4_crop_vs_brute_force_oracle()["arithmetic"] == "exact"


def test_full_size_c5_scene_properties():
    """BASELINE configs[4] stand-in at full geometry (285 134 triangles, 1280x720, 16 bounces, S = 1, every live surface model,
    two area lights) with few samples: the checks that need no CPU at this size - statistics identities, NaN-free image, and a
    cropped window that equals the same window of the full render (the RNG is keyed by the global pixel)."""
    from adapt_amd.renderer import Renderer
    from adapt_amd.synth import bunny_field
    em, arr, objs, cfg = bunny_field()
    r = Renderer(em, arr, objs, cfg)
    assert (r.w, r.h, r.num_prims, r.max_bounce, r.num_shadow_ray) == (1280, 720, 285134, 16, 1) and r.info()["traversal"] == "bvh"
    r.render(n_spp=2)
    st, img = r.stats(), r.pixels.to_numpy()
    n = 1280 * 720 * 2
    assert st["n_samples"] == n and st["n_lit"] <= st["n_shadow_traced"] <= st["n_shadow"] <= st["n_shade"]      # S = 1; no light sample on an emitter hit
    assert n < st["n_extend"] <= n + st["n_shade"] and 2.0 < st["n_shade"] / n < 8.0
    # upstream zeroes NaN samples and lets +-inf through (vanilla_renderer.py:119): no NaN ever, inf only as a rare pdf = 0 path
    assert not np.isnan(img).any() and np.isinf(img).any(axis=2).mean() < 1e-4
    fin = img[np.isfinite(img).all(axis=2)]
    assert 0.05 < fin.mean() < 5.0
    r.close()                                     # 8 class queues x 3 lanes: ~30 GiB of queues per renderer at this film size
    cfg2 = dict(cfg); cfg2["film"] = {"width": 1280, "height": 720, "crop_x": 640, "crop_y": 300, "crop_rx": 56, "crop_ry": 36}
    c = Renderer(em, arr, objs, cfg2)
    c.render(n_spp=2)
    win, full = c.pixels.to_numpy()[584:696, 264:336], img[584:696, 264:336]
    assert c.stats()["n_samples"] == 2 * 112 * 72
    assert np.array_equal(win, full)              # one light sample per vertex: no two float atomics meet on a radiance slot
    c.close()


@pytest.mark.parametrize("cx,cy", [(640, 360), (330, 250), (930, 200)])
def test_full_size_c5_crop_matches_brute_force_oracle(cx, cy):
    """tests/gpu_cases.py c5_crop_vs_brute_force_oracle on the exact build"""
    from gpu_cases import c5_crop_vs_brute_force_oracle
    assert c5_crop_vs_brute_force_oracle(cx, cy)["arithmetic"] == "exact"


def test_full_size_properties_c3(renderer):
    """BASELINE configs[2] shape (csphere balls-mono, 512x512, 16 bounces, S = 4 light samples per vertex, area light, spheres,
    glass, mirror, Fresnel blend) at a reduced sample count: statistics identities, energy bounds, NaN-free image, and a cropped
    window vs the same window of the full render."""
    r = renderer("balls_mono")
    assert (r.w, r.h, r.max_bounce, r.num_shadow_ray) == (512, 512, 16, 4)
    r.render(n_spp=16)
    st, img = r.stats(), r.pixels.to_numpy()
    n = 512 * 512 * 16
    assert st["n_samples"] == n and st["n_poisoned"] * 1000 < st["n_shadow"]
    # four light samples per shaded vertex, except on the emitter itself (single light: break_flag, vanilla_renderer.py:84-86)
    assert st["n_shadow"] <= 4 * st["n_shade"] and st["n_shadow"] > 3.5 * st["n_shade"]
    assert st["n_lit"] <= st["n_shadow_traced"] <= st["n_shadow"] and n < st["n_extend"] <= n + st["n_shade"]
    assert 3.5 < st["n_shade"] / n < 5.0 and 60.0 < st["n_draws"] / n < 95.0            # 4.21 shades, 77 draws per sample
    assert not np.isnan(img).any() and np.isinf(img).any(axis=2).mean() < 1e-4
    fin = img[np.isfinite(img).all(axis=2)]
    assert fin.min() > -1e-3 and 0.1 < fin.mean() < 2.0


def test_full_size_c3_crop_matches_oracle(parsed, oracle_scene):
    """C3 at full film size, a 128 x 96 window x 16 spp, all 16 bounces and S = 4: HIP (wave sweep) vs the oracle, same stream."""
    assert GC.c3_crop_vs_oracle(parsed, oracle_scene, spp=16, within=0.995, rel=1e-4, counters=5e-4)["arithmetic"] == "exact"


@pytest.mark.parametrize("tag", ["cbox", "bunnies1", "bunnies3"])
def test_hip_vs_the_reference_intersectors_on_recorded_rays(tag):
    """tests/golden/bvhref_*.npz: rays answered by the reference's own BVH walk and (the first ones) by its own brute force.
    HIP returns the brute-force answer on every ray: equal to both reference intersectors where those agree, and on the rays of
    the 95 050-triangle scene where the reference's BVH walk loses a hit (DESIGN "the reference's BVH path") HIP has the nearer hit
    its brute force finds."""
    from adapt_amd.renderer import Renderer
    tup, fs, g = GC.bvhref_scene(tag)
    r = Renderer(*tup, width=64, height=64)
    try:
        O, D, TM = g["ray_o"], g["ray_d"], g["ray_tmax"]
        prim, t, uv = r.intersect(O, D)
        occ = r.occluded(O, D, TM)
        hb, hv = g["brute_hit"], g["bvh_hit"]
        n = hb.shape[0]
        miss = hb[:, 1] < 0
        assert np.array_equal(prim[:n][~miss], np.int32(hb[:, 1][~miss])) and np.array_equal(t[:n][~miss], hb[:, 2][~miss]) and (prim[:n][miss] < 0).all()
        assert np.array_equal(uv[:n][~miss], hb[:, 3:5][~miss]) and np.array_equal(occ[:n], g["brute_occ"])
        # the rest of the batch was answered by the reference's BVH walk only
        hit = hv[:, 1] >= 0
        same = (prim == np.int32(hv[:, 1])) & hit & (t == hv[:, 2]) | (~hit & (prim < 0))
        nearer = hit & (prim >= 0) & (t < hv[:, 2]) | (~hit & (prim >= 0))
        assert (same | nearer).all()
        assert nearer.sum() <= (45 if tag == "bunnies3" else 0)         # 41 of the 682 rays were picked for being lost by the walk
        assert ((occ == g["bvh_occ"]) | (occ == 1)).all() and (occ != g["bvh_occ"]).sum() <= (10 if tag == "bunnies3" else 0)
    finally:
        r.close()


# ---- the reference's own bundled scene files (arrays from its parser, tests/golden/refscene_*.npz)
from conftest import REF_SCENE_TAGS, scene_from_golden  # noqa: E402


@pytest.mark.parametrize("tag", REF_SCENE_TAGS)
def test_reference_bundled_scene_hip_vs_reference_run(tag):
    """HIP render of one of the reference's bundled scenes vs (a) the image the reference's own kernel produced on the same
    Philox stream (fixture) and (b) the oracle at more samples; path statistics exact."""
    from adapt_amd.renderer import Renderer
    from adapt_amd.scene_pack import make_config, pack_scene
    from oracle import binding as ob
    tup, g = scene_from_golden(tag)
    w, h = int(g["width"]), int(g["height"])
    r = Renderer(*tup, width=w, height=h)
    try:
        rc = make_config(tup[3], width=w, height=h)
        # 0.99: 768 pixels, one flipped branch is 0.13 %
        GC.fixture_then_oracle(r, g, ob.OracleScene(pack_scene(*tup), rc.cam_t), rc, 24, tag, within=0.99, rel=1e-3, draws_tol=2e-3, stat_tol=5e-4)
    finally:
        r.close()


def test_texture_lookup_vs_reference_vectors_and_oracle(parsed, flat, oracle_scene):
    """Texture.query on the device: the reference's own lookups (fixture) and the oracle on a dense coordinate sweep."""
    from adapt_amd.renderer import DeviceScene
    g = golden("scene_textured.npz")
    sc = DeviceScene(flat("textured"))
    try:
        tin, tout = g["texq_in"], g["texq_out"]
        got = sc.texture_query(tin[:, 0], tin[:, 1], tin[:, 2:4])
        bad = (got.view(np.uint32) != tout.view(np.uint32)).any(axis=1)
        assert int(bad.sum()) == 0                                     # as on the CPU (test_oracle_golden.test_texture_query_bit_exact: no recorded lookup differs, wrap seams included)
        rs = np.random.RandomState(3)
        fs = flat("textured")
        maps, objs = np.nonzero(fs.tex_i[:, :, 0].T > -255)
        k = rs.randint(len(maps), size=20000)
        uv = rs.uniform(-3, 4, size=(20000, 2)).astype(np.float32)
        a = sc.texture_query(maps[k], objs[k], uv)
        b = oracle_scene("textured").texture_query(maps[k], objs[k], uv)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    finally:
        sc.close()


# ---- volumetric path tracer (VolumeRenderer, renderer/vpt.py): homogeneous media, null surfaces, tracked light samples
from conftest import VPT_SCENE_TAGS  # noqa: E402


@pytest.mark.parametrize("tag", VPT_SCENE_TAGS)
def test_volumetric_hip_vs_reference_run_and_oracle(tag):
    """tests/gpu_cases.py volumetric_scene_vs_reference_run_and_oracle on the exact build"""
    from gpu_cases import volumetric_scene_vs_reference_run_and_oracle
    assert volumetric_scene_vs_reference_run_and_oracle(tag)["arithmetic"] == "exact"


@pytest.mark.parametrize("mode", ["bvh", "sweep", "tile"])
def test_volumetric_every_traversal_mode(mode, monkeypatch):
    """media_a (null fog cube, scattering glass ball, scattering world) under each closest-hit implementation: the transmittance walk
    and the free-path sampling see the same surfaces whichever one finds them."""
    from adapt_amd.renderer import VolumeRenderer
    from adapt_amd.scene_pack import make_config, pack_scene
    from oracle import binding as ob
    monkeypatch.setenv("APT_TRAVERSAL", mode)
    tup, g = scene_from_golden("media_a", "vptscene")
    w, h, spp = 64, 48, 8
    r = VolumeRenderer(*tup, width=w, height=h)
    try:
        assert r.info()["traversal"] == mode
        r.render(n_spp=spp)
        rc = make_config(tup[3], width=w, height=h, volumetric=True)
        ref, _, ost = ob.OracleScene(pack_scene(*tup), rc.cam_t).render(rc, spp)
        image_within(r.color.to_numpy(), ref, spp, 0.99, 1e-3, label=mode)
        counters_within(r.stats(), ost, 1e-3, 0, label=mode)
    finally:
        r.close()


def test_volumetric_partition_and_batch_invariance():
    """Two ranks' tiles side by side equal the single-rank image (RNG keyed by the global pixel), and one sample per batch equals
    the automatic batching: vpt_cbox takes one light sample per vertex, so no two float atomics ever meet on a radiance slot."""
    from adapt_amd.renderer import VolumeRenderer
    tup, g = scene_from_golden("vpt_cbox", "vptscene")
    w, h, spp = 64, 32, 6
    full = VolumeRenderer(*tup, width=w, height=h)
    full.render(n_spp=spp); ref = full.color.to_numpy(); full.close()
    one = VolumeRenderer(*tup, width=w, height=h, spp_per_batch=1)
    one.render(n_spp=spp); assert np.array_equal(one.color.to_numpy(), ref); one.close()
    img = np.zeros_like(ref)
    for rank in range(2):
        r = VolumeRenderer(*tup, width=w, height=h, rank=rank, world_size=2, band_width=16)
        r.render(n_spp=spp)
        img[r.plan.columns(rank)] = r.tile_accum()
        r.close()
    assert np.array_equal(img, ref)


def test_surface_tracer_ignores_media_like_the_reference():
    """`--type pt` on a scene with media: Renderer.render never looks at them (vanilla_renderer.py), so the image equals the oracle's
    surface-only render and differs from the volumetric one."""
    from adapt_amd.renderer import Renderer, VolumeRenderer
    from adapt_amd.scene_pack import make_config, pack_scene
    from oracle import binding as ob
    tup, g = scene_from_golden("vpt_volbox", "vptscene")
    w, h, spp = 48, 36, 8
    a = Renderer(*tup, width=w, height=h); a.render(n_spp=spp); pa = a.color.to_numpy(); a.close()
    b = VolumeRenderer(*tup, width=w, height=h); b.render(n_spp=spp); pb = b.color.to_numpy(); b.close()
    rc = make_config(tup[3], width=w, height=h)
    ref = ob.OracleScene(pack_scene(*tup), rc.cam_t).render(rc, spp)[0]
    m = image_metrics(pa / spp, ref / spp)
    assert m["frac_within"] >= 0.99 and m["relMSE"] <= 1e-3, m
    assert float(np.abs(pa - pb).mean()) > 1e-2


def test_medium_functions_vs_reference_vectors():
    """Free-path sampling, phase sampling / evaluation and transmittance on the device against the reference-run vectors: decisions
    (medium event or not, draws consumed) exact, floats to the per-call tolerance (device expf / logf / double-precision sincos
    against glibc's float functions)."""
    from adapt_amd.renderer import medium_probe
    g = golden("media_functions.npz")
    mi, mf = g["med_i"], g["med_f"]
    x = g["mfp_in"]; m = np.int32(x[:, 0])
    in7 = np.zeros((x.shape[0], 7), np.float32); in7[:, 0] = x[:, 1]
    out = medium_probe(mi[m], mf[m], 0, in7, seed=779)
    y = g["mfp_out"]
    assert np.array_equal(out[:, 0], y[:, 0]) and np.array_equal(out[:, 5], y[:, 5])          # same events, same number of draws
    assert close(out[:, 1:5], y[:, 1:5], rel=2e-5)     # a free path is -log(1 - eps) / u_e: relative error of logf near eps -> 0 is amplified
    x = g["scat_in"]; m = np.int32(x[:, 0])
    in7 = np.zeros((x.shape[0], 7), np.float32); in7[:, :3] = x[:, 1:4]
    out = medium_probe(mi[m], mf[m], 1, in7, seed=780)
    y = g["scat_out"]
    assert np.array_equal(out[:, 7], y[:, 7])
    assert close(out[:, :3], y[:, :3], rel=1e-5, abs_=2e-6) and close(out[:, 3:7], y[:, 3:7], rel=1e-5)
    x = g["eval_in"]; m = np.int32(x[:, 0])
    out = medium_probe(mi[m], mf[m], 2, x[:, 1:8])
    assert close(out[:, :4], g["eval_out"], rel=1e-5)


@pytest.mark.parametrize("tag", ["cbox", "balls_mono", "textured", "features_a", "microfacet"])
def test_volumetric_tracer_on_scenes_without_media(tag, renderer, parsed, oracle_scene):
    """`--type vpt` on surface-only scenes (the reference's default renderer type): no medium ever scatters, but the loop differs from
    the surface tracer's - roulette before the hit, emission against the geometric normal, no normal / bump maps (vpt.py never calls
    process_ns), albedo textures on every vertex - so it is checked against the oracle's volumetric loop, not against `pt`."""
    from adapt_amd.renderer import VolumeRenderer
    w, h, spp = 48, 36, 8
    tup = parsed(tag)
    r = VolumeRenderer(*tup, width=w, height=h)
    try:
        r.render(n_spp=spp)
        rc = make_config(tup[3], width=w, height=h, volumetric=True)
        ref, _, ost = oracle_scene(tag).render(rc, spp)
        image_within(r.color.to_numpy(), ref, spp, 0.99, 1e-3, label=tag)
        counters_within(r.stats(), ost, 1e-3, 0, label=tag)
    finally:
        r.close()


@pytest.mark.parametrize("name", ["volgrid_a", "volgrid_b"])
def test_grid_volume_hip_vs_reference_run_and_oracle(name):
    """tests/gpu_cases.py grid_volume_vs_reference_run_and_oracle on the exact build"""
    from gpu_cases import grid_volume_vs_reference_run_and_oracle
    assert grid_volume_vs_reference_run_and_oracle(name)["arithmetic"] == "exact"


def test_full_size_properties_volumetric_fog_box():
    """The volumetric bench workload (`bench.py --config v1`: fog Cornell box, 512x512, 16 bounces) at a reduced sample count, through
    properties that need no oracle at this size: sample additivity across calls and lanes (bit-exact: one light sample per vertex),
    statistics identities of the loop, the fog's visible effect, and a crop window that equals the same window of the full render."""
    import os
    from conftest import ROOT
    from adapt_amd.parsers.xml_parser import scene_parsing
    from adapt_amd.renderer import Renderer, VolumeRenderer
    tup = scene_parsing(os.path.join(ROOT, "scenes", "vpt"), "cbox_fog.xml")
    r = VolumeRenderer(*tup)
    assert (r.w, r.h, r.max_bounce, r.num_shadow_ray) == (512, 512, 16, 1) and r.info()["shade_variant"].startswith("volumetric, sorted by event: medium | lambertian")
    r.render(n_spp=24)
    st, img = r.stats(), r.color.to_numpy()
    n = 512 * 512 * 24
    assert st["n_samples"] == n and st["n_shade"] < st["n_extend"] and st["n_shadow"] <= st["n_shade"]       # null crossings extend without shading
    assert st["n_lit"] <= st["n_shadow_traced"] <= st["n_shadow"] and st["n_track"] >= st["n_shadow_traced"] and st["n_poisoned"] == 0
    assert np.isfinite(img).all() and img.min() >= 0
    two = VolumeRenderer(*tup)
    two.render(n_spp=10); two.render(n_spp=14)
    assert np.array_equal(two.color.to_numpy(), img) and two.cnt[None] == 24                               # 10 + 14 samples == 24 samples
    two.close()
    # the fog cube is where the small box stands: the surface tracer sees through the null surface's object as if it were black
    # (a null BSDF scatters nothing there), the volumetric tracer sees light scattered inside it
    s = Renderer(*tup); s.render(n_spp=24); simg = s.color.to_numpy(); s.close()
    assert float(np.abs(simg - img).mean()) > 0.05 * float(img.mean())
    # crop window: same pixels as in the full frame (RNG keyed by the global pixel)
    prop = dict(tup[3]); prop["film"] = dict(prop["film"], crop_x=256, crop_y=200, crop_rx=40, crop_ry=30)
    c = VolumeRenderer(tup[0], tup[1], tup[2], prop)
    c.render(n_spp=24)
    cimg = c.color.to_numpy()
    assert np.array_equal(cimg[c.start_x:c.end_x, c.start_y:c.end_y], img[c.start_x:c.end_x, c.start_y:c.end_y])
    assert not cimg[:c.start_x].any() and not cimg[c.end_x:].any()
    c.close(); r.close()


def test_both_tracers_estimate_the_same_image_without_media(parsed):
    """Independent check of the two loops against each other: on a scene without media the surface tracer and the volumetric tracer
    are different estimators (roulette placement, emission weighting, draw order) of the same integral, so their converged images must
    agree within Monte-Carlo noise.  Cornell box, 48x48, 4096 spp each: region means within 2 %."""
    from adapt_amd.renderer import Renderer, VolumeRenderer
    tup = parsed("cbox")
    a = Renderer(*tup, width=48, height=48); a.render(n_spp=4096); ia = a.pixels.to_numpy().astype(np.float64); a.close()
    b = VolumeRenderer(*tup, width=48, height=48, seed=7); b.render(n_spp=4096); ib = b.pixels.to_numpy().astype(np.float64); b.close()
    assert np.isfinite(ia).all() and np.isfinite(ib).all()
    for (x0, x1, y0, y1) in ((0, 48, 0, 48), (0, 16, 8, 40), (32, 48, 8, 40), (12, 36, 0, 12), (12, 36, 30, 48)):
        ma, mb = ia[x0:x1, y0:y1].mean(axis=(0, 1)), ib[x0:x1, y0:y1].mean(axis=(0, 1))
        assert np.all(np.abs(ma - mb) <= 0.02 * np.maximum(ma, mb) + 1e-4), ((x0, x1, y0, y1), ma, mb)


def test_many_small_objects_fall_back_to_the_wave_sweep(parsed, monkeypatch):
    """The tiled sweep keeps a list per object in LDS; beyond 34 objects those lists no longer fit a CU and the renderer has to pick
    the plain wave sweep instead of failing at launch.  Cornell box with its five wall quads repeated to 38 objects / 96 primitives
    (coincident copies: the sweep resolves ties in the reference's object order, so the oracle image is matched exactly as usual)."""
    import copy
    from adapt_amd.renderer import Renderer
    from adapt_amd.scene_pack import pack_scene
    from oracle import binding as ob
    em, arr, objs, prop = parsed("cbox")
    arr = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in arr.items()}
    objs = list(objs)
    first = np.cumsum([0] + [o.tri_num for o in objs])
    quads = [k for k, o in enumerate(objs) if o.tri_num == 2 and o.type == 0]
    assert len(quads) >= 5
    extra = []
    while len(objs) + len(extra) < 38:
        extra.append(quads[len(extra) % len(quads)])
    for k in extra:
        sl = slice(first[k], first[k] + 2)
        for key in ("primitives", "n_g", "n_s", "uvs"):
            arr[key] = np.concatenate([arr[key], arr[key][sl]], axis=0)
        objs.append(copy.copy(objs[k]))
    tup = (em, arr, objs, prop)
    assert len(objs) == 38 and arr["primitives"].shape[0] == 34 + 2 * len(extra) <= 96
    r = Renderer(*tup, width=48, height=48)
    try:
        assert r.info()["traversal"] == "sweep"
        r.render(n_spp=8)
        rc = make_config(prop, width=48, height=48)
        ref, cnt, ost = ob.OracleScene(pack_scene(*tup), rc.cam_t).render(rc, 8)
        m = image_metrics(r.pixels.to_numpy(), ref / np.float32(cnt))
        assert m["frac_within"] >= 0.995 and m["relMSE"] <= 1e-4, m
        assert abs(r.stats()["n_draws"] - ost["n_draws"]) <= 2e-4 * ost["n_draws"]
    finally:
        r.close()
    monkeypatch.setenv("APT_TRAVERSAL", "tile")          # asking for the tiled sweep explicitly must not select it either
    r2 = Renderer(*tup, width=32, height=32)
    assert r2.info()["traversal"] == "sweep"
    r2.render(n_spp=1); r2.synchronize(); r2.close()


@pytest.mark.parametrize("tag,vol", [("cbox", False), ("balls_mono", False), ("balls_mono", True)])
def test_no_light_samples_at_all(tag, vol, parsed, oracle_scene):
    """num_shadow_ray = 0 (no next-event estimation: only paths that run into an emitter carry light; upstream then uses a sample
    weight of 1, path_tracer.py:71-74).  Queues, class counters and the walk passes must cope with a shadow stage that never runs,
    sorted and unsorted, in both tracers."""
    from adapt_amd.renderer import Renderer, VolumeRenderer
    tup = parsed(tag)
    cls = VolumeRenderer if vol else Renderer
    r = cls(*tup, width=40, height=40, num_shadow_ray=0)
    try:
        r.render(n_spp=16)
        st = r.stats()
        assert st["n_shadow"] == 0 and st["n_shadow_traced"] == 0 and st["n_samples"] == 40 * 40 * 16
        rc = make_config(tup[3], width=40, height=40, num_shadow_ray=0, volumetric=vol)
        ref, cnt, ost = oracle_scene(tag).render(rc, 16)
        m = image_metrics(r.pixels.to_numpy(), ref / np.float32(cnt))
        assert m["frac_within"] >= 0.995 and m["relMSE"] <= 1e-4, (tag, vol, m)
        assert abs(st["n_shade"] - ost["n_shade"]) <= 2e-4 * ost["n_shade"] + 2
    finally:
        r.close()


@pytest.mark.parametrize("vol", [False, True])
def test_degenerate_bounce_limits(vol, parsed, oracle_scene):
    """max_bounce = 0 and 1: the surface tracer's for-loop does not run at all with 0 (black image), the volumetric tracer's while-loop
    always runs its body once (vpt.py:161-245) - both as the oracle."""
    from adapt_amd.renderer import Renderer, VolumeRenderer
    tup = parsed("balls_mono")
    for mb in (0, 1):
        r = (VolumeRenderer if vol else Renderer)(*tup, width=32, height=32, max_bounce=mb)
        try:
            r.render(n_spp=8)
            rc = make_config(tup[3], width=32, height=32, max_bounce=mb, volumetric=vol)
            ref, cnt, ost = oracle_scene("balls_mono").render(rc, 8)
            m = image_metrics(r.pixels.to_numpy(), ref / np.float32(cnt))
            assert m["frac_within"] >= 0.995, (vol, mb, m)
            assert abs(r.stats()["n_shade"] - ost["n_shade"]) <= 2
            if not vol and mb == 0:
                assert not r.color.to_numpy().any()
        finally:
            r.close()


@pytest.mark.parametrize("w,h,world,bw", [(50, 30, 3, 4), (37, 20, 8, 4), (64, 17, 5, 7)])
def test_ragged_film_partitions(w, h, world, bw, renderer):
    """Widths that are not a multiple of band x ranks: the last band is short, ranks own different numbers of columns (some of the
    8 ranks of a 37-pixel film own a single band) - the assembled tiles still equal the single-renderer image, bit for bit."""
    from adapt_amd.tiles import TilePlan, assemble
    full = renderer("cbox", width=w, height=h)
    full.render(n_spp=4)
    ref = full.color.to_numpy()
    plan = TilePlan(w, h, bw, world)
    tiles = []
    for rank in range(world):
        if len(plan.columns(rank)) == 0:
            tiles.append(np.zeros((0, h, 3), np.float32)); continue
        r = renderer("cbox", width=w, height=h, rank=rank, world_size=world, band_width=bw)
        r.render(n_spp=4)
        tiles.append(r.tile_accum())
        assert tiles[-1].shape == (len(plan.columns(rank)), h, 3)
    assert np.array_equal(assemble(plan, tiles), ref)


def test_device_bvh_builder_gives_the_same_answers(bunnies_small, monkeypatch):
    """APT_BVH_BUILDER=lbvh | ploc: the binary tree is built on the GPU (csrc/bvh_gpu.hip: Morton sort, then either Karras' radix tree +
    bottom-up fit, or rounds of nearest-neighbour merging by box area) instead of by the host's binned SAH.  Different trees, the same answers: closest hits (primitive, t, barycentrics) and occlusion flags equal
    the oracle's brute force exactly, and on a scene with one light sample per vertex the image is BIT-identical to the SAH build's."""
    from adapt_amd.renderer import Renderer
    from adapt_amd.scene_pack import pack_scene
    from adapt_amd.synth import bunny_field
    from oracle import binding as ob
    rs = np.random.RandomState(21)
    n = 8000
    o = rs.uniform([0.3, 0.2, 0.3], [5.2, 5.2, 5.2], size=(n, 3)).astype(np.float32)
    d = rs.normal(size=(n, 3)).astype(np.float32); d /= np.linalg.norm(d, axis=1, keepdims=True)
    tmax = rs.uniform(0.2, 6.0, n).astype(np.float32)
    sc = ob.OracleScene(pack_scene(*bunnies_small), make_config(bunnies_small[3]).cam_t)
    _, prim_o, t_o, uv_o, _ = sc.intersect(o, d)
    occ_o = sc.occluded(o, d, tmax)
    field = bunny_field(levels=1)
    cfg = dict(field[3]); cfg["film"] = {"width": 1280, "height": 720, "crop_x": 640, "crop_y": 330, "crop_rx": 60, "crop_ry": 40}
    images = {}
    for builder in ("sah", "lbvh", "ploc"):
        monkeypatch.setenv("APT_BVH_BUILDER", builder)
        r = Renderer(*bunnies_small, width=64, height=64)
        assert r.info()["bvh_builder"] == builder                 # the builder asked for built the tree: no PLOC -> LBVH retry, no host fallback
        prim, t, uv = r.intersect(o, d)
        assert np.array_equal(prim, prim_o) and np.array_equal(t, t_o) and np.array_equal(uv[prim >= 0], uv_o[prim >= 0]), builder
        assert np.array_equal(r.occluded(o, d, tmax), occ_o), builder
        r.close()
        f = Renderer(field[0], field[1], field[2], cfg)
        assert f.info()["bvh_builder"] == builder
        f.render(n_spp=3)
        images[builder] = f.color.to_numpy()
        assert f.stats()["n_samples"] == 3 * 120 * 80
        f.close()
    assert np.array_equal(images["sah"], images["lbvh"]) and np.array_equal(images["sah"], images["ploc"]) and images["sah"].max() > 0


def test_million_primitive_scene_takes_the_device_builder(monkeypatch):
    """Above a million primitives the tree is built on the device (PLOC) by default, the collapse and the record tables on host threads.
    The 1.14 M-triangle bunny field: same closest hits (primitive, t, barycentrics) and occlusion flags as with the host SAH builder,
    on rays through the field; a cropped window renders to the same image bit for bit."""
    from adapt_amd.renderer import Renderer
    from adapt_amd.synth import bunny_field
    field = bunny_field(levels=4)
    assert field[1]["primitives"].shape[0] >= 1000000
    cfg = dict(field[3]); cfg["film"] = {"width": 1280, "height": 720, "crop_x": 640, "crop_y": 330, "crop_rx": 48, "crop_ry": 32}
    rs = np.random.RandomState(77)
    n = 20000
    o = rs.uniform([0.3, 0.2, -1.0], [5.2, 5.2, 1.0], size=(n, 3)).astype(np.float32)
    tgt = rs.uniform([0.5, 0.0, 1.0], [5.0, 2.0, 5.0], size=(n, 3)).astype(np.float32)
    d = tgt - o; d /= np.linalg.norm(d, axis=1, keepdims=True)
    tmax = rs.uniform(0.5, 8.0, n).astype(np.float32)
    out = {}
    for builder in (None, "sah"):
        if builder is None:
            monkeypatch.delenv("APT_BVH_BUILDER", raising=False)
        else:
            monkeypatch.setenv("APT_BVH_BUILDER", builder)
        r = Renderer(field[0], field[1], field[2], cfg)
        try:
            assert r.info()["traversal"] == "bvh"
            assert r.info()["bvh_builder"] == ("ploc" if builder is None else "sah")      # what the test's name says: otherwise it compares the SAH tree with itself
            prim, t, uv = r.intersect(o, d)
            occ = r.occluded(o, d, tmax)
            r.render(n_spp=2)
            out[builder] = (prim, t, uv, occ, r.color.to_numpy())
        finally:
            r.close()
    a, b = out[None], out["sah"]
    assert (a[0] >= 0).mean() > 0.9 and len(np.unique(a[0])) > 3000
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)
    assert a[4].max() > 0


@pytest.mark.parametrize("builder", ["sah", "lbvh", "ploc"])
def test_tree_builders_on_degenerate_inputs(builder, monkeypatch):
    """What trips agglomerative and radix builders: forty COINCIDENT triangles (identical boxes and centroids: every Morton key ties, every
    union area ties - PLOC must still find a mutual pair each round), a sliver fan sharing one edge, and a scene of just two primitives.
    Closest hits equal the oracle's brute force bit for bit; coincident triangles resolve to the lowest primitive index, as upstream."""
    from adapt_amd.renderer import Renderer
    from adapt_amd.scene_pack import pack_scene
    from adapt_amd.synth import _Builder, _brdf, _room, _sensor, _spot
    from oracle import binding as ob
    monkeypatch.setenv("APT_BVH_BUILDER", builder)
    monkeypatch.setenv("APT_TRAVERSAL", "bvh")
    white = _brdf("lambertian", "#BDBDBD")
    light = [_spot("6.0, 6.0, 6.0", "100.0", (2.7, 5.2, 2.7), (0.0, -1.0, 0.1), 40.0, "s")]
    tri = np.float32([[[2.0, 1.0, 2.5], [3.4, 1.0, 2.5], [2.0, 2.6, 2.5]]])
    fan = np.float32([[[1.0, 0.5, 3.0], [1.0, 3.5, 3.0], [1.0 + 1e-3 * (k + 1), 2.0, 3.0 - 0.2 * k]] for k in range(9)])
    scenes = []
    b = _Builder(); _room(b, white, white, white); b.mesh(np.repeat(tri, 40, axis=0), white); b.mesh(fan, white)
    scenes.append(b.finish(light, _sensor(64, 64, 4, 1)))
    b = _Builder(); b.mesh(np.concatenate([tri, tri + np.float32([0.3, 0.2, 0.8])]), white)
    scenes.append(b.finish(light, _sensor(64, 64, 4, 1)))
    # the room plus 30 spheres (the builders' sphere branch): tiny, large, overlapping, concentric, and two identical ones
    b = _Builder(); _room(b, white, white, white)
    rs = np.random.RandomState(32)
    balls = [((2.3, 1.8, 2.7), 1e-3), ((3.2, 2.9, 2.4), 2e-3), ((2.6, 1.6, 2.8), 1.1), ((1.6, 2.6, 3.0), 0.9)]                   # tiny, large (and overlapping)
    balls += [((1.4, 1.0, 2.4), r) for r in (0.05, 0.2, 0.4, 0.6)]                                                               # concentric
    balls += [((3.3, 3.3, 2.3), 0.3)] * 2                                                                                       # identical
    balls += [(tuple(rs.uniform([1.0, 0.5, 2.0], [3.6, 3.6, 3.4])), float(rs.uniform(0.05, 0.5))) for _ in range(30 - len(balls))]
    assert len(balls) == 30
    for centre, radius in balls:
        b.sphere(centre, radius, white)
    scenes.append(b.finish(light, _sensor(64, 64, 4, 1)))
    rs = np.random.RandomState(31)
    for tup in scenes:
        n = 6000
        o = rs.uniform([0.3, 0.2, -2.0], [5.2, 5.2, 1.5], size=(n, 3)).astype(np.float32)
        tgt = rs.uniform([1.0, 0.5, 2.0], [3.6, 3.6, 3.4], size=(n, 3)).astype(np.float32)
        d = tgt - o; d /= np.linalg.norm(d, axis=1, keepdims=True)
        tmax = rs.uniform(0.5, 8.0, n).astype(np.float32)
        fs = pack_scene(*tup)
        sc = ob.OracleScene(fs, make_config(tup[3]).cam_t)
        _, prim_o, t_o, uv_o, _ = sc.intersect(o, d)
        is_sphere_prim = np.repeat(fs.obj_info[:, 2], fs.obj_info[:, 1]).astype(bool)
        r = Renderer(*tup, width=32, height=32)
        try:
            assert r.info()["traversal"] == "bvh" and r.info()["bvh_builder"] == builder        # the builder asked for, not a fallback
            prim, t, uv = r.intersect(o, d)
            assert (prim_o >= 0).sum() > n // 10
            tri_hit = (prim >= 0) & ~is_sphere_prim[np.maximum(prim, 0)]    # barycentrics are only defined (and used) for triangles
            assert is_sphere_prim.sum() in (0, 30) and (not is_sphere_prim.any() or (is_sphere_prim[prim_o[prim_o >= 0]]).sum() > n // 10)
            assert np.array_equal(prim, prim_o) and np.array_equal(t, t_o) and np.array_equal(uv[tri_hit], uv_o[tri_hit])
            assert np.array_equal(r.occluded(o, d, tmax), sc.occluded(o, d, tmax))
            r.render(n_spp=2)
            assert np.isfinite(r.color.to_numpy()).all()
        finally:
            r.close()


# ---------------------------------------------------------------- what the driver launches on the 8-GPU node: bench.py under torch.distributed.run
def test_two_and_three_rank_bench_on_one_gpu_equal_the_single_rank_image(tmp_path):
    """bench.py exactly as the driver starts it for N > 1 (torch.distributed.run, one process per rank), except that every rank renders
    on cuda:0 and the tiles travel over gloo: real `Renderer(rank, world_size)` instances in separate processes, the all_gather, the
    tile assembly.  Weak scaling (N x the samples) and strong scaling (same film and samples) both reproduce the single-process
    image BIT FOR BIT, because the Philox key is the global pixel; the JSON line carries the contract's fields and per-rank timings."""
    one, img1 = GC.run_bench(1, ["--spp", "6"], tmp_path, "n1")
    assert one["n_gpus"] == 1 and one["scaling"] == "weak" and one["config"]["spp_per_step"] == 6 and img1.shape == (256, 256, 3)
    weak, img2 = GC.run_bench(2, ["--spp", "3"], tmp_path, "n2w")                        # 2 ranks x 3 spp = 6 spp per step
    assert weak["n_gpus"] == 2 and weak["scaling"] == "weak" and weak["config"]["spp_per_step"] == 6
    assert np.array_equal(img2, img1)
    strong, img3 = GC.run_bench(3, ["--spp", "6", "--scaling", "strong"], tmp_path, "n3s")
    assert strong["n_gpus"] == 3 and strong["scaling"] == "strong" and strong["config"]["spp_per_step"] == 6
    assert np.array_equal(img3, img1)
    for d in (weak, strong):
        pr = d["per_rank"]
        assert len(pr["render_ms_per_step"]) == d["n_gpus"] and len(pr["gather_ms_per_step"]) == d["n_gpus"] and min(pr["render_ms_per_step"]) > 0
        assert sum(pr["samples"]) == 256 * 256 * 6                                          # the ranks' pixels partition the film
        for k in ("metric", "value", "unit", "steps", "warmup", "ms_per_step", "higher_is_better", "vs_baseline", "dtype", "data", "config", "roofline"):
            assert k in d
        assert d["value"] > 0 and d["roofline"]["bound"] in ("hbm", "valu") and "frac_credited" in d["roofline"] and {"shade"} <= set(d["roofline"]["stages"]) <= {"extend", "shade", "shadow"}      # (no extend / shadow stage where the shade kernel traces its own rays: stages.hpp "rays traced in place")
