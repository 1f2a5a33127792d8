"""The PRODUCT build (libadapt_mi.so, `arithmetic: fast`: what bench.py, smoke() and render.py run) against the oracle, the reference-run
fixtures and the exact build, at SURVEY 8(d)'s stated tolerances.

What differs from the exact build (tests/test_gpu_parity.py): scenes of up to 96 primitives take the FLAT SWEEP (traverse.hpp) -
precomputed-transform records, parallelograms as one record, explicit FMAs, one reciprocal per test, two rays per lane - instead of the
reference's loop operation for operation.  The shading arithmetic is the same in both builds.  Stated tolerances:
  * intersector: `t` within 1e-5 relative, same primitive unless tied (a different primitive is acceptable only at the same distance);
  * images, same Philox stream: >= 99 % of pixels within 1e-3 (1 + |x|) at 64 spp on C1 and relMSE <= 1e-4; a path whose hit moved by
    an ulp can flip a branch and re-draw the path, so scenes with specular chains (glass, mirrors: the error of a hit point is amplified
    by every bounce) are held to relMSE and to the path statistics instead of the per-pixel fraction;
  * path statistics (shaded vertices, light samples, random numbers drawn): within 5e-4 - a systematic deviation (a quirk of the
    reference not reproduced) shows here first: coplanar faces and NaN slabs both moved these counts by 0.3-1.2 % before they were handled;
  * statistical cross-check against a CPU render with another seed.
Scenes too large for the flat sweep walk the same 8-wide tree in both builds; the product build tests the tree's leaves with the flat sweep's
precomputed-transform arithmetic (same tolerance), everything else is shared.
"""
import os

import numpy as np
import pytest

import gpu_cases as GC
from conftest import SCENES, golden, image_metrics, record_metric
from flat_cases import _quad_soup
from gpu_cases import counters_within, image_within
from parity_bounds import COUNTER_TOL, PRODUCT_IMAGE_CASES as IMAGE_CASES, SAME_SEED_FRACTION_OF_NOISE, VPT_PRODUCT_BOUNDS
from adapt_amd.scene_pack import make_config

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _fast_build():
    from adapt_amd import _lib
    prev = _lib.use("fast")
    yield
    _lib.use(prev)


@pytest.fixture
def renderer(parsed):
    """tests/gpu_cases.py renderer_factory: every renderer a test makes is closed when that test ends"""
    with GC.renderer_factory(parsed) as make:
        yield make


def test_the_product_build_is_the_fast_one_and_small_scenes_take_the_flat_sweep(renderer):
    from adapt_amd import _lib
    assert _lib.arithmetic() == "fast" and b"arithmetic: fast" in _lib.load().apt_version()
    maps = open("/proc/self/maps").read()
    import os
    assert os.path.realpath(_lib.LIB_PATHS["fast"]) in maps
    for tag in ("cbox", "balls_mono", "glass_box", "features_a"):
        info = renderer(tag, width=32, height=32).info()
        assert info["traversal"] == "flat" and info["arithmetic"] == "fast", (tag, info)
    ex = renderer("cbox", width=32, height=32, exact=True).info()
    assert ex["arithmetic"] == "exact" and ex["traversal"] == "tile"


def _rays(n, seed):
    rs = np.random.RandomState(seed)
    o = rs.uniform([0.1, 0.1, 0.1], [5.4, 5.3, 5.4], size=(n, 3)).astype(np.float32)
    d = rs.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    tmax = rs.uniform(0.2, 8.0, n).astype(np.float32)
    return o, d, tmax


def _check_hits(prim, t, uv, prim_o, t_o, uv_o, is_tri, d, normals, tris=None):
    """t within 1e-5 relative, same primitive unless tied.  A ray-plane distance is a quotient of a height over the plane and
    a cosine, and the height carries the rounding of coordinates of size ~5 (a few 1e-7) whatever formula computes it - upstream's
    included: where the height itself is small the RELATIVE error of t is unbounded, so such hits are held to the equivalent absolute
    statement, the hit point moving by less than 1e-6 of the scene's extent along the surface normal."""
    same = prim == prim_o
    hit = same & (prim_o >= 0)
    dt = np.abs(t.astype(np.float64) - t_o.astype(np.float64))
    rel_ok = dt <= 1e-5 * np.abs(t_o)
    tri = hit & is_tri
    cos = np.abs(np.einsum("ij,ij->i", normals[prim_o[tri]].astype(np.float64), d[tri].astype(np.float64)))
    assert np.all(rel_ok[tri] | (dt[tri] * cos <= 5.5e-6)), (float((dt[tri] / np.abs(t_o[tri])).max()), float((dt[tri] * cos).max()))
    assert rel_ok[tri].mean() >= 0.995                                              # the relative statement holds for all but rays that start within ~1e-2 of a surface
    sph = hit & ~is_tri                                                             # spheres: the reference's test operation for operation - same bits
    assert np.array_equal(t[sph], t_o[sph])
    assert np.all(t[same & (prim_o < 0)] == np.float32(1e7))
    # a different primitive: only at the same distance (shared edges, coplanar faces), or a hit / miss decided in the last bit on a
    # silhouette edge (at most a handful of rays in 10^5)
    diff = ~same
    tied = np.abs(t[diff] - t_o[diff]) <= 1e-5 * np.maximum(np.abs(t_o[diff]), 1e-2)
    assert diff.mean() <= 5e-3 and (~tied).sum() <= max(3, int(2e-5 * len(prim))), (diff.sum(), (~tied).sum())
    if tris is None:                                                                # Cornell-sized primitives: the barycentrics themselves
        assert np.abs(uv[tri] - uv_o[tri]).max() <= 5e-5 if tri.any() else True
    elif tri.any():
        # meshes of small triangles: a barycentric is a length divided by an edge, so the statement that does not depend on the triangle's
        # size is the POINT the barycentrics name - it moves by no more than the hit point may move along the ray (1e-5 t, and the absolute
        # floor above)
        e1, e2 = (tris[prim_o[tri], 1] - tris[prim_o[tri], 0]).astype(np.float64), (tris[prim_o[tri], 2] - tris[prim_o[tri], 0]).astype(np.float64)
        dP = (uv[tri, 0:1] - uv_o[tri, 0:1]).astype(np.float64) * e1 + (uv[tri, 1:2] - uv_o[tri, 1:2]).astype(np.float64) * e2
        assert np.all(np.linalg.norm(dP, axis=1) <= 1e-5 * np.abs(t_o[tri]) + 5.5e-6), float(np.linalg.norm(dP, axis=1).max())


@pytest.mark.parametrize("tag,kw", [("cbox", {}), ("glass_box", {}), ("balls_mono", {}), ("balls_mono", {"num_shadow_ray": 1}), ("features_b", {}), ("textured", {"num_shadow_ray": 3})])
def test_fix_up_lists_carry_every_ray_when_asked_to(tag, kw, renderer, monkeypatch):
    """The hot flat kernels hand the rays they cannot settle to fix-up launches (stages.hpp "Fix-up lists").  APT_FLAT_DEFER_ALL=1 makes
    EVERY ray such a ray: extend and shadow entries of all bounces then travel through the lists - unsorted and class-sorted, one light
    sample per vertex and samples queued by vertex - and are resolved by the reference-order sweep, i.e. with the exact build's
    arithmetic.  Where the exact build itself sweeps in reference order (every scene without a 6-primitive object takes its `sweep`
    mode; the others its tiled twin, which returns the same hits), path statistics must then be the exact build's to the last count, and images
    bit for bit (one light sample per vertex) or to the last bit of a differently associated sum (several)."""
    w, h, spp = 48, 40, 6
    e = renderer(tag, width=w, height=h, exact=True, **kw)
    e.render(n_spp=spp); ref = e.color.to_numpy(); est = e.stats()
    monkeypatch.setenv("APT_FLAT_DEFER_ALL", "1")
    f = renderer(tag, width=w, height=h, **kw)
    assert f.info()["traversal"] == "flat" and f.info()["arithmetic"] == "fast"
    f.render(n_spp=spp); img = f.color.to_numpy(); st = f.stats()
    # Rounds 3-5 asserted equality to the last count and bit here: the product build then shaded with the exact build's arithmetic.  Since round 6
    # it evaluates cos / sin / pow in float and the non-delta shading code's divisions and roots with the 1-ulp instructions (adapt_amd/build.py), so a sampled direction differs in its last bit now and then and a handful of the
    # ~10^4 paths of this render take another branch: counts agree to 2.5e-3 (measured with every ray deferred: 7e-5 .. 1.7e-3 on renders of ~10^4 vertices), pixels as far as a
    # re-drawn path among six samples lets them.  What "every ray through the lists" must still deliver to the last count is the SAMPLES.
    assert st["n_samples"] == est["n_samples"]
    for k in ("n_extend", "n_shade", "n_shadow", "n_shadow_traced", "n_lit", "n_draws"):
        assert abs(st[k] - est[k]) <= max(2.5e-3 * est[k], 8), (k, st[k], est[k])
    m = image_metrics(img / spp, ref / spp)
    record_metric(f"fix-up lists carry every ray {tag} {kw}", m)
    assert m["frac_within"] >= 0.95 and abs(np.nanmean(img) - np.nanmean(ref)) <= 0.02 * np.nanmean(ref), m


@pytest.mark.parametrize("tag,kw", [("cbox", {}), ("glass_box", {}), ("balls_mono", {}), ("balls_mono", {"num_shadow_ray": 1}), ("features_b", {}), ("textured", {"num_shadow_ray": 3})])
def test_fix_up_lists_match_the_reference_order_sweep_of_the_same_build(tag, kw, renderer, monkeypatch):
    """The sibling of the test above inside the product build: every ray through the fix-up lists (APT_FLAT_DEFER_ALL=1) against the
    same library with its traversal forced to the reference-order mode the exact build picks for the scene (`sweep`, or `tile` where
    an object has 6 primitives).  Both resolve every ray with the reference-order intersector and shade with the same arithmetic, so
    the path statistics agree to the last count; the image is bit-equal with one light sample per vertex and, with several, equal up
    to the association of the light-sample sum (rtol 4 ulp)."""
    w, h, spp = 48, 40, 6
    mode = renderer(tag, width=8, height=8, exact=True, **kw).info()["traversal"]
    assert mode in ("sweep", "tile")
    monkeypatch.setenv("APT_TRAVERSAL", mode)
    s = renderer(tag, width=w, height=h, **kw)
    assert s.info()["traversal"] == mode and s.info()["arithmetic"] == "fast"
    s.render(n_spp=spp); ref = s.color.to_numpy(); sst = s.stats()
    monkeypatch.delenv("APT_TRAVERSAL")
    monkeypatch.setenv("APT_FLAT_DEFER_ALL", "1")
    f = renderer(tag, width=w, height=h, **kw)
    assert f.info()["traversal"] == "flat" and f.info()["arithmetic"] == "fast"
    f.render(n_spp=spp); img = f.color.to_numpy(); st = f.stats()
    for k in ("n_samples", "n_extend", "n_shade", "n_shadow", "n_shadow_traced", "n_lit", "n_draws"):
        assert st[k] == sst[k], (k, st[k], sst[k])
    if f.num_shadow_ray == 1:
        assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))
    same = (img == ref) | (np.isnan(img) & np.isnan(ref))
    rel = np.abs(img.astype(np.float64) - ref) / np.maximum(np.abs(ref.astype(np.float64)), np.finfo(np.float32).tiny)
    record_metric(f"fix-up lists vs reference-order sweep, product build {tag} {kw}",
                  {"mode": mode, "bit_equal_frac": float(same.mean()), "max_rel": float(np.where(same, 0.0, rel).max())})
    assert np.all(same | (rel <= 4 * 2.0 ** -23))


@pytest.mark.parametrize("tag,kw", [("cbox", {}), ("cbox", {"max_bounce": 1}), ("glass_box", {"num_shadow_ray": 1}), ("balls_mono", {"num_shadow_ray": 1}), ("textured", {"num_shadow_ray": 1})])
def test_rays_traced_in_place_render_the_staged_pipeline_s_image(tag, kw, renderer, monkeypatch):
    """Unsorted flat-sweep renders with one light sample per vertex run ONE launch per bounce (shade_stage.hpp "rays traced in place",
    APT_FUSED=2, the default): the shade kernel sweeps its light sample and its continuation ray itself, k_generate the camera rays, and
    the rays that need the reference-order code are served by the next launch's prologue.  Against the staged pipeline - APT_FUSED=0
    (extend + fix-up + shade + shadow) - the ray, the records and the arithmetic per (ray, record) are the same, so
    the image is the same up to the few rays the pair-wise sweep defers in addition (a plain record next to a coplanar group), and the
    path statistics agree to 1e-4; rays that hit nothing are counted although they never enter a queue."""
    w, h, spp = 64, 48, 16
    out = {}
    monkeypatch.setenv("APT_SORTED", "0")                       # (scenes of several material classes: one all-models kernel instead of class queues)
    for mode in ("0", "2"):
        monkeypatch.setenv("APT_FUSED", mode)
        r = renderer(tag, width=w, height=h, **kw)
        assert r.info()["traversal"] == "flat"
        name = r.info()["shade_variant"]
        assert ("rays traced in place" in name) == (mode == "2"), name
        r.render(n_spp=spp)
        out[mode] = (r.color.to_numpy(), r.stats())
    img0, st0 = out["0"]
    for mode in ("2",):
        img, st = out[mode]
        assert st["n_samples"] == st0["n_samples"] and st["n_extend"] >= st["n_samples"]
        for k in ("n_extend", "n_shade", "n_shadow", "n_shadow_traced", "n_lit", "n_draws"):
            assert abs(st[k] - st0[k]) <= max(2, 1e-4 * st0[k]), (mode, k, st[k], st0[k])
        fin = np.isfinite(img0) & np.isfinite(img)
        assert fin.mean() > 0.999
        close = np.abs(img - img0)[fin] <= 1e-4 * (1.0 + np.abs(img0[fin]))
        assert close.mean() >= 0.99, (mode, float(close.mean()))


FULL_SIZE = os.environ.get("APT_FULL_SIZE_PARITY") == "1"


@pytest.mark.skipif(not FULL_SIZE, reason="minutes of host time for the oracle: APT_FULL_SIZE_PARITY=1 (the run of record is profiles/r0N_full_size_parity.log)")
@pytest.mark.parametrize("tag,spp", [("cbox", 1024), ("balls_mono", 1024)])
def test_full_size_parity_c2_c3_product_build(tag, spp, renderer, parsed, oracle_scene, capsys):
    """BASELINE configs[1] and [2] at their FULL size, product build against the oracle on the same Philox stream, every pixel, held to
    SURVEY 8(d)'s tolerance (the exact build's twin in test_gpu_parity.py is held to 1e-7)."""
    # non-finite pixels (upstream lets +inf through, vanilla_renderer.py:119): the oracle's, or zero-pdf knife-edges and nothing else ("explained")
    info = GC.full_size_parity(renderer, parsed, oracle_scene, capsys, tag, spp, 0.99, 1e-4, 5e-4, non_finite="explained")
    assert info["arithmetic"] == "fast" and info["traversal"] == "flat"


def test_c2_full_frame_every_pixel_128_spp_product_build(renderer, parsed, oracle_scene):
    """BASELINE configs[1] at its full film size and bounce count, 128 of its 1024 spp, product build against the oracle on the same Philox
    stream, EVERY pixel (~5 s of the box's host threads: un-gated, unlike the 1024-spp comparison above).  SURVEY 8(d) asks for 99 % of the
    pixels within 1e-3 (1 + x) and relMSE 1e-4; the run of record at 1024 spp measured 99.96 % and 5.3e-8, and the bounds here are
    that measurement with a margin of two."""
    info = GC.full_frame_every_pixel(renderer, parsed, oracle_scene, "cbox", 128, 0.998, 2e-6, 2e-5, metric="c2 full frame 128 spp product build")
    assert info["arithmetic"] == "fast" and info["traversal"] == "flat"


def test_c3_full_frame_every_pixel_64_spp_product_build(renderer, parsed, oracle_scene):
    """BASELINE configs[2] (csphere: glass, mirror, Fresnel blend, four light samples per vertex, 16 bounces) at its full film size, 64 of its
    1024 spp, product build against the oracle on the same Philox stream, EVERY pixel of the 512 x 512 film, un-gated (round 5 had a 128 x 96
    crop and 8 x 8 tile means; ~10 s of the box's host threads).  Held to SURVEY 8(d) as it is worded: >= 99 % of the pixels within
    1e-3 (1 + x), relMSE <= 1e-4 (run of record at 1024 spp, profiles/r05_full_size_parity.log: 99.970 %, 3.5e-8)."""
    info = GC.full_frame_every_pixel(renderer, parsed, oracle_scene, "balls_mono", 64, 0.99, 1e-4, 5e-5, metric="c3 full frame 64 spp product build")      # 0.99, 1e-4: SURVEY 8(d), verbatim
    assert info["arithmetic"] == "fast" and info["traversal"] == "flat"


def test_the_one_non_finite_pixel_of_c2_is_a_zero_pdf_knife_edge(renderer, parsed, oracle_scene):
    """BENCH_r03's parity leg: pixel (215, 277) of C2 is inf in the oracle's 512-spp render and finite in the product build's.  Sample 508
    of that pixel draws a cosine-hemisphere variate of exactly 0 at its first vertex (Philox word 0x000000a9 >> 8): pdf = 0, throughput =
    spec / 0 = +inf or NaN by the sign of the rounding residue of n_s . out, which hangs on the last bits of the barycentrics the
    un-normalised vertex normal is interpolated with.  The exact build computes them with the reference's arithmetic and reproduces the
    oracle's inf; the product build's intersector returns them to 1e-6 and may land on either side - the mismatch class
    bench.py accepts (and the only one: oracle/binding.py explain_non_finite).  Rendered here as a one-pixel crop with the sample counter
    set to 507, so that the one sample rendered IS sample 508."""
    from adapt_amd.renderer import Renderer
    from oracle import binding as ob
    i, j, cnt = 215, 277, 508
    words = ob.rng_stream(i * 512 + j, 0, cnt, 4)
    assert int(words[3]) >> 8 == 0                                                  # the draw behind it: jitter x, jitter y, light pick, THEN the cosine variate
    em, arr, objs, cfg = parsed("cbox")
    cfg = dict(cfg); cfg["film"] = {"width": 512, "height": 512, "crop_x": i, "crop_y": j, "crop_rx": 1, "crop_ry": 1}
    rc = make_config(cfg)
    assert rc.do_crop and rc.start_x <= i < rc.end_x and rc.start_y <= j < rc.end_y
    col, ev, nd = oracle_scene("cbox").trace_sample(rc, i, j, cnt)
    assert np.isinf(col).all() and np.isfinite(ev[0, 9:12]).all() and np.isinf(ev[1, 9:12]).all()      # throughput 1 at the first vertex, +inf after its sample
    out = {}
    for exact in (True, False):
        r = Renderer(em, arr, objs, cfg, exact=exact)
        try:
            r.cnt[None] = cnt - 1
            r.render(n_spp=1)
            out[exact] = r.color.to_numpy()[i, j].copy()
            assert r.stats()["n_samples"] == (rc.end_x - rc.start_x) * (rc.end_y - rc.start_y)
        finally:
            r.close()
    assert np.isinf(out[True]).all()                                                 # exact build: the reference's barycentrics, the reference's inf
    assert np.isinf(out[False]).all() or np.isfinite(out[False]).all()              # product build: either side of the knife-edge, never a NaN in the framebuffer
    a = np.zeros((512, 512, 3), np.float32); b = a.copy(); b[i, j] = col; a[i, j] = out[False]
    if not np.isinf(out[False]).all():
        ok, findings = oracle_scene("cbox").explain_non_finite(rc, a, b, cnt)
        assert ok and findings[0]["zero_pdf_vertices"][-1]["sample"] == cnt and findings[0]["zero_pdf_vertices"][-1]["vertex"] == 0, findings


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_flat_records_of_merged_triangle_pairs_answer_as_the_exact_build(seed):
    """The record builder merges coplanar triangle pairs with a convex outline into one record (parallelogram or convex quadrilateral) and
    must leave every other pair alone: random quad soups, product build against the exact build on the same rays."""
    from adapt_amd.renderer import Renderer
    tup = _quad_soup(seed)
    o, d, tmax = _rays(200000, 40 + seed)
    f = Renderer(*tup, width=32, height=32)
    e = Renderer(*tup, width=32, height=32, exact=True)
    try:
        assert f.info()["traversal"] == "flat" and f.info()["arithmetic"] == "fast" and e.info()["arithmetic"] == "exact"
        prim, t, uv = f.intersect(o, d)
        prim_o, t_o, uv_o = e.intersect(o, d)
        assert (prim_o >= 0).mean() > 0.2
        _check_hits(prim, t, uv, prim_o, t_o, uv_o, np.ones(len(prim), bool), d, f.flat.normals)
        assert (f.occluded(o, d, tmax) != e.occluded(o, d, tmax)).sum() <= 3
    finally:
        f.close(); e.close()


def _decal_scene():
    """A floor with a decal lying exactly in its plane (a coplanar group: both quads sit in the flat sweep's tie sections), and in FRONT of
    the pair a ball, a lone triangle and a convex quad - records of the plain sections that run after the tie sections."""
    from adapt_amd import synth
    b = synth._Builder()
    white, red = synth._brdf("lambertian", "#BDBDBD"), synth._brdf("lambertian", "#DD2525")

    def quad(p0, e1, e2):
        p0, e1, e2 = np.float64(p0), np.float64(e1), np.float64(e2)
        return np.float32([[p0, p0 + e1, p0 + e1 + e2], [p0, p0 + e1 + e2, p0 + e2]])
    b.mesh(quad((0.5, 0.0, 0.5), (4.5, 0, 0), (0, 0, 4.5)), white)                       # floor
    b.mesh(quad((1.5, 0.0, 1.5), (2.5, 0, 0), (0, 0, 2.5)), red)                         # decal, same plane
    b.sphere((2.7, 1.0, 2.7), 0.7, white)
    b.mesh(np.float32([[(1.0, 0.6, 1.0), (2.2, 0.6, 1.1), (1.3, 0.6, 2.4)]]), red)      # lone triangle over the decal's corner
    p = np.float64([(3.2, 0.5, 3.1), (4.4, 0.5, 3.3), (4.6, 0.5, 4.5), (3.0, 0.5, 4.0)])  # convex quadrilateral, not a parallelogram
    b.mesh(np.float32([[p[0], p[1], p[2]], [p[0], p[2], p[3]]]), white)
    em = [synth._spot("6.0, 6.0, 6.0", "100.0", (2.7, 5.0, 2.7), (0.0, -1.0, 0.0), 40.0, "s")]
    return b.finish(em, synth._sensor(64, 64, 4, 1))


def test_a_sphere_or_plain_face_in_front_of_a_coplanar_pair_keeps_its_hit():
    """the plain record sections run after the coplanar-group sections and used to leave the pair's runner-up behind; the fix-up
    pass then 'tie-broke' the ball against the decal far behind it and the ray went through the ball."""
    from adapt_amd.renderer import Renderer
    tup = _decal_scene()
    rs = np.random.RandomState(11)
    n = 100000
    o = rs.uniform([0.6, 2.0, 0.6], [4.9, 4.0, 4.9], size=(n, 3)).astype(np.float32)
    tgt = rs.uniform([0.6, 0.0, 0.6], [4.9, 0.0, 4.9], size=(n, 3)).astype(np.float32)
    d = tgt - o; d /= np.linalg.norm(d, axis=1, keepdims=True)
    tmax = rs.uniform(0.5, 6.0, n).astype(np.float32)
    f = Renderer(*tup, width=32, height=32)
    e = Renderer(*tup, width=32, height=32, exact=True)
    try:
        assert f.info()["traversal"] == "flat" and e.info()["arithmetic"] == "exact"
        prim, t, uv = f.intersect(o, d)
        prim_o, t_o, uv_o = e.intersect(o, d)
        is_tri = prim_o != 4                                                            # primitive 4 is the ball
        assert (prim_o == 4).mean() > 0.05 and (prim_o == 5).mean() > 0.01              # the ball (primitive 4) and the lone triangle are in front of the pair often enough
        assert np.array_equal(prim == 4, prim_o == 4)                                     # no ray passes through the ball
        _check_hits(prim, t, uv, prim_o, t_o, uv_o, is_tri, d, f.flat.normals)
        assert (f.occluded(o, d, tmax) != e.occluded(o, d, tmax)).sum() <= 3
        # and through the render pipeline (hot kernel + fix-up lists): same path statistics as the exact build
        f.render(n_spp=8); e.render(n_spp=8)
        sf, se = f.stats(), e.stats()
        for k in ("n_shade", "n_shadow", "n_draws"):
            assert abs(sf[k] - se[k]) <= max(5e-4 * se[k], 20), (k, sf[k], se[k])
    finally:
        f.close(); e.close()


@pytest.mark.parametrize("tag", ["cbox", "balls_mono", "glass_box", "features_a", "features_c"])
def test_flat_sweep_hits_vs_oracle_and_exact_build(tag, renderer, oracle_scene):
    n = 100000
    o, d, tmax = _rays(n, 7)
    r = renderer(tag, width=96, height=96)
    sc = oracle_scene(tag)
    prim, t, uv = r.intersect(o, d)
    obj_o, prim_o, t_o, uv_o, _ = sc.intersect(o, d)
    is_tri = r.flat.obj_info[np.maximum(obj_o, 0), 2] == 0
    _check_hits(prim, t, uv, prim_o, t_o, uv_o, is_tri, d, r.flat.normals)
    occ, occ_o = r.occluded(o, d, tmax), sc.occluded(o, d, tmax)
    assert (occ != occ_o).sum() <= 3, int((occ != occ_o).sum())                      # a blocker within an ulp of the light distance
    # the exact build answers as the oracle does, bit for bit (same rays): the two builds differ by the tolerance above and by nothing else
    e = renderer(tag, width=96, height=96, exact=True)
    pe, te, ue = e.intersect(o, d)
    same = pe == prim_o
    assert np.all(te[~same] == t_o[~same]) and np.array_equal(te[same], t_o[same])


def test_flat_sweep_vs_reference_vectors(renderer):
    """the rays the reference's own intersector answered (fixtures): same primitive, t to 1e-5, occlusion flags"""
    for tag in ("cbox", "balls_mono", "glass_box", "features_a"):
        g = golden(f"scene_{SCENES[tag][2]}.npz")
        r = renderer(tag, width=64, height=64)
        prim, t, uv = r.intersect(g["ray_o"], g["ray_d"])
        h = g["ray_hit"]
        ref_prim = h[:, 1].astype(np.int32)
        same = prim == ref_prim
        assert (~same).sum() <= 1, (tag, int((~same).sum()))
        hit = same & (ref_prim >= 0)
        assert (np.abs(t[hit] - h[hit, 2]) <= 1e-5 * np.maximum(np.abs(h[hit, 2]), 0.3)).all(), tag      # (absolute 3e-6 below t = 0.3: see _check_hits)
        assert (r.occluded(g["ray_o"], g["ray_d"], g["ray_tmax"]) != g["ray_occ"]).sum() <= 1, tag


def test_rays_with_a_zero_direction_component_get_the_reference_answer(renderer, oracle_scene):
    """Upstream's per-object slab cull sees 0 / 0 = NaN for such rays when the origin lies on a box plane and skips objects the primitive
    test would accept: the flat sweep hands them to the reference-order sweep, so they match the oracle exactly."""
    tag = "features_a"
    rs = np.random.RandomState(5)
    n = 4096
    o = rs.uniform([0.1, 0.1, 0.1], [5.4, 5.3, 5.4], size=(n, 3)).astype(np.float32)
    d = rs.normal(size=(n, 3)).astype(np.float32)
    d[np.arange(n), rs.randint(3, size=n)] = 0.0
    d[:64] = np.float32([0.0, 1.0, 0.0]); o[:64, 0] = 0.0                            # mod-Phong's absorbed direction from points on the wall x = 0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    tmax = rs.uniform(0.2, 8.0, n).astype(np.float32)
    r, sc = renderer(tag, width=64, height=64), oracle_scene(tag)
    prim, t, uv = r.intersect(o, d)
    obj_o, prim_o, t_o, uv_o, _ = sc.intersect(o, d)
    assert np.array_equal(prim, prim_o) and np.array_equal(t, t_o)
    assert np.array_equal(r.occluded(o, d, tmax), sc.occluded(o, d, tmax))


# IMAGE_CASES (tests/parity_bounds.py PRODUCT_IMAGE_CASES): tag, width, height, spp, overrides, min fraction of pixels within
# 1e-3 (1 + |x|), max relMSE, with where they are inside SURVEY 8(d) and where they are regression guards, and why
@pytest.mark.parametrize("tag,w,h,spp,ov,min_within,max_rel", IMAGE_CASES)
def test_image_matches_oracle_same_stream(tag, w, h, spp, ov, min_within, max_rel, renderer, parsed, oracle_scene):
    """tests/gpu_cases.py image_vs_oracle_same_stream on the product build: this scene's row, the counters with their absolute floor, and
    the same energy"""
    info = GC.image_vs_oracle_same_stream(renderer, parsed, oracle_scene, tag, w, h, spp, ov, min_within, max_rel, *COUNTER_TOL, host_threads=True,
                                          metric=f"image_case {tag} {w}x{h}x{spp} {ov}", same_energy=True)
    assert info["arithmetic"] == "fast"


@pytest.mark.parametrize("tag", ["cbox", "balls_mono", "glass_box", "features_a", "features_b", "features_c", "textured", "microfacet"])
def test_image_matches_reference_run(tag, renderer):
    """Directly against the fixture recorded from the reference's own kernel (same Philox stream; 2-6 spp on ~1000 pixels: one re-drawn path is 0.1 % of the pixels)"""
    # draws' floor of 400: a re-drawn glass path of features_c is ~80 draws; two or three of them differ in a render this small, in either direction
    assert GC.image_vs_reference_run(renderer, tag, 0.93, 1e-2, 2e-3, draws_floor=400)["arithmetic"] == "fast"


@pytest.mark.parametrize("tag", ["cbox", "balls_mono", "textured", "glass_box", "features_a", "features_b", "features_c", "microfacet"])
def test_statistical_cross_check_other_seed(tag, renderer, parsed, oracle_scene):
    """SURVEY 8(d), as it is worded: "relMSE(HIP, CPU-other-seed) within 1.5x of relMSE(CPU-seedA, CPU-seedB)" - the product build is the same
    ESTIMATOR, not merely the same stream.  Every scene of IMAGE_CASES (round 6: the five feature scenes added - the ones whose same-stream
    per-pixel agreement is below 8(d)'s 99 %, for which this is the check that says the difference is re-drawn paths and not a bias)."""
    hip, cpu, info = GC.other_seed_images(renderer, parsed, oracle_scene, tag)
    GC.other_seed_criterion(tag, hip, cpu, SAME_SEED_FRACTION_OF_NOISE[tag])
    assert info["arithmetic"] == "fast"


@pytest.mark.parametrize("tag,spp", [("textured", 1024), ("features_a", 2048), ("cbox", 2048), ("glass_box", 1024), ("balls_mono", 1024), ("features_b", 1024), ("features_c", 1024), ("microfacet", 1024)])
def test_no_systematic_difference_between_the_builds(tag, spp, renderer):
    """The bias probe of round 3 (tools/gpu_bias_probe.py, profiles/r03_bias_probe.log) as a test: at a sample count where the per-pixel
    chaos of ulp-level hit differences averages out, the product build shades the same number of vertices as the exact build on the same
    stream to 3e-4, carries the same energy to 1e-3, and its image differs from the exact build's by far less than two seeds of the exact
    build differ from each other.  The two scenes that are not below 6e-5, and why (round 5, profiles/r05_bias_cause.log):
      textured   -2.3e-4: rays that RE-HIT THE SURFACE THEY START ON.  A grazing ray's height over its own plane is rounding noise and
                 t = noise / cosine passes the 1e-4 threshold or not by the last bits; the fused height of the flat sweep carries less noise:
                 5-7 % fewer vertices within 2e-3 of the vertex before them than the exact build (-345 of 5 298 at 1 024 spp), each taking
                 the 3-5 vertices of the rest of its path with it (-1 409) - the normal-mapped wall sends many rays along itself.
      features_a +1.6e-4: the ABSORBED branch of its modified-Phong wall (brdf.py:209-229) emits the direction (0, 1, 0) with zero throughput
                 from a point on the wall x = 0; upstream's slab cull then sees 0 / 0 = NaN for every object whose box starts at x = 0 - but
                 only when the hit point's x is EXACTLY 0, which fl(fl(-o.x / d.x) * d.x) + o.x of the reference's solve is about half of the
                 time and the flat sweep's -T.s * rcp(T.d) is not: the product build's copy of that ray goes on to hit the ceiling.  The
                 difference appears at the second vertex and nowhere else (max_bounce 1: identical; 2: +1.2e-4), carries no radiance, and is
                 gone with a Blinn-Phong wall in its place (next test)."""
    w, h = 64, 48
    res = {}
    for key, exact, seed in (("fast", False, 0), ("exact", True, 0), ("exact1", True, 1)):
        r = renderer(tag, width=w, height=h, exact=exact, seed=seed)
        r.render(n_spp=spp)
        img = r.pixels.to_numpy().astype(np.float64)
        img[~np.isfinite(img).all(axis=2)] = 0.0
        res[key] = (img, r.stats())
        r.close()
    (f, sf), (e, se), (e1, _) = res["fast"], res["exact"], res["exact1"]
    # (random numbers: a vertex that is lost takes the draws of the rest of its path with it - the longest paths of `textured` are the ones
    # that graze their own wall - so the draw count moves by up to 1.5x the vertex count's share: measured -3.3e-4 there, with the height
    # T . s rounded like upstream's as well: -3.29e-4, tools/build_variant.sh ufh -DAPT_FLAT_UNFUSED_HEIGHT=1)
    for k, tol in (("n_shade", 3e-4), ("n_shadow", 3e-4), ("n_draws", 5e-4)):
        assert abs(sf[k] - se[k]) <= tol * se[k], (tag, k, sf[k], se[k], (sf[k] - se[k]) / se[k])
    assert abs(f.mean() - e.mean()) <= 1e-3 * e.mean(), (f.mean(), e.mean())

    def rel(a, b):
        return float(np.mean((a - b) ** 2 / (b ** 2 + 1e-2)))
    noise = rel(e, e1)
    assert rel(f, e) <= 0.02 * noise, (rel(f, e), noise)


def test_the_vertex_count_bias_of_features_a_is_its_absorbed_mod_phong_ray(tmp_path):
    """features_a shades +1.6e-4 more vertices in the product build (above).  With the modified-Phong wall made Blinn-Phong - same geometry,
    same lights, no absorbed branch, hence no zero-throughput (0, 1, 0) ray that upstream's NaN slab cull drops or keeps by the last bit of
    a hit point - the two builds agree to 5e-5 (measured: -1e-6 at two bounces, +4e-6 / +1.8e-5 at six)."""
    import os
    from adapt_amd.parsers import scene_parsing
    from adapt_amd.renderer import Renderer
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    xml = open(os.path.join(root, "scenes", "test", "features_a.xml")).read()
    assert '<brdf type="mod-phong" id="right_wall">' in xml
    xml = xml.replace('<brdf type="mod-phong" id="right_wall">', '<brdf type="phong" id="right_wall">').replace("../meshes/", os.path.join(root, "scenes", "meshes") + "/")
    (tmp_path / "fa_phong_wall.xml").write_text(xml)
    tup = scene_parsing(str(tmp_path), "fa_phong_wall.xml")
    n = {}
    for exact in (False, True):
        r = Renderer(*tup, width=64, height=48, exact=exact)
        try:
            r.render(n_spp=1024)
            n[exact] = r.stats()["n_shade"]
        finally:
            r.close()
    assert abs(n[False] - n[True]) <= 5e-5 * n[True], (n, (n[False] - n[True]) / n[True])


def test_determinism_batches_lanes_and_partitions(renderer, parsed, monkeypatch):
    """the product build is bit-reproducible, and its image does not depend on batch size, render lanes or the rank partition"""
    from adapt_amd.tiles import assemble
    for tag, spp in (("cbox", 12), ("balls_mono", 6)):                   # balls_mono: four light samples per vertex (radiance planes: no float atomics)
        a = renderer(tag, width=80, height=48)
        a.render(n_spp=spp)
        img = a.color.to_numpy()
        b = renderer(tag, width=80, height=48, spp_per_batch=5)
        b.render(n_spp=spp)
        assert np.array_equal(img, b.color.to_numpy()), tag
        c = renderer(tag, width=80, height=48)
        c.render(n_spp=spp // 2); c.render(n_spp=spp - spp // 2)
        assert np.array_equal(img, c.color.to_numpy()), tag
        monkeypatch.setenv("APT_LANES", "1")
        one = renderer(tag, width=80, height=48)
        monkeypatch.delenv("APT_LANES")
        one.render(n_spp=spp)
        assert np.array_equal(img, one.color.to_numpy()), tag
        tiles = []
        for rank in range(3):
            t = renderer(tag, width=80, height=48, rank=rank, world_size=3, band_width=4)
            t.render(n_spp=spp)
            tiles.append(t.tile_accum())
        assert np.array_equal(assemble(a.plan.__class__(80, 48, 4, 3), tiles), img), tag


def test_full_size_c2_and_c3_properties(renderer):
    """BASELINE configs[1] / [2] at their full film size through the product build: every sample generated, rays = samples + shaded
    vertices (vanilla_renderer.py:109), shadow rays = S x shaded vertices, finite image, energy in the expected range."""
    for tag, mb, S, lo, hi in (("cbox", 8, 1, 0.05, 1.0), ("balls_mono", 16, 4, 0.05, 2.0)):
        r = renderer(tag, width=512, height=512, max_bounce=mb)
        spp = 16
        r.render(n_spp=spp)
        st = r.stats()
        img = r.pixels.to_numpy()
        assert r.info()["traversal"] == "flat"
        assert st["n_samples"] == 512 * 512 * spp
        assert st["n_shadow"] == S * st["n_shade"] or tag == "balls_mono"          # a vertex on the light itself samples no light when it is the only one
        assert st["n_shadow"] <= S * st["n_shade"] and st["n_shadow_traced"] <= st["n_shadow"] and st["n_lit"] <= st["n_shadow_traced"]
        assert np.isfinite(img).mean() > 0.99999 and lo < float(np.nanmean(img[np.isfinite(img)])) < hi, tag
        r.close()


def test_full_size_c3_crop_matches_oracle(parsed, oracle_scene):
    """C3 (csphere, 512 x 512, 16 bounces, four light samples) on a 128 x 96 window of the full frame against the oracle, same stream"""
    assert GC.c3_crop_vs_oracle(parsed, oracle_scene, spp=32, within=0.93, rel=1e-4, counters=5e-4, host_threads=True)["arithmetic"] == "fast"


def test_volumetric_tracer_through_the_flat_sweep(parsed, oracle_scene):
    """the volumetric tracer's closest-hit queries (k_extend_flat, and the transmittance walk through the one-ray adapter) on the fog box"""
    from adapt_amd.parsers import scene_parsing
    from adapt_amd.renderer import VolumeRenderer
    from adapt_amd.scene_pack import pack_scene
    from oracle import binding as ob
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tup = scene_parsing(os.path.join(root, "scenes", "vpt"), "cbox_fog.xml")
    w, h, spp = 64, 64, 16
    r = VolumeRenderer(*tup, width=w, height=h)
    try:
        assert r.info()["traversal"] == "flat"
        r.render(n_spp=spp)
        rc = make_config(tup[3], width=w, height=h, volumetric=True)
        osc = ob.OracleScene(pack_scene(*tup), rc.cam_t)
        ref, cnt, ost = osc.render(rc, spp, threads=ob.num_threads())
        image_within(r.color.to_numpy(), ref, spp, 0.95, 1e-3)
        counters_within(r.stats(), ost, 1e-3, 0)
    finally:
        r.close()


# ---- product-build twins of the exact module's volumetric and large-scene cases (tests/gpu_cases.py: same bodies, this build's tolerances)
from conftest import VPT_SCENE_TAGS  # noqa: E402


@pytest.mark.parametrize("tag", VPT_SCENE_TAGS)
def test_volumetric_product_build_vs_reference_run_and_oracle(tag):
    """`render.py --type vpt` and `bench.py --config v1..v3` run THIS build: its closest-hit queries go through the flat sweep (hot kernel +
    fix-up lists) where the exact build runs the reference's loop.  All five vpt scenes against the reference-run fixtures and the oracle."""
    from gpu_cases import volumetric_scene_vs_reference_run_and_oracle
    info = volumetric_scene_vs_reference_run_and_oracle(tag, **VPT_PRODUCT_BOUNDS)
    assert info["arithmetic"] == "fast"


@pytest.mark.parametrize("name", ["volgrid_a", "volgrid_b"])
def test_grid_volume_product_build_vs_reference_run_and_oracle(name):
    from gpu_cases import grid_volume_vs_reference_run_and_oracle
    info = grid_volume_vs_reference_run_and_oracle(name, within=0.97, rel=3e-3, draws_tol=4e-3, stat_tol=3e-3)
    assert info["arithmetic"] == "fast"


def test_full_size_c4_crop_product_build_vs_brute_force_oracle():
    """BASELINE configs[3] at full geometry on the build bench.py measures (its BVH walk may differ from the exact build's inside SURVEY
    8(d)'s intersector tolerance: this is the test that holds it to the oracle, not a tie to the exact build on a toy scene)."""
    from gpu_cases import c4_crop_vs_brute_force_oracle
    assert c4_crop_vs_brute_force_oracle(within=0.999, rel=1e-8)["arithmetic"] == "fast"          # (measured: 100 %, 3.9e-12)


@pytest.mark.parametrize("cx,cy", [(640, 360), (330, 250), (930, 200)])
def test_full_size_c5_crop_product_build_vs_brute_force_oracle(cx, cy):
    from gpu_cases import c5_crop_vs_brute_force_oracle
    assert c5_crop_vs_brute_force_oracle(cx, cy, within=0.999, rel=3e-6)["arithmetic"] == "fast"          # (measured, worst of the three windows: 99.967 %, 1.2e-6)


def test_rendering_zero_samples_is_a_no_op(renderer):
    """apt_render(r, 0) divided by zero in the batch split (Renderer.render(n_spp=0) passes 0 straight through).  Surface and
    volumetric path: nothing rendered, counter untouched, and the renderer still works afterwards."""
    from adapt_amd.renderer import VolumeRenderer
    from adapt_amd.parsers import scene_parsing
    import os
    r = renderer("cbox", width=32, height=24)
    r.render(n_spp=0)
    assert r.cnt[None] == 0 and r.stats()["n_samples"] == 0 and not np.any(r.color.to_numpy())
    r.render(n_spp=2); r.render(n_spp=0)
    assert r.cnt[None] == 2 and r.stats()["n_samples"] == 32 * 24 * 2
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    v = VolumeRenderer(*scene_parsing(os.path.join(root, "scenes", "vpt"), "cbox_fog.xml"), width=32, height=24)
    try:
        v.render(n_spp=0)
        assert v.cnt[None] == 0
        v.render(n_spp=1)
        assert v.cnt[None] == 1 and np.isfinite(v.pixels.to_numpy()).all()
    finally:
        v.close()


def test_non_finite_rays_hit_nothing_in_the_tree_walk(monkeypatch):
    """The 64-byte node test reads a child's hit from the SIGN of (exit - entry), and v_max / v_min drop NaN operands: a ray with a NaN or
    infinite component would walk the whole tree.  make_walk_ray turns such rays into rays that enter nothing (traverse.hpp) - as under the
    compare-based test of rounds 2-5, where every `tn <= tf` on NaN slabs was false.  Both builds; finite rays next to them are unaffected."""
    from adapt_amd.renderer import Renderer
    from adapt_amd.synth import three_bunnies
    monkeypatch.setenv("APT_TRAVERSAL", "bvh")
    tup = three_bunnies(1)
    rs = np.random.RandomState(11)
    n = 2048
    o = rs.uniform([0.5, 0.5, 0.5], [5.0, 5.0, 5.0], size=(n, 3)).astype(np.float32)
    d = rs.normal(size=(n, 3)).astype(np.float32); d /= np.linalg.norm(d, axis=1, keepdims=True)
    bad = np.arange(0, n, 7)
    o2, d2 = o.copy(), d.copy()
    d2[bad[0::3], 0] = np.nan; d2[bad[1::3], 1] = np.inf; o2[bad[2::3], 2] = np.nan
    for exact in (False, True):
        r = Renderer(*tup, width=32, height=32, exact=exact)
        try:
            assert r.info()["traversal"] == "bvh"
            p_ref, t_ref, _ = r.intersect(o, d)
            p, t, _ = r.intersect(o2, d2)
            good = np.ones(n, bool); good[bad] = False
            assert (p[bad] == -1).all(), (exact, p[bad][:8])
            assert np.array_equal(p[good], p_ref[good]) and np.array_equal(t[good], t_ref[good]) and (p_ref[good] >= 0).sum() > n // 4
            occ = r.occluded(o2, d2, np.full(n, 3.0, np.float32))
            assert not occ[bad].any()
        finally:
            r.close()


@pytest.mark.parametrize("tag,mode", [("cbox", "tile"), ("balls_mono", "sweep"), ("features_b", "tile"), ("glass_box", "sweep"), ("features_a", "sweep")])
def test_shipped_library_is_bit_checked_where_it_runs_the_reference_arithmetic(tag, mode, renderer, monkeypatch):
    """the bit-exact parity tests run on libadapt_mi_exact.so, the library that ships is libadapt_mi.so.  With APT_TRAVERSAL forced
    to one of the exact build's small-scene intersectors the shipped library executes the exact build's code in every stage - queues, class
    sorting, radiance slots, finalize - and, through round 5, the same shading arithmetic: images and statistics were equal bit for bit.  Since
    round 6 its cos / sin / tan / pow are OCML's float functions and its non-delta shading divides with v_rcp_f32 (adapt_amd/build.py), so what is left
    to assert is that NOTHING ELSE differs: sample counts equal, every other count within 2.5e-3 (a few of ~10^4 paths re-drawn after a last-bit difference in a direction), the image
    within a re-drawn path's reach.  Cornell box, one bounce (Lambertian + point light: no path can take another branch - the light sample's
    1 / d^2 and the direction to the light are its only rounded-differently operations) has the same counts and the same image to 1e-6,
    which pins the rest of the pipeline."""
    w, h, spp = 64, 48, 5
    monkeypatch.setenv("APT_TRAVERSAL", mode)
    e = renderer(tag, width=w, height=h, exact=True)
    f = renderer(tag, width=w, height=h)
    assert f.info()["arithmetic"] == "fast" and f.info()["traversal"] == mode == e.info()["traversal"], (f.info(), e.info())
    e.render(n_spp=spp); f.render(n_spp=spp)
    se, sf = e.stats(), f.stats()
    assert sf["n_samples"] == se["n_samples"]
    for k in ("n_extend", "n_shade", "n_shadow", "n_shadow_traced", "n_lit", "n_draws"):
        assert abs(sf[k] - se[k]) <= max(2.5e-3 * se[k], 8), (k, sf[k], se[k])
    m = image_metrics(f.color.to_numpy() / spp, e.color.to_numpy() / spp)
    record_metric(f"shipped library on the exact build's intersector {tag} {mode}", m)
    assert m["frac_within"] >= 0.95, m
    if tag == "cbox":
        e1 = renderer(tag, width=w, height=h, exact=True, max_bounce=1)
        f1 = renderer(tag, width=w, height=h, max_bounce=1)
        e1.render(n_spp=spp); f1.render(n_spp=spp)
        assert all(e1.stats()[k] == f1.stats()[k] for k in ("n_samples", "n_extend", "n_shade", "n_shadow", "n_shadow_traced", "n_lit", "n_draws"))
        assert np.allclose(f1.color.to_numpy(), e1.color.to_numpy(), rtol=2e-6, atol=0, equal_nan=True)


@pytest.mark.parametrize("which", ["bunnies1", "bunnies2", "balls_mono", "features_c"])
def test_product_walk_hits_within_tolerance_of_the_exact_build(which, parsed, monkeypatch):
    """Scenes beyond the flat sweep walk the same 8-wide tree in both builds, but the product build tests its leaves with the flat sweep's
    precomputed-transform records (traverse.hpp tri_two: one reciprocal instead of the adjugate solve with an IEEE division).  SURVEY 8(d):
    t within 1e-5 relative, same primitive unless tied, on 1e5 random rays per scene; occlusion flags equal up to blockers within an ulp of
    the light distance; spheres (small scenes forced onto the tree) bit-equal, their test is the reference's in both builds."""
    from adapt_amd.renderer import Renderer
    from adapt_amd.synth import three_bunnies
    if which.startswith("bunnies"):
        tup = three_bunnies(levels=int(which[-1]))
    else:
        tup = parsed(which)
        monkeypatch.setenv("APT_TRAVERSAL", "bvh")
    o, d, tmax = _rays(100000, 17)
    f = Renderer(*tup, width=48, height=48)
    e = Renderer(*tup, width=48, height=48, exact=True)
    try:
        assert f.info()["traversal"] == "bvh" == e.info()["traversal"] and f.info()["arithmetic"] == "fast" and e.info()["arithmetic"] == "exact"
        prim, t, uv = f.intersect(o, d)
        prim_o, t_o, uv_o = e.intersect(o, d)
        assert (prim_o >= 0).mean() > 0.5
        is_tri = f.flat.obj_info[np.searchsorted(f.flat.obj_info[:, 0], np.maximum(prim_o, 0), side="right") - 1, 2] == 0
        _check_hits(prim, t, uv, prim_o, t_o, uv_o, is_tri, d, f.flat.normals, tris=f.flat.prims.reshape(-1, 3, 3))
        assert (f.occluded(o, d, tmax) != e.occluded(o, d, tmax)).sum() <= 3
        f.render(n_spp=4); e.render(n_spp=4)
        sf, se = f.stats(), e.stats()
        for k in ("n_shade", "n_shadow", "n_draws"):
            assert abs(sf[k] - se[k]) <= max(1e-3 * se[k], 50), (k, sf[k], se[k])
        m = image_metrics(f.color.to_numpy() / 4, e.color.to_numpy() / 4)
        assert m["frac_within"] >= (0.97 if which.startswith("bunnies") else 0.85) and m["relMSE"] <= 5e-3, m
    finally:
        f.close(); e.close()


@pytest.mark.parametrize("tag,scene", [("c2", "cbox"), ("c3", "balls_mono")])
def test_full_frame_c2_c3_against_the_oracle_statistics(tag, scene, renderer):
    """BASELINE configs[1] / [2] at their FULL film size (512 x 512, all bounces; 64 of the 1024 spp) against the oracle's render of the
    same samples (tests/golden/fullsize_*.npz, tests/golden/gen/gen_fullsize_stats.py): path statistics, the 8 x 8 grid of tile means, and
    the image at 1/8 resolution."""
    info = GC.full_frame_vs_oracle_statistics(renderer, tag, scene, counters=1e-4, tiles=2e-3, within=0.99, rel=1e-5)
    assert info["arithmetic"] == "fast"


def test_two_gpu_rccl_bench_equals_the_single_gpu_image(tmp_path):
    """bench.py exactly as the driver launches it on a multi-GPU node - torch.distributed.run, one rank per GPU, backend "nccl" (= RCCL over
    xGMI), the device-resident all_gather of tiles - with a world of TWO: the gathered image equals the one-GPU image bit for bit (the Philox
    key is the global pixel).  Needs two visible devices: skipped on the one-GPU test boxes, runs wherever the scaling runs do."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    imgs = {}
    for n in (1, 2):
        line, imgs[n] = GC.run_bench(n, ["--scaling", "strong", "--spp", "8"], tmp_path, f"n{n}", rank_args=(), timeout=900)
        assert line["n_gpus"] == n and line["value"] > 0
    assert np.array_equal(imgs[1], imgs[2])


def test_plain_bench_gpus_2_launches_itself(tmp_path):
    """`python bench.py --gpus 2 ...` started WITHOUT torch.distributed.run (as the driver starts N = 1): bench.py becomes its own launcher,
    two ranks render on cuda:0 (--single-device) and gather over gloo; the line says n_gpus == 2, the process group reports a world of two,
    and the gathered image is the one-rank image bit for bit."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    imgs = {}
    for n in (1, 2):
        line, imgs[n] = GC.run_bench(n, ["--scaling", "strong", "--spp", "6"], tmp_path, f"self{n}", torchrun=False, env=env, timeout=900)
        assert line["n_gpus"] == n and line["value"] > 0
        if n > 1:
            pg = line["per_rank"]["collective"]["process_group"]
            assert pg["world_size"] == 2 and pg["backend"] == "gloo" and len(line["per_rank"]["samples"]) == 2
    assert np.array_equal(imgs[1], imgs[2])


def test_bench_dump_outputs_are_the_timed_steps_and_do_not_depend_on_warmup(tmp_path):
    """`bench.py --dump-outputs DIR`: the timed renderer's image, accumulation and event counts after exactly `--steps` timed steps, all
    finite (non-finite components marked in nonfinite.npy); two runs that differ only in `--warmup` write the same arrays bit for bit, and the result line carries `steps` and `ms_per_step`."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {}
    for warmup in (0, 2):
        d = tmp_path / f"w{warmup}"
        cmd = [sys.executable, "bench.py", "--gpus", "1", "--config", "c1", "--steps", "3", "--warmup", str(warmup), "--spp", "2",
               "--no-cpu-baseline", "--no-profile", "--dump-outputs", str(d)]
        res = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr[-2000:]
        line = json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][-1])
        assert line["steps"] == 3 and line["ms_per_step"] > 0
        out[warmup] = {k: np.load(d / f"{k}.npy") for k in ("image", "accum", "counters", "nonfinite")}
    a = out[0]
    assert all(np.isfinite(v).all() for v in a.values())
    assert a["image"].dtype == a["accum"].dtype == a["nonfinite"].dtype == np.float32
    assert a["image"].shape == a["accum"].shape == a["nonfinite"].shape == (256, 256, 3)
    assert a["counters"].dtype == np.float64 and a["counters"][0] == 256 * 256 * 2 * 3           # n_samples: the three timed steps only
    fin = a["nonfinite"] == 0
    assert fin.mean() > 0.99 and np.allclose(a["image"][fin], a["accum"][fin] / np.float32(6), rtol=1e-6, atol=0)
    for k in ("image", "accum", "counters", "nonfinite"):
        assert np.array_equal(a[k], out[2][k]), k


def test_nine_material_classes_on_the_tree_lose_no_hits(monkeypatch):
    """with all nine surface-model classes in one scene (the microfacet switch on) there are more classes than class
    queues, the scene renders unsorted through the all-models kernel - and the leaf-slot word of the product build's tree must not carry
    a class id at all: id 8 in bits 28.. set the sign bit, which the walk's hand-in reads as "nothing hit", so every closest hit on the
    ninth class's object was lost.  Nine small bunnies, one per class, in the Cornell room; product build against the exact build."""
    import adapt_amd.materials as mats
    from adapt_amd import synth
    from adapt_amd.renderer import Renderer
    monkeypatch.setattr(mats, "ENABLE_MICROFACET", True)
    b = synth._Builder()
    white = synth._brdf("lambertian", "#BDBDBD")
    synth._room(b, white, synth._brdf("lambertian", "#DD2525"), synth._brdf("lambertian", "#25DD25"))
    m = synth._mat
    nine = [synth._brdf("lambertian", "#FFFFFF"), synth._brdf("phong", "#BCBCBC", "8.0", "#303030"), synth._brdf("specular", "#DEDEDE"),
            synth._brdf("mod-phong", "#BCBCBC", "10.0", "#424242"),
            m('<brdf type="fresnel-blend" id="fb"><rgb name="k_d" value="#CACACA"/><rgb name="k_s" value="#333333"/><rgb name="k_g" r="10" g="1000"/></brdf>'),
            m('<brdf type="oren-nayar" id="on"><rgb name="k_d" value="#C8B496"/><rgb name="sigma" value="20.0"/></brdf>'),
            m('<brdf type="thin-coat" id="tc"><rgb name="k_d" value="#9696C8"/><rgb name="k_s" value="0.9"/><rgb name="sigma" r="20" g="20" b="1.5"/></brdf>'),
            m('<bsdf type="lambertian" id="lt"><rgb name="k_d" value="#E0E0E0"/><medium type="transparent"><float name="ior" value="1.4"/></medium></bsdf>'),
            m('<brdf type="microfacet" id="mf"><rgb name="k_d" value="#E0C8A0"/><rgb name="roughness" value="0.2"/><rgb name="ref_ior" r="1.0" g="1.5" b="0.0"/></brdf>')]
    bunny = synth._bunny(1)
    for k, mat in enumerate(nine):
        b.mesh(synth._place(bunny, 0.3, (0.95 + 1.8 * (k % 3), 0.0, 0.9 + 1.75 * (k // 3))), mat)
    point = synth.SOURCE_MAP["point"](synth.xet.fromstring('<emitter type="point" id="p"><rgb name="emission" value="30.0, 30.0, 30.0"/><point name="center" x="2.78" y="5.0" z="2.8"/></emitter>'))
    tup = b.finish([point], synth._sensor(96, 72, 6, 1))
    f = Renderer(*tup, width=96, height=72)
    e = Renderer(*tup, width=96, height=72, exact=True)
    try:
        assert f.info()["traversal"] == "bvh" == e.info()["traversal"] and f.info()["arithmetic"] == "fast"
        assert "all models" in f.info()["shade_variant"], f.info()["shade_variant"]            # nine classes: unsorted
        o, d, _ = _rays(60000, 23)
        prim, t, _ = f.intersect(o, d)
        prim_o, t_o, _ = e.intersect(o, d)
        assert (prim == prim_o).mean() >= 0.999 and np.array_equal(prim >= 0, prim_o >= 0)
        first = f.flat.obj_info[:, 0]
        obj = np.searchsorted(first, np.maximum(prim, 0), side="right") - 1
        for k in range(5, 14):                                                                # every bunny is hit by some of the rays
            assert ((obj == k) & (prim >= 0)).sum() > 50, k
        f.render(n_spp=4); e.render(n_spp=4)
        sf, se = f.stats(), e.stats()
        for key in ("n_extend", "n_shade", "n_shadow", "n_draws"):
            assert abs(sf[key] - se[key]) <= max(2e-3 * se[key], 50), (key, sf[key], se[key])
    finally:
        f.close(); e.close()


@pytest.mark.parametrize("tag", ["vpt_cbox", "media_a"])
def test_flat_transmittance_walk_against_the_tiled_walk(tag, monkeypatch):
    """k_vshadow_flat (two light samples per lane on the flat sweep) against the walk it replaces in
    the product build (APT_VSHADOW_FLAT=0: k_vshadow<tile / sweep>, the reference's arithmetic) on the same stream:
    the same samples are followed (n_shadow_traced equal), segments walked and samples that arrive agree to 1e-3 (a hit within an ulp of
    the light or of a null surface may fall on the other side), the images to the product build's per-pixel tolerance."""
    from conftest import scene_from_golden
    from adapt_amd.renderer import VolumeRenderer
    tup, g = scene_from_golden(tag, "vptscene")
    w, h = int(g["width"]), int(g["height"])
    out = {}
    for flat in ("1", "0"):
        monkeypatch.setenv("APT_VSHADOW_FLAT", flat)
        r = VolumeRenderer(*tup, width=w, height=h)
        try:
            assert r.info()["arithmetic"] == "fast"
            r.render(n_spp=24)
            out[flat] = (r.color.to_numpy() / 24, r.stats())
        finally:
            r.close()
    a, b = out["1"], out["0"]
    assert a[1]["n_shadow_traced"] == b[1]["n_shadow_traced"] and a[1]["n_shade"] == b[1]["n_shade"] and a[1]["n_draws"] == b[1]["n_draws"]
    for k in ("n_track", "n_lit"):
        assert abs(a[1][k] - b[1][k]) <= max(1e-3 * b[1][k], 20), (k, a[1][k], b[1][k])
    m = image_metrics(a[0], b[0])
    assert m["frac_within"] >= 0.99 and m["relMSE"] <= 1e-4, m


def test_cli_end_to_end_writes_a_jpeg_and_resumes_from_its_checkpoint(tmp_path, capsys):
    """render.py's flow through adapt_amd.cli.main on the GPU: AdaPT's flags (--no_gui renders iter_num + 1 samples, render.py:80-81), the
    output name `<img_name>-<scene file>-<type>.<ext>`, --img_ext jpg (parsers/opts.py:25), and a --save_iter checkpoint that a second run
    loads (render.py:96-100,119-121): the counter continues where the first run saved."""
    import os
    from adapt_amd.cli import main
    pil = pytest.importorskip("PIL.Image")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--input_path", os.path.join(root, "scenes"), "--scene", "cbox", "--name", "c2_cbox.xml", "--type", "pt", "--no_gui",
              "--output_path", str(tmp_path / "out"), "--chkpt_path", str(tmp_path / "chk"), "--img_name", "t", "--img_ext", "jpg", "--width", "64", "--height", "48"]
    assert main(common + ["--iter_num", "7", "--save_iter", "4"]) == 0
    out = tmp_path / "out" / "t-c2_cbox-pt.jpg"
    with pil.open(out) as im:
        assert im.format == "JPEG" and im.size == (64, 48)
        a = np.asarray(im.convert("RGB"), np.float32)
    assert a.mean() > 5.0                                            # a lit Cornell box, not a black frame
    assert (tmp_path / "chk" / "t-c2_cbox-pt.pkl").exists()
    text = capsys.readouterr().out
    assert "8 samples" in text                                       # iter_num + 1
    assert main(common + ["--iter_num", "3", "--load"]) == 0
    text = capsys.readouterr().out
    assert "recovered from check-point, elapsed counter: 4" in text  # saved before iteration 4 (the last multiple of save_iter below 8)
