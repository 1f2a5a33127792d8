"""The flat sweep (traverse.hpp "Flat sweep", the path of the headline configs) at its capacity, on the device.  The bundled scenes stop at
36 primitives and 9 record pairs; the scenes of tests/flat_cases.py fill the stream - 96 primitives, 41 and 48 pairs, every section with
an odd tail, pairs across the plain / coplanar-group border, a record of all-zero rows - so that the strip words of the three culls
carry bits at 32 and above, the shading records fill their LDS array and the hit primitive its 8 bits.  Held here:
  * closest hits and occlusion of the product build against the oracle's brute force and the exact build (test_gpu_fast._check_hits), on
    4099 rays (an odd tail for the two-rays-per-lane kernels), 129 and 1;
  * every A/B switch of the flat path, on and off, to the same render bit for bit (gpu_ab.assert_same_run), and the light-strip rows at
    16 and 17 emitters;
  * every ray through the fix-up lists against the reference-order sweep of the same build;
  * the image against the oracle on the same Philox stream, both builds, all four variants (tests/parity_bounds.py);
  * the step from 96 to 97 primitives, where the renderer leaves the flat sweep for the tree.
The CPU side of the same scenes: tests/test_flat_records.py, test_camera_cull.py, test_shadow_cull.py, test_light_strips.py."""
import numpy as np
import pytest

from conftest import record_metric
from flat_cases import CAPACITY_SCENES, VARIANTS, capacity, many_lights, over_by_one
from gpu_ab import TRACED, assert_same_run, open_renderer, run_of
from gpu_cases import counters_within, image_within
from parity_bounds import COUNTER_TOL, EXACT, VPT_PRODUCT_BOUNDS, capacity_product_row
from test_camera_cull import FLAT_MAX_PRIMS
from test_gpu_fast import _check_hits, _rays
from adapt_amd.scene_pack import make_config, pack_scene

pytestmark = pytest.mark.gpu

FILM = (48, 40, 8)                      # width, height, samples per pixel of the renders here
LEAN = "lambertian/point"


def _oracle(fs, tup):
    from oracle import binding as ob
    return ob.OracleScene(fs, make_config(tup[3]).cam_t)


# ---------------------------------------------------------------- hits
@pytest.mark.parametrize("n", [4099, 129, 1])
@pytest.mark.parametrize("name", list(CAPACITY_SCENES))
def test_capacity_hits_vs_oracle_and_exact_build(name, n):
    tup, fs = capacity(name)
    o, d, tmax = _rays(n, 7)
    sc = _oracle(fs, tup)
    obj_o, prim_o, t_o, uv_o, _ = sc.intersect(o, d)
    occ_o = sc.occluded(o, d, tmax)
    is_tri = fs.obj_info[np.maximum(obj_o, 0), 2] == 0
    with open_renderer(tup, 32, 32) as f, open_renderer(tup, 32, 32, exact=True) as e:
        assert f.info()["traversal"] == "flat" and f.info()["arithmetic"] == "fast" and e.info()["arithmetic"] == "exact"
        assert f.flat.prims.shape[0] == FLAT_MAX_PRIMS
        prim, t, uv = f.intersect(o, d)
        occ = f.occluded(o, d, tmax)
        pe, te, ue = e.intersect(o, d)
        occ_e = e.occluded(o, d, tmax)
    assert is_tri.any() and (prim_o >= 0).all()                                     # a closed room
    _check_hits(prim, t, uv, prim_o, t_o, uv_o, is_tri, d, fs.normals)
    _check_hits(prim, t, uv, pe, te, ue, is_tri, d, fs.normals)
    assert (occ != occ_o).sum() <= 3 and (occ != occ_e).sum() <= 3, (int((occ != occ_o).sum()), int((occ != occ_e).sum()))
    # the exact build answers as the oracle does, bit for bit: the two builds differ by _check_hits' tolerance and by nothing else
    same = pe == prim_o
    assert np.all(te[~same] == t_o[~same]) and np.array_equal(te[same], t_o[same]) and np.array_equal(occ_e, occ_o)
    if n == 4099: assert np.unique(prim_o).size >= 85                               # the rays reach the whole stream


# ---------------------------------------------------------------- A/B switches
SWITCHES = ("APT_CAMERA_CULL", "APT_SHADOW_CULL", "APT_LIGHT_STRIPS", "APT_CAMERA_FUSE", "APT_RECORD_STAGE", "APT_LIVE_ROWS")
# scene, variant, unsorted.  `delta` has two material classes (Lambertian, delta) and so takes the class-sorted pipeline by default; unsorted
# (gpu_ab.open_renderer: APT_SORTED=0, one light sample per vertex) it takes the non-lean traced kernels, as `sorted` then does too
AB_CASES = [(name, variant, unsorted) for name in CAPACITY_SCENES for variant, unsorted in (("lean", False), ("delta", False), ("delta", True), ("sorted", True))]


def _ab_run(tup, env, **kw):
    """-> Run, the forms the renderer reports"""
    w, h, spp = FILM
    with open_renderer(tup, w, h, env=env, **kw) as r:
        assert r.info()["traversal"] == "flat" and r.info()["arithmetic"] == "fast"
        return run_of(r, spp), {"APT_CAMERA_FUSE": r.camera_fused(), "APT_LIGHT_STRIPS": r.light_strips(), "APT_RECORD_STAGE": r.record_staged(), "APT_LIVE_ROWS": r.live_rows()}


@pytest.mark.parametrize("name,variant,unsorted", AB_CASES)
def test_every_switch_of_the_flat_path_leaves_a_capacity_render_bit_identical(name, variant, unsorted):
    tup, _ = capacity(name, variant)
    on, forms = _ab_run(tup, {}, unsorted=unsorted)
    traced, lean = variant == "lean" or unsorted, variant == "lean"
    assert on.traced == traced and (LEAN in on.variant) == lean, on.variant
    # the camera-fed launch and its masks go with the traced kernels, the staged record and the live rows with the lean ones
    assert forms == {"APT_CAMERA_FUSE": traced, "APT_LIGHT_STRIPS": traced, "APT_RECORD_STAGE": lean, "APT_LIVE_ROWS": lean}, forms
    assert on.fused == traced and on.stats["n_samples"] == FILM[0] * FILM[1] * FILM[2]
    assert 0 < on.stats["n_lit"] < on.stats["n_shadow"]                             # samples reach the light, and some are blocked
    for sw in SWITCHES:
        off, forms_off = _ab_run(tup, {sw: "0"}, unsorted=unsorted)
        if sw in forms_off: assert forms_off[sw] is False, (sw, forms_off)
        if sw in ("APT_CAMERA_FUSE", "APT_SHADOW_CULL"): assert forms_off["APT_LIGHT_STRIPS"] is False      # the masks belong to the camera-fed launch and cover the occluder lists
        assert_same_run(on, off, f"{name} {variant} {sw}=0")


@pytest.mark.parametrize("n,masks", [(16, True), (17, False)])
def test_light_strip_rows_end_at_sixteen_emitters(n, masks):
    tup = many_lights(n)
    on, forms = _ab_run(tup, {})
    off, forms_off = _ab_run(tup, {"APT_LIGHT_STRIPS": "0"})
    assert LEAN in on.variant and on.traced and on.fused
    assert forms["APT_LIGHT_STRIPS"] is masks and forms_off["APT_LIGHT_STRIPS"] is False, (n, forms, forms_off)
    assert_same_run(on, off, f"{n} lights")


# ---------------------------------------------------------------- every ray through the fix-up lists
@pytest.mark.parametrize("variant", ["lean", "delta", "sorted"])
def test_capacity_fix_up_lists_match_the_reference_order_sweep_of_the_same_build(variant):
    """tests/test_gpu_fast.py test_fix_up_lists_match_the_reference_order_sweep_of_the_same_build, its criteria, on capacity_mixed"""
    tup, _ = capacity("capacity_mixed", variant)
    w, h, spp = FILM
    with open_renderer(tup, 8, 8, exact=True) as e:
        mode = e.info()["traversal"]
    assert mode in ("sweep", "tile")
    with open_renderer(tup, w, h, env={"APT_TRAVERSAL": mode}) as s:
        assert s.info()["traversal"] == mode and s.info()["arithmetic"] == "fast"
        s.render(n_spp=spp); ref = s.color.to_numpy(); sst = s.stats()
    with open_renderer(tup, w, h, env={"APT_FLAT_DEFER_ALL": "1"}) as f:
        assert f.info()["traversal"] == "flat" and f.info()["arithmetic"] == "fast"
        f.render(n_spp=spp); img = f.color.to_numpy(); st = f.stats(); n_shadow_ray = f.num_shadow_ray
    same = (img == ref) | (np.isnan(img) & np.isnan(ref))
    rel = np.abs(img.astype(np.float64) - ref) / np.maximum(np.abs(ref.astype(np.float64)), np.finfo(np.float32).tiny)
    record_metric(f"capacity fix-up lists vs reference-order sweep, product build {variant}",
                  {"mode": mode, "bit_equal_frac": float(same.mean()), "max_rel": float(np.where(same, 0.0, rel).max())})
    for k in ("n_samples", "n_extend", "n_shade", "n_shadow", "n_shadow_traced", "n_lit", "n_draws"):
        assert st[k] == sst[k], (k, st[k], sst[k])
    assert n_shadow_ray == (4 if variant == "sorted" else 1)
    if n_shadow_ray == 1:
        assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))
    assert np.all(same | (rel <= 4 * 2.0 ** -23))


# ---------------------------------------------------------------- the image against the oracle, same stream
_oracle_renders = {}


def _oracle_render(key, tup, fs, volumetric):
    """the oracle's accumulation and counters at FILM, computed once per scene and shared by the two builds (read-only)"""
    if key not in _oracle_renders:
        from oracle import binding as ob
        w, h, spp = FILM
        rc = make_config(tup[3], width=w, height=h, volumetric=volumetric)
        ref, _, ost = ob.OracleScene(fs, rc.cam_t).render(rc, spp, threads=ob.num_threads())
        ref.setflags(write=False)
        _oracle_renders[key] = (ref, ost)
    return _oracle_renders[key]


def _image_vs_oracle(key, tup, fs, build, volumetric, within, rel, counters, floor, env=None):
    w, h, spp = FILM
    ref, ost = _oracle_render(key, tup, fs, volumetric)
    with open_renderer(tup, w, h, exact=(build == "exact"), volumetric=volumetric, env=env) as r:
        info = r.info()
        r.render(n_spp=spp)
        acc, st = r.color.to_numpy(), r.stats()
    assert info["arithmetic"] == build, info
    report = lambda m, a, b, fin: record_metric(f"capacity image {key} {w}x{h}x{spp} {build} build {env or ''}", dict(
        m, traversal=info["traversal"], variant=info["shade_variant"], **{k: st[k] for k in ("n_shade", "n_shadow", "n_draws")}, **{k + "_oracle": ost[k] for k in ("n_shade", "n_shadow", "n_draws")}))
    image_within(acc, ref, spp, within, rel, label=(key, build), report=report)
    assert st["n_samples"] == ost["n_samples"] == w * h * spp, (key, st["n_samples"], ost["n_samples"])
    counters_within(st, ost, counters, floor, label=(key, build))
    return info


def _bounds(build, variant, name="capacity_mixed"):
    """-> within, relMSE, counters (relative, floor): the exact build's statement, or the row the variant borrows (tests/parity_bounds.py)"""
    if build == "exact": return EXACT.within, EXACT.rel, EXACT.counters, 0
    if variant == "volumetric": return VPT_PRODUCT_BOUNDS["within"], VPT_PRODUCT_BOUNDS["rel"], VPT_PRODUCT_BOUNDS["stat_tol"], 0
    return (*capacity_product_row(name, variant), *COUNTER_TOL)


@pytest.mark.parametrize("build", ["exact", "fast"])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(CAPACITY_SCENES))
def test_capacity_image_matches_oracle_same_stream(name, variant, build):
    tup, fs = capacity(name, variant)
    info = _image_vs_oracle(f"{name} {variant}", tup, fs, build, variant == "volumetric", *_bounds(build, variant, name))
    if build == "fast":
        assert info["traversal"] == "flat", info
        assert (TRACED in info["shade_variant"]) == (variant == "lean"), info           # (`delta` and `sorted`: class-sorted; below, `delta` traced)
        if variant == "volumetric": assert info["shade_variant"].startswith("volumetric"), info
        if variant == "lean": assert LEAN in info["shade_variant"], info


@pytest.mark.parametrize("name", list(CAPACITY_SCENES))
def test_capacity_image_of_the_non_lean_traced_kernels_matches_oracle_same_stream(name):
    """`delta` unsorted (APT_SORTED=0; it has one light sample per vertex): the traced kernels of a variant with mirrors and glass, held to
    the same row and the same oracle render as the class-sorted pipeline above"""
    tup, fs = capacity(name, "delta")
    info = _image_vs_oracle(f"{name} delta", tup, fs, "fast", False, *_bounds("fast", "delta", name), env={"APT_SORTED": "0"})
    assert info["traversal"] == "flat" and TRACED in info["shade_variant"] and LEAN not in info["shade_variant"], info


# ---------------------------------------------------------------- 96 / 97 primitives
def test_one_primitive_more_leaves_the_flat_sweep_for_the_tree():
    """api.hip pack_flat builds no flat records beyond APT_FLAT_MAX_PRIMS primitives, and pick_traversal honours APT_TRAVERSAL only for a
    mode the scene can be traced with: forcing `flat` on 97 primitives falls back to the tree, silently - the same render.
    (`lean` has one material per coplanar overlap: between two faces at the same distance the product build's tree leaves let the first
    one tested win, where the flat sweep reproduces the reference's choice - with two colours the tree's image measured 2.2 % of its
    pixels off the oracle's, profiles/NOTES.md; which face was hit is still compared, by _check_hits' "same primitive unless tied".)"""
    tup, fs = capacity("capacity_mixed")
    more = over_by_one(tup)
    fs_more = pack_scene(*more)
    assert fs.prims.shape[0] == FLAT_MAX_PRIMS and fs_more.prims.shape[0] == FLAT_MAX_PRIMS + 1
    o, d, tmax = _rays(4099, 7)
    w, h, spp = FILM
    with open_renderer(tup, w, h) as f, open_renderer(more, w, h) as b:
        assert f.info()["traversal"] == "flat" and b.info()["traversal"] == "bvh" and b.info()["arithmetic"] == "fast"
        prim, t, uv = f.intersect(o, d)
        prim_b, t_b, uv_b = b.intersect(o, d)
        occ, occ_b = f.occluded(o, d, tmax), b.occluded(o, d, tmax)
        plain = run_of(b, spp)
    assert (prim_b < FLAT_MAX_PRIMS).all()                                          # nothing reaches the triangle behind the back wall
    is_tri = ~np.isin(prim_b, np.flatnonzero(np.repeat(fs.obj_info[:, 2], fs.obj_info[:, 1])))
    _check_hits(prim, t, uv, prim_b, t_b, uv_b, is_tri, d, fs.normals)
    assert (occ != occ_b).sum() <= 3, int((occ != occ_b).sum())
    with open_renderer(more, w, h, env={"APT_TRAVERSAL": "flat"}) as forced:
        assert forced.info()["traversal"] == "bvh"
        assert_same_run(plain, run_of(forced, spp), "APT_TRAVERSAL=flat on 97 primitives")
    # both sides of the step meet the bound of the 96-primitive scene (the oracle sweeps 96 and 97 primitives by brute force)
    _image_vs_oracle("capacity_mixed lean", tup, fs, "fast", False, *_bounds("fast", "lean"))
    info = _image_vs_oracle("capacity_mixed lean + 1", more, fs_more, "fast", False, *_bounds("fast", "lean"))
    assert info["traversal"] == "bvh"
