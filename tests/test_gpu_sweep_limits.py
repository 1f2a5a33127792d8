"""The reference-order sweeps of csrc/traverse.hpp - `sweep_wg` (wave sweep), `sweep_tile` (tiled sweep) and the plain `sweep` the tile's
redo falls back on - at their list, LDS and key limits, on the device, against the oracle's brute-force intersector, which the exact
build must match bit for bit.  The scenes and ray batches are those of tests/sweep_cases.py; tests/test_sweep_cases_host.py shows on the
CPU that they reach the edges.  Which test sits on which limit:

  sweep_wg, BLOCK = 256
    APT_SWEEP_LIST_MIN = 6 (fans of 5, 6 and 7 next to each other)       test_explicit_rays[tile_34-sweep], [tile_35-sweep]
    APT_SWEEP_MAX_LISTS = 128 (142 listed objects, 15 % of the rays
      end past list 128; unlisted objects before and after it)           test_explicit_rays[lists_130-sweep], the lists_130 render and aov
    a list as long as the block, 64-ray chunks, empty lists              the `aimed(...)`, `away` and `random[:n]` batches of every scene
    sweep_wg<true> (k_shadow<TRACE_SWEEP> only)                          test_surface_render_matches_the_oracle[tile_35], [lists_130]
  sweep_tile, APT_TILE_NT = 512
    160 KiB of LDS: 34 objects fit, 35 do not; the launch attribute      test_the_mode_steps, every tile_34 test under `tile`
    phase B's chunk walk over full lists                                 the `aimed(...)` batches under `tile` (512-entry lists)
    primitive indices with bit 15 set in the reduction key               test_explicit_rays[keys_16-tile]
    forced modes up to 65 535 primitives                                 test_explicit_rays[keys_16-sweep], [keys_16-tile]
    the redo rule (near ties at the running minimum)                     test_explicit_rays[ties-tile], the ties renders
  APT_VSHADOW_NT = 256: k_vshadow<TRACE_TILE>, <TRACE_SWEEP>             test_volumetric_walk_through_the_tile_and_the_wave_sweep
    ... in the product build (APT_VSHADOW_FLAT=0)                        test_product_build_walks_through_the_tile_when_its_flat_walk_is_off
  k_aov_trace<TRACE_TILE> at 34 objects, <TRACE_SWEEP> past list 128     test_feature_buffers_through_the_sweeps
"""
import time

import numpy as np
import pytest

import aov_cases as ac
import null_stack_cases as ns
import sweep_cases as sc
from conftest import record_metric
from gpu_ab import assert_same_run, open_renderer, run_of
from gpu_cases import counters_within, image_within
from parity_bounds import EXACT, VPT_PRODUCT_BOUNDS
from test_gpu_fast import _check_hits
from adapt_amd.scene_pack import make_config

pytestmark = pytest.mark.gpu

FILM = (48, 40, 8)                      # width, height, samples per pixel of the renders here
BUILDS = ("exact", "fast")


@pytest.fixture(autouse=True, scope="module")
def _wall_time():
    t0 = time.time()
    yield
    record_metric("sweep limits: wall time of tests/test_gpu_sweep_limits.py", {"seconds": round(time.time() - t0, 1)})


def _open(name, build, mode, w=32, h=32, **kw):
    """a renderer of scene `name` in `build` with APT_TRAVERSAL=`mode` (None: nothing forced)"""
    scene_kw = kw.pop("scene_kw", {})
    return open_renderer(sc.scene(name, **scene_kw)[0], w, h, exact=(build == "exact"), env={"APT_TRAVERSAL": mode} if mode else {}, **kw)


def _is(r, build, mode):
    info = r.info()
    assert info["traversal"] == mode and info["arithmetic"] == build, (info, build, mode)


# ---------------------------------------------------------------- the mode steps
def test_the_mode_steps():
    """api.hip pick_traversal: 34 objects are the last that get a tile (159 896 B of the CU's 163 840 B of LDS, asked for through
    hipFuncSetAttribute), 35 take the wave sweep, also when the tile is asked for; more than 96 primitives walk the tree unless a sweep
    is asked for, and a scene of more than 34 objects is never given the tile"""
    assert sc.DEFAULT_MODE["tile_34"] == "tile" and sc.DEFAULT_MODE["tile_35"] == "sweep" and sc.DEFAULT_MODE["lists_130"] == "bvh"
    for name, mode in sc.DEFAULT_MODE.items():
        with _open(name, "exact", None) as r: _is(r, "exact", mode)
    for build in BUILDS:
        with _open("tile_35", build, "tile") as r: _is(r, build, "sweep" if build == "exact" else "flat")      # (the product build: back to its own default)
        with _open("tile_35", build, "sweep") as r: _is(r, build, "sweep")
        with _open("lists_130", build, "sweep") as r: _is(r, build, "sweep")
        with _open("lists_130", build, "tile") as r: _is(r, build, "bvh")
        with _open("lists_130", build, None) as r: _is(r, build, "bvh")
        for name in ("tile_34", "keys_16", "ties"):
            for mode in ("sweep", "tile"):
                with _open(name, build, mode) as r: _is(r, build, mode)


# ---------------------------------------------------------------- explicit rays
def _answers(r, name):
    """-> {batch: (prim, t, uv, occluded)} of renderer r for every batch of the scene"""
    out = {}
    for batch, (o, d, tmax) in sc.batches(name).items():
        prim, t, uv = r.intersect(o, d)
        out[batch] = (prim, t, uv, r.occluded(o, d, tmax))
    return out


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("name,mode", [(name, mode) for name, modes in sc.MODES.items() for mode in modes])
def test_explicit_rays(name, mode):
    """apt_intersect goes through k_extend<MODE, 0> (sweep_wg<false>, sweep_tile<false, 512>), apt_occluded through sweep_any and
    sweep_tile<true, 512>.  Exact build: primitive, distance, the barycentrics of triangle hits and the occlusion flags are the
    oracle's, bit for bit, in every batch.  Product build: held to the oracle by test_gpu_fast._check_hits; a batch in which no ray ends
    on a triangle (a prefix of one degenerate ray) has nothing for that criterion to average and is held to the oracle's bits instead."""
    _, fs = sc.scene(name)
    tris = fs.prims.reshape(-1, 3, 3) if name in ("keys_16", "lists_130") else None          # small triangles: _check_hits' statement about the point
    with _open(name, "exact", mode) as e:
        _is(e, "exact", mode)
        exact = _answers(e, name)
    with _open(name, "fast", mode) as f:
        _is(f, "fast", mode)
        fast = _answers(f, name)
    equal_rays = total = 0
    for batch, (o, d, tmax) in sc.batches(name).items():
        obj_o, prim_o, t_o, uv_o, occ_o = sc.oracle_hits(name, batch)
        is_tri = (prim_o >= 0) & (fs.obj_info[np.maximum(obj_o, 0), 2] == 0)
        prim, t, uv, occ = exact[batch]
        ok = (prim == prim_o) & (t.view(np.uint32) == t_o.view(np.uint32))
        equal_rays += int(ok.sum()); total += len(ok)
        assert np.array_equal(prim, prim_o), (name, mode, batch, int((prim != prim_o).sum()), np.flatnonzero(prim != prim_o)[:8])
        assert np.array_equal(t, t_o), (name, mode, batch, int((t != t_o).sum()))
        assert np.array_equal(uv[is_tri], uv_o[is_tri]), (name, mode, batch)
        assert np.array_equal(occ, occ_o), (name, mode, batch, int((occ != occ_o).sum()))
        prim, t, uv, occ = fast[batch]
        if is_tri.any():
            _check_hits(prim, t, uv, prim_o, t_o, uv_o, is_tri, d, fs.normals, tris=tris)
        else:
            assert np.array_equal(prim, prim_o) and np.array_equal(t, t_o), (name, mode, batch)
        assert (occ != occ_o).sum() <= 3, (name, mode, batch, int((occ != occ_o).sum()))
    record_metric(f"sweep limits: explicit rays {name} {mode}, exact build vs oracle", {"rays": total, "bit_equal_frac": equal_rays / total, "batches": len(exact)})
    # a prefix is a partial block of the same rays: the same answers
    for n in sc.PREFIXES:
        for got in (exact, fast):
            assert all(_same_bits(a, b[:n]) for a, b in zip(got[f"random[:{n}]"], got["random"])), (name, mode, n)


@pytest.mark.parametrize("name", [name for name, modes in sc.MODES.items() if len(modes) == 2])
def test_the_wave_sweep_and_the_tile_agree_bit_for_bit_in_the_product_build(name):
    """forced `sweep` against forced `tile`: the same arithmetic on another schedule - primitive, distance, barycentrics, flags"""
    with _open(name, "fast", "sweep") as s, _open(name, "fast", "tile") as t:
        _is(s, "fast", "sweep"); _is(t, "fast", "tile")
        a, b = _answers(s, name), _answers(t, name)
    _, fs = sc.scene(name)
    sphere_prim = np.repeat(fs.obj_info[:, 2] != 0, fs.obj_info[:, 1])
    for batch in a:
        (pa, ta, ua, oa), (pb, tb, ub, ob_) = a[batch], b[batch]
        tri = (pa >= 0) & ~sphere_prim[np.maximum(pa, 0)]                                    # (barycentrics are defined, and used, for triangles only)
        assert np.array_equal(pa, pb) and _same_bits(ta, tb) and _same_bits(ua[tri], ub[tri]) and np.array_equal(oa, ob_), (name, batch)


# ---------------------------------------------------------------- renders
_oracle_renders = {}


def _oracle_render(name, volumetric=False, scene_kw=None):
    """the oracle's accumulation and counters at FILM, computed once per scene and left unchanged"""
    key = (name, volumetric)
    if key not in _oracle_renders:
        from oracle import binding as ob
        w, h, spp = FILM
        tup, fs = sc.scene(name, **(scene_kw or {}))
        rc = make_config(tup[3], width=w, height=h, volumetric=volumetric)
        ref, _, ost = ob.OracleScene(fs, rc.cam_t).render(rc, spp, threads=ob.num_threads())
        ref.setflags(write=False)
        _oracle_renders[key] = (ref, ost)
    return _oracle_renders[key]


def _held_to_exact_row(label, run, ref, ost):
    w, h, spp = FILM
    same = run.accum.view(np.uint32) == ref.view(np.uint32)
    report = lambda m, a, b, fin: record_metric(f"sweep limits: render {label} {w}x{h}x{spp} exact build vs oracle", dict(
        m, bit_equal_frac=float(same.mean()), **{k: run.stats[k] for k in ("n_shade", "n_shadow", "n_lit", "n_draws")}, **{k + "_oracle": ost[k] for k in ("n_shade", "n_shadow", "n_lit", "n_draws")}))
    image_within(run.accum, ref, spp, EXACT.within, EXACT.rel, label=label, report=report)
    assert run.stats["n_samples"] == ost["n_samples"] == w * h * spp, (label, run.stats["n_samples"], ost["n_samples"])
    counters_within(run.stats, ost, EXACT.counters, 0, label=label)


@pytest.mark.parametrize("name,mode", [("tile_34", "tile"), ("tile_35", "sweep"), ("lists_130", "sweep"), ("ties", "tile")])
def test_surface_render_matches_the_oracle(name, mode):
    """the exact build on the oracle's Philox stream, held to parity_bounds.EXACT as test_every_traversal_mode_gives_the_same_hits_and_image
    holds its scene.  Under `sweep` the light samples go through sweep_wg<true>, which nothing else reaches."""
    w, h, spp = FILM
    ref, ost = _oracle_render(name)
    with _open(name, "exact", None if sc.DEFAULT_MODE[name] == mode else mode, w, h) as r:
        _is(r, "exact", mode)
        run = run_of(r, spp)
    assert 0 < run.stats["n_lit"] < run.stats["n_shadow"], run.stats                         # light samples arrive, and some are blocked
    _held_to_exact_row(f"{name} {mode}", run, ref, ost)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", ["tile_34", "ties"])
def test_the_wave_sweep_and_the_tile_render_the_same_run(name, build):
    w, h, spp = FILM
    runs = {}
    for mode in ("sweep", "tile"):
        with _open(name, build, mode, w, h) as r:
            _is(r, build, mode)
            runs[mode] = run_of(r, spp)
    assert runs["sweep"].stats["n_samples"] == w * h * spp and runs["sweep"].stats["n_lit"] > 0
    assert_same_run(runs["sweep"], runs["tile"], f"{name} {build}: sweep against tile")


def test_volumetric_walk_through_the_tile_and_the_wave_sweep():
    """tile_34 with its box a null-surface pane of scattering medium, in a scattering world, through VolumeRenderer on the exact build:
    under `tile` the transmittance walk is k_vshadow<TRACE_TILE> with its 256-thread tile at 34 objects, under `sweep`
    k_vshadow<TRACE_SWEEP>; seven passes per iteration (tests/null_stack_cases.py assert_walk).  The two are the same run, and the run is
    held to the oracle by parity_bounds.EXACT, the row the exact build's volumetric renders of tests/test_gpu_flat_capacity.py are held to."""
    w, h, spp = FILM
    ref, ost = _oracle_render("tile_34", True, {"volumetric": True})
    assert ost["n_track"] > ost["n_shadow"]                                                  # light samples that walk more than one segment
    runs = {}
    for mode in ("tile", "sweep"):
        with _open("tile_34", "exact", mode, w, h, volumetric=True, scene_kw={"volumetric": True}) as r:
            run = runs[mode] = run_of(r, spp)
            ns.assert_walk(r, f"exact/{mode}")
    assert_same_run(runs["tile"], runs["sweep"], "volumetric tile_34: tile against sweep")
    st = runs["tile"].stats
    assert 0 < st["n_track"] <= ost["n_track"], (st["n_track"], ost["n_track"])              # (the device follows only the samples that can contribute)
    _held_to_exact_row("tile_34 volumetric tile", runs["tile"], ref, ost)


def test_product_build_walks_through_the_tile_when_its_flat_walk_is_off():
    """APT_VSHADOW_FLAT=0 puts k_vshadow<TRACE_TILE> in the place of the product build's flat walk (api.hip plan_lds_and_grids: the
    renderer still reports `flat`, the walk takes seven launches per iteration instead of three): the same 256-thread tile at 34 objects
    in the other library, held to the oracle by the row the product build's volumetric renders are held to (VPT_PRODUCT_BOUNDS)."""
    w, h, spp = FILM
    ref, ost = _oracle_render("tile_34", True, {"volumetric": True})
    with open_renderer(sc.scene("tile_34", volumetric=True)[0], w, h, volumetric=True, env={"APT_VSHADOW_FLAT": "0"}) as r:
        run = run_of(r, spp)
        ns.assert_walk(r, "fast/tile")
    image_within(run.accum, ref, spp, VPT_PRODUCT_BOUNDS["within"], VPT_PRODUCT_BOUNDS["rel"], label="tile_34 volumetric, product build, tiled walk",
                 report=lambda m, a, b, fin: record_metric(f"sweep limits: render tile_34 volumetric {w}x{h}x{spp} product build, APT_VSHADOW_FLAT=0, vs oracle", dict(
                     m, n_track=run.stats["n_track"], n_track_oracle=ost["n_track"], n_lit=run.stats["n_lit"], n_lit_oracle=ost["n_lit"])))
    assert run.stats["n_samples"] == ost["n_samples"] == w * h * spp
    counters_within(run.stats, ost, VPT_PRODUCT_BOUNDS["stat_tol"], 0, label="tile_34 volumetric, product build, tiled walk")
    assert 0 < run.stats["n_track"] <= ost["n_track"]


# ---------------------------------------------------------------- feature buffers
@pytest.mark.parametrize("name,mode", [("tile_34", "tile"), ("lists_130", "sweep")])
def test_feature_buffers_through_the_sweeps(name, mode):
    """aov() traces the camera rays of the rendered samples with k_aov_trace<MODE>: under `tile` at 34 objects with 160 KB of LDS, under
    `sweep` through sweep_wg<false> past its 128th list.  Exact build, test_gpu_aov's criterion for the render's own rays: per pixel the
    depth sum and the hit count are the float32 in-order sums over the oracle's hits of the pixel-samples' camera rays - and so are the
    albedo and normal sums, which name the object and the primitive that was hit."""
    w, h, spp = FILM
    tup, fs = sc.scene(name)
    osc, rc, _ = ac.oracle_of(tup, w, h)
    assert rc.anti_alias
    d = np.zeros((w, h, spp, 3), np.float32)
    for i in range(w):
        for j in range(h):
            for s in range(spp):
                d[i, j, s] = osc.pix2ray(rc, i, j, s + 1, ac.jitter(rc, i, j, s + 1))
    hit, prim, t, kd, n_s = ac.oracle_aov(osc, fs, rc, d.reshape(-1, 3))
    want = np.zeros((w, h, 8), np.float32)
    cols = np.concatenate([kd, t[:, None], n_s, hit[:, None].astype(np.float32)], axis=1).astype(np.float32).reshape(w, h, spp, 8)
    for s in range(spp): want = want + cols[:, :, s]                                         # float32, in sample order
    with _open(name, "exact", None if sc.DEFAULT_MODE[name] == mode else mode, w, h) as r:
        _is(r, "exact", mode)
        r.render(n_spp=spp)
        raw = r.tile_aov()
        a = r.aov()
    same = raw.view(np.uint32) == want.view(np.uint32)
    listed = sc.listed_objects(fs)
    past = int(np.isin(sc.prim_object(fs)[prim[hit]], listed[sc.SWEEP_MAX_LISTS:]).sum()) if len(listed) > sc.SWEEP_MAX_LISTS else 0
    record_metric(f"sweep limits: aov {name} {mode} exact build vs oracle", {"rays": int(hit.size), "hits": int(hit.sum()), "bit_equal_frac": float(same.mean()),
                                                                            "depth_bit_equal_frac": float(same[..., 3].mean()), "hits_past_list_128": past})
    assert np.array_equal(raw[..., 7], want[..., 7])
    assert np.array_equal(raw[..., 3], want[..., 3])
    assert np.array_equal(raw[..., 0:3], want[..., 0:3]) and np.array_equal(raw[..., 4:7], want[..., 4:7])
    assert np.array_equal(a["hit_fraction"], want[..., 7] / np.float32(spp)) and hit.mean() > 0.9
    if name == "lists_130": assert past >= 0.05 * hit.size                                   # the camera sees the large objects past list 128
