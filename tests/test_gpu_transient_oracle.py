"""Transient bins bin by bin against the oracle's per-contribution log (oracle/pt_oracle.c orc_render_contributions, binned by
oracle/binding.py transient_bins: the float32 rule of DESIGN.md §4.5).  The windows come from each case's log: 128 bins between the
0.1 % and 99.9 % quantiles of the contribution times (both tails outside), and a fine window of 256 bins 0.2 % of the median time wide
(about 1 % of a median segment), which puts many contributions near an edge.

Exact build: every bin's count equals the oracle's and its rgb agrees to 1e-5 relative (summation order), on the pixels whose total
(the transient renderer's framebuffer: every contribution, binned or not) matches the log's - the others have a poisoned or diverged
sample (an ulp can re-draw a path) and are counted and bounded.  Product build: on the pixels whose total matches to 1e-5,
the cumulative counts and energy at each edge differ from the oracle's by at most that edge's near-edge records (a time that lies within
2e-5 t of an edge, where the product build's slightly different hits may put it on the other side) plus 1e-5 relative; per-bin relMSE
and frac_within as image_metrics measures them.  The window's edges end to end and the binning rule on explicit times close the file.
The measured figures behind the bounds are in profiles/r06_transient_metrics.log."""
import xml.etree.ElementTree as xet

import numpy as np
import pytest

from conftest import image_metrics, record_metric
from adapt_amd.scene_pack import make_config, pack_scene
from oracle import binding as ob

pytestmark = pytest.mark.gpu

BUILDS = ["fast", "exact"]
# case id: (scene, film width, height, spp, APT_TRAVERSAL, make_config / Renderer overrides)
CASES = {
    "cbox": ("cbox", 48, 32, 8, None, {}),
    "cbox-bvh": ("cbox", 48, 32, 8, "bvh", {}),
    "cbox-sweep": ("cbox", 48, 32, 8, "sweep", {}),
    "cbox-tile": ("cbox", 48, 32, 8, "tile", {}),
    "balls_mono": ("balls_mono", 48, 32, 8, None, {}),                      # S = 4, class-sorted group kernels
    "glass_box": ("glass_box", 48, 32, 8, None, {}),                        # glass ior 1.5
    "features_a": ("features_a", 48, 32, 8, None, {}),                      # five emitter types, frosted 1.33
    "features_c": ("features_c", 48, 32, 8, None, {}),
    "textured": ("textured", 48, 32, 8, None, {}),
    "microfacet": ("microfacet", 48, 32, 8, None, {}),
    "bunnies_small": ("bunnies_small", 64, 48, 8, None, {}),                # the 8-wide tree
    "cbox-S2": ("cbox", 48, 32, 8, None, {"num_shadow_ray": 2}),
    "cbox-S3": ("cbox", 48, 32, 8, None, {"num_shadow_ray": 3}),
    "cbox-ior1.25": ("cbox_ior", 48, 32, 8, None, {}),                      # world medium ior 1.25
}
WINDOWS = ["coarse", "fine"]


class _Medium:
    def __init__(self, ior):
        self.ior = ior


class _World:
    def __init__(self, ior):
        self.medium = _Medium(ior)


@pytest.fixture(scope="module")
def case_scene(parsed):
    cache = {}

    def get(name):
        if name not in cache:
            if name == "bunnies_small":
                from adapt_amd.synth import three_bunnies
                cache[name] = three_bunnies(levels=1)
            elif name == "cbox_ior":
                e, a, o, prop = parsed("cbox")
                cache[name] = (e, a, o, dict(prop, world=_World(1.25)))
            else:
                cache[name] = parsed(name)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def case_log(case_scene):
    """(scene, rc, records, per_sample) of a case: the oracle's log of the renderer's samples 1 .. spp"""
    cache = {}

    def get(case):
        if case not in cache:
            name, w, h, spp, _, ov = CASES[case]
            scene = case_scene(name)
            rc = make_config(scene[3], width=w, height=h, **ov)
            sc = ob.OracleScene(pack_scene(*scene), rc.cam_t, build_bvh=bool(rc.use_bvh) and name == "bunnies_small")
            recs, per, _ = sc.contributions(rc, spp)
            assert recs.nbytes < 50e6
            cache[case] = (scene, rc, recs, per)
        return cache[case]
    return get


def _window(recs, kind):
    t = recs["t32"].astype(np.float64)
    if kind == "coarse":
        lo, hi = np.quantile(t, [0.001, 0.999])
        return np.float32(lo), np.float32((hi - lo) / 128), 128
    step = np.float32(2e-3 * np.median(t))
    return np.float32(np.median(t) - 128 * float(step)), step, 256


def _render(scene, build, w, h, spp, traversal, ov, window, monkeypatch):
    from adapt_amd.renderer import Renderer
    if traversal:
        monkeypatch.setenv("APT_TRAVERSAL", traversal)
    lo, step, n = window
    r = Renderer(*scene, exact=(build == "exact"), width=w, height=h, spp_per_batch=min(spp, 4),
                 transient={"sample_count": n, "min_time": float(lo), "interval": float(step)}, **ov)
    try:
        assert r.rc.transient_min_time == float(lo) and r.rc.transient_interval == float(step)
        if traversal:
            assert r.info()["traversal"] == traversal
        r.render(n_spp=spp)
        cube = r.tile_transient().reshape(n, w * h, 4).astype(np.float64)
        total = r.color.to_numpy().reshape(w * h, 3).astype(np.float64)
        return cube, total, r.stats()
    finally:
        r.close()


def _cumulative_excess(dev, ref, near):
    """per pixel: max over edges k = 1..n of |cumsum(dev - ref)[k]| - (near[0] + near[k]) - a record that moves across edge k changes
    the sum below k by itself, one that crosses edge 0 (into or out of the window) every sum above it; moves across other edges cancel"""
    d = np.cumsum(dev - ref, axis=0)                             # [k - 1]: the bins below edge k
    allow = near[0][None] + near[1:]
    return np.abs(d) - allow


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("case", list(CASES))
def test_bins_match_the_oracle_log(case, build, window, case_log, monkeypatch):
    name, w, h, spp, traversal, ov = CASES[case]
    scene, rc, recs, per = case_log(case)
    lo, step, n = win = _window(recs, window)
    npix = w * h
    # near an edge: within 2e-5 t for the exact build (its times are the oracle's); the product build's hit distances are the oracle's only
    # to 1e-5 relative per segment, over paths of up to ~10 segments: 1e-4 t (at 2e-5 it moved 1-2 records more per case)
    sums, counts, near_cnt, near_e = ob.transient_bins(recs, npix, lo, step, n, near_rel=2e-5 if build == "exact" else 1e-4)
    cube, total, st = _render(scene, build, w, h, spp, traversal, ov, win, monkeypatch)
    dev_rgb, dev_cnt = cube[..., :3], cube[..., 3]
    assert np.array_equal(dev_cnt, np.round(dev_cnt))
    # the pixel's total is time-independent: where it matches the log's, the pixel's contributions are the oracle's
    rgb = recs["rgb"].astype(np.float64)
    fin = np.isfinite(rgb).all(axis=1)
    ref_total, ref_mag = np.zeros((npix, 3)), np.zeros((npix, 3))
    np.add.at(ref_total, recs["pixel"][fin], rgb[fin])
    np.add.at(ref_mag, recs["pixel"][fin], np.abs(rgb[fin]))
    inf_pix = np.zeros(npix, bool)
    inf_pix[recs["pixel"][~fin]] = True
    keep = ~inf_pix & np.isfinite(total).all(axis=1) & np.all(np.abs(total - ref_total) <= 1e-5 * ref_mag + 1e-12, axis=1)
    dropped_pix = per[..., 4].reshape(npix, spp).any(axis=1)         # a NaN colour in the oracle: the device drops another term set
    diverged = ~keep & ~inf_pix
    metric = {"pixels": npix, "records": int(len(recs)), "binned": int(counts.sum()), "near_edge": int(near_cnt.sum()),
              "left_out": int(diverged.sum()), "left_out_with_nan_sample": int((diverged & dropped_pix).sum()), "n_poisoned": st["n_poisoned"],
              "window": [float(lo), float(step), n]}
    cnt_x = _cumulative_excess(dev_cnt[:, keep], counts[:, keep].astype(np.float64), near_cnt[:, keep].astype(np.float64))
    e_dev, e_ref = dev_rgb[:, keep].sum(-1), sums[:, keep].sum(-1)
    e_rel = 1e-5 if build == "exact" else 1e-4                     # product: fast reciprocals in the light terms
    e_x = _cumulative_excess(e_dev, e_ref, near_e[:, keep].sum(-1)) - e_rel * ref_mag[keep].sum(-1)[None]
    moved = np.any(dev_cnt[:, keep] != counts[:, keep], axis=0)
    metric.update(moved_pixels=int(moved.sum()), count_excess=float(cnt_x.max()), energy_excess=float(e_x.max()))
    if build == "exact":
        same = ~moved
        rel = np.abs(dev_rgb[:, keep][:, same] - sums[:, keep][:, same]) / np.maximum(np.abs(sums[:, keep][:, same]), 1e-30)
        rel = np.where(np.abs(dev_rgb[:, keep][:, same] - sums[:, keep][:, same]) <= 1e-12, 0.0, rel)
        lit = sums[:, keep][:, same] != 0
        metric["max_rel_bin"] = float(rel.max()) if rel.size else 0.0
        metric["bins_within_1e-5"] = float(np.mean(rel[lit] <= 1e-5)) if lit.any() else 1.0
        record_metric(f"transient_oracle_bins[{case},{build},{window}]", metric)
        # the exact build's hits, draws and light positions are the oracle's: the same counts bin for bin, the same rgb to summation order
        # on almost every bin.  A few dim bins differ more: the exact build's transcendentals are the double ones rounded once, the
        # oracle's glibc's float ones (a few ulp a call), chained along a path (measured: at most 2.7e-4 on cbox S = 3).
        assert metric["max_rel_bin"] <= 1e-3 and metric["bins_within_1e-5"] >= 0.99, metric
        assert moved.sum() <= max(1, int(near_cnt[:, keep].any(axis=0).sum())), metric
        assert cnt_x.max() <= 0 and e_x.max() <= 0, metric
        # the pixels left out: a poisoned / NaN sample, or a path an ulp re-drew - at most 0.5 % of them beyond the former
        assert (diverged & ~dropped_pix).sum() <= max(st["n_poisoned"], 0) + 0.005 * npix, metric
    else:
        a = dev_rgb[:, keep].reshape(-1, 1, 3) / spp
        b = sums[:, keep].reshape(-1, 1, 3) / spp
        m = image_metrics(a, b)
        metric.update(relMSE=m["relMSE"], frac_within=m["frac_within"])
        record_metric(f"transient_oracle_bins[{case},{build},{window}]", metric)
        # a weak light sample can exist in one build and not the other (an occlusion test or a zero term decided by an ulp): its energy is
        # below the filter's, its count is not - measured at most 2 such per pixel (bound: twice that); a wrong time moves hundreds
        assert cnt_x.max() <= 4 and e_x.max() <= 0, metric
        # the product build's images match the oracle's to 1e-3 (1 + x), not 1e-5: pixels whose total differs more are left out
        # (measured: up to 15.4 % of them on features_c, 4 % on features_a, at most 3.4 % elsewhere)
        assert diverged.sum() <= 0.2 * npix, metric
        assert m["frac_within"] >= 0.995 and m["relMSE"] <= 1e-4, metric


# ---------------------------------------------------------------- the window's edges end to end (exact build)
def _light_wall(w, h):
    """camera rays (anti-aliasing off, one bounce) hit an area-light quad at z = 8 head-on: each pixel has one contribution, the emitter
    hit at the camera ray's length, whose float32 time the oracle gives bit for bit"""
    from adapt_amd.emitters import SOURCE_MAP
    from adapt_amd.synth import _Builder, _brdf, _sensor
    from transient_cases import _quad
    b = _Builder()
    b.mesh(_quad(8.0, -1.0), _brdf("lambertian", "#BDBDBD"), emitter=0)
    area = SOURCE_MAP["area"](xet.fromstring('<emitter type="area" id="a"><rgb name="emission" value="5.0, 5.0, 5.0"/></emitter>'))
    scene = b.finish([area], _sensor(w, h, 1, 1))
    scene[3]["anti_alias"] = False
    return scene


@pytest.fixture(scope="module")
def wall():
    w, h = 24, 16
    scene = _light_wall(w, h)
    rc = make_config(scene[3], width=w, height=h)
    recs, per, _ = ob.OracleScene(pack_scene(*scene), rc.cam_t).contributions(rc, 1)
    assert len(recs) == w * h and np.all(recs["kind"] == 0) and np.array_equal(recs["pixel"], np.arange(w * h))
    return scene, w, h, recs["t32"]


def _wall_counts(wall, window, monkeypatch):
    scene, w, h, t = wall
    cube, total, st = _render(scene, "exact", w, h, 1, None, {}, window, monkeypatch)
    return cube[..., 3]


def _search_max_time_on(t_q, lo, n):
    """an interval whose window end, rounded from double, is exactly t_q"""
    base = np.float32((float(t_q) - float(lo)) / n)
    for k in range(-64, 65):
        step = base
        for _ in range(abs(k)):
            step = np.nextafter(step, np.float32(np.inf if k > 0 else -np.inf))
        if ob.transient_max_time(lo, step, n) == t_q:
            return step
    return None


def _search_round_up(t, order):
    """(pixel, min_time, interval, n_bins) with t[pixel] < max_time whose quotient float32(t - min_time) / interval rounds to n_bins"""
    for lo in (np.float32(-7.1), np.float32(0.0), np.float32(float(t.min()) * 0.5), np.float32(float(t.min()) - 1.0)):
        for n in (3, 5, 7, 10, 100):
            for q in order[::-1]:
                step = np.float32((float(t[q]) - float(lo)) / n)
                for _ in range(16):
                    step = np.nextafter(step, np.float32(np.inf))
                    if t[q] < ob.transient_max_time(lo, step, n) and (t[q] - lo) / step >= np.float32(n):
                        return q, lo, step, n
    return None


def test_window_edges_end_to_end(wall, monkeypatch):
    scene, w, h, t = wall
    order = np.argsort(t, kind="stable")
    # min_time equal to a pixel's time drops that pixel (strict lower bound), keeps the one just later
    p = int(order[len(t) // 2])
    lo, n = t[p], 4
    step = np.float32((float(t.max()) - float(lo)) / n * 1.01)
    counts = _wall_counts(wall, (lo, step, n), monkeypatch)
    recs = np.zeros(len(t), ob.CONTRIB_DTYPE)
    recs["pixel"], recs["rgb"], recs["t32"], recs["t64"] = np.arange(len(t)), 1.0, t, t
    _, ref, _, _ = ob.transient_bins(recs, len(t), lo, step, n)
    assert counts[:, p].sum() == 0 and np.array_equal(counts, ref)
    assert ref.sum() == (t > lo).sum()
    # a window whose float32 end is exactly a pixel's time drops that pixel (strict upper bound)
    lo2, n2 = np.float32(float(t.min()) - 1.0), 3
    for q in order[::-1][:40]:
        step2 = _search_max_time_on(t[q], lo2, n2)
        if step2 is not None and (t < t[q]).any():
            break
    assert step2 is not None
    counts2 = _wall_counts(wall, (lo2, step2, n2), monkeypatch)
    _, ref2, _, _ = ob.transient_bins(recs, len(t), lo2, step2, n2)
    assert counts2[:, q].sum() == 0 and np.array_equal(counts2, ref2) and (t == t[q]).sum() == (ref2.sum(0) == 0).sum()
    # a window in which a pixel's quotient rounds up to n_bins: the pixel lands in the last bin
    found = _search_round_up(t, order)
    assert found is not None
    q, lo3, step3, n3 = found
    counts3 = _wall_counts(wall, (lo3, step3, n3), monkeypatch)
    _, ref3, _, _ = ob.transient_bins(recs, len(t), lo3, step3, n3)
    assert counts3[n3 - 1, q] == 1 and np.array_equal(counts3, ref3)
    record_metric("transient_window_edges[exact]", {"min_pixel_time": float(lo), "max_time": float(t[order[-1]]), "round_up": [float(t[q]), float(lo3), float(step3), n3]})


# ---------------------------------------------------------------- the binning rule on explicit times, both builds
def _probe(build, t, lo, step, n):
    from adapt_amd import _lib
    lib = _lib.load(build)
    t = np.ascontiguousarray(t, np.float32)
    out = np.full(len(t), -7, np.int32)
    _lib.check(lib.apt_transient_bin_probe(0, len(t), t.ctypes.data_as(_lib.f32p), float(lo), float(step), int(n), out.ctypes.data_as(_lib.i32p)),
               "apt_transient_bin_probe", lib)
    return out


def _edge_times(rng, lo, step, n, count):
    """times at and a few ulp around every edge (the window's ends included), NaN / inf, and uniform times over the window"""
    edges = np.float32(float(lo) + float(step) * np.arange(n + 1, dtype=np.float64))
    edges = np.concatenate([edges, [ob.transient_max_time(lo, step, n), np.float32(lo)]]).astype(np.float32)
    around = [edges]
    up, down = edges.copy(), edges.copy()
    for _ in range(4):
        up, down = np.nextafter(up, np.float32(np.inf)), np.nextafter(down, np.float32(-np.inf))
        around += [up, down]
    rest = count - sum(len(a) for a in around) - 3
    uni = rng.uniform(float(lo) - float(step), float(lo) + float(step) * (n + 1), rest).astype(np.float32)
    return np.concatenate(around + [np.float32([np.nan, np.inf, -np.inf]), uni])


@pytest.mark.parametrize("build", BUILDS)
def test_bin_probe_matches_the_rule(build):
    rng = np.random.default_rng(5)
    from transient_cases import _rounding_up_window
    lo_r, step_r, n_r, t_r = _rounding_up_window()
    windows = [(np.float32(2.5), np.float32(0.25), 8), (np.float32(-7.1), np.float32(0.013), 400), (np.float32(10.3), np.float32(0.7), 100),
               (np.float32(11.0), np.float32(0.05), 200), (lo_r, step_r, n_r)]
    per = 1_000_000 // len(windows)
    total_mismatch = 0
    for lo, step, n in windows:
        t = _edge_times(rng, lo, step, n, per)
        if (lo, step, n) == (lo_r, step_r, n_r):
            t = np.concatenate([t, [t_r]]).astype(np.float32)
        got, want = _probe(build, t, lo, step, n), ob.transient_bin_index(t, lo, step, n)
        bad = np.flatnonzero(got != want)
        total_mismatch += len(bad)
        assert len(bad) == 0, (float(lo), float(step), n, [(float(t[k]), int(got[k]), int(want[k])) for k in bad[:5]])
    assert _probe(build, [t_r], lo_r, step_r, n_r).tolist() == [n_r - 1]
    record_metric(f"transient_bin_probe[{build}]", {"times": per * len(windows), "mismatches": total_mismatch})
