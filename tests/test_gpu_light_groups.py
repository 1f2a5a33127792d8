"""Light groups on the device, on both builds of the library unless a case says otherwise: the planes cell by cell against
the oracle's single-lit logs (tests/light_group_cases.py; the premise is pinned on the CPU by tests/test_light_groups_host.py), their sum
against the framebuffer and the steady image, relighting against renders of the scene with scaled emitters, small shapes and bookkeeping,
the refusals and the CLI, and the steady, transient and path-length renderers around a light-group one.

The bounds are the project's own for these same records through the same pipeline (tests/test_gpu_path_lengths.py
test_planes_match_the_oracle_log).  The measured figures are in profiles/r07_light_group_metrics.log."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, image_metrics, record_metric
from light_group_cases import CASES, light_group_sums, scaled_lights, single_lit
from adapt_amd.scene_pack import make_config, pack_scene
from oracle import binding as ob

pytestmark = pytest.mark.gpu

BUILDS = ["fast", "exact"]
KW = dict(width=48, height=32, spp_per_batch=4)
# distinct rgb gains per emitter of features_b (quad, ball, pt, spot, beam): a zero, non-powers-of-two, a plain 1
GAINS = np.float32([[0.3, 1.7, 0.9], [2.5, 0.0, 1.1], [0.0, 0.0, 0.0], [1.3, 0.7, 3.1], [1.0, 1.0, 1.0]])


@pytest.fixture
def renderer():
    """factory: Renderer(*scene, exact=..., **kw); every renderer a test makes is closed when the test ends"""
    from adapt_amd.renderer import Renderer
    made = []

    def make(scene, build, **kw):
        r = Renderer(*scene, exact=(build == "exact"), **kw)
        made.append(r)
        return r
    yield make
    for r in made:
        r.close()


@pytest.fixture(scope="module")
def case_ref(parsed):
    """(scene, rc, full log, sums, counts) of a case: the oracle's log of the renderer's samples 1 .. spp and the E single-lit logs
    split by emitter and part, computed once per case"""
    cache = {}

    def get(case):
        if case not in cache:
            name, w, h, spp, _, ov = CASES[case]
            scene = parsed(name)
            rc, fs = make_config(scene[3], width=w, height=h, **ov), pack_scene(*scene)
            full, per, _ = ob.OracleScene(fs, rc.cam_t).contributions(rc, spp)
            singles = [ob.OracleScene(single_lit(fs, k), rc.cam_t).contributions(rc, spp)[0] for k in range(fs.n_sources)]
            assert sum(len(s) for s in singles) == len(full)
            sums, counts = light_group_sums(singles, w * h)
            cache[case] = (scene, rc, full, sums, counts)
        return cache[case]
    return get


def kept_pixels(total, full, npix):
    """-> (keep, inf_pix): the pixels whose device total matches the full log's within 1e-5 (sum of magnitudes) + 1e-12 - there the pixel's
    contributions are the oracle's (the keep rule of tests/test_gpu_path_lengths.py) -, and those with a non-finite record"""
    rgb = full["rgb"].astype(np.float64)
    fin = np.isfinite(rgb).all(axis=1)
    ref_total, ref_mag = np.zeros((npix, 3)), np.zeros((npix, 3))
    np.add.at(ref_total, full["pixel"][fin], rgb[fin])
    np.add.at(ref_mag, full["pixel"][fin], np.abs(rgb[fin]))
    inf_pix = np.zeros(npix, bool)
    inf_pix[full["pixel"][~fin]] = True
    keep = ~inf_pix & np.isfinite(total).all(axis=1) & np.all(np.abs(total - ref_total) <= 1e-5 * ref_mag + 1e-12, axis=1)
    return keep, inf_pix


def rel_err(a, b):
    return np.where(np.abs(a - b) <= 1e-12, 0.0, np.abs(a - b) / np.maximum(np.abs(b), 1e-30))


# ---------------------------------------------------------------- 1. the planes against the single-lit logs
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("case", list(CASES))
def test_planes_match_the_single_lit_logs(case, build, case_ref, renderer, monkeypatch):
    name, w, h, spp, env, ov = CASES[case]
    scene, rc, full, sums, counts = case_ref(case)
    npix, E = w * h, len(scene[0])
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = renderer(scene, build, width=w, height=h, spp_per_batch=4, light_groups=True, **ov)
    info = r.info()
    if "APT_TRAVERSAL" in env:
        assert info["traversal"] == env["APT_TRAVERSAL"]
    assert info["shade_variant"].endswith(" [light groups]")
    if name == "features_b":
        assert info["shade_variant"].startswith("sorted") == ("APT_SORTED" not in env), info["shade_variant"]      # the group twins / the unsorted twin
    assert r.emitter_ids == [e.id for e in scene[0]] and len(r.emitter_ids) == E
    r.render(n_spp=spp)
    planes = r.tile_light_groups()
    assert planes.shape == (E, 2, w, h, 4) == sums.shape[:2] + (w, h, 4)
    planes = planes.reshape(E, 2, npix, 4).astype(np.float64)
    total = r.color.to_numpy().reshape(npix, 3).astype(np.float64)
    st = r.stats()
    assert st["n_stray_light"] == 0, st
    dev_rgb, dev_cnt = planes[..., :3], planes[..., 3]
    assert np.array_equal(dev_cnt, np.round(dev_cnt))
    keep, inf_pix = kept_pixels(total, full, npix)
    diverged = ~keep & ~inf_pix
    d_cnt = np.abs(dev_cnt[:, :, keep] - counts[:, :, keep])
    metric = {"pixels": npix, "records": int(len(full)), "emitters": E, "records_per_emitter": counts.sum((1, 2)).tolist(), "left_out": int(diverged.sum()),
              "n_poisoned": st["n_poisoned"], "max_count_diff": float(d_cnt.max()), "cells_with_count_diff": int((d_cnt > 0).sum())}
    a, b = dev_rgb[:, :, keep], sums[:, :, keep]
    if build == "exact":
        rel, lit = rel_err(a, b), b != 0
        metric["max_rel_cell"] = float(rel.max()) if rel.size else 0.0
        metric["cells_within_1e-5"] = float(np.mean(rel[lit] <= 1e-5)) if lit.any() else 1.0
        print(f"light_group_planes[{case},{build}]: {metric}")
        record_metric(f"light_group_planes[{case},{build}]", metric)
        assert d_cnt.max() == 0, metric
        assert metric["cells_within_1e-5"] >= 0.99 and metric["max_rel_cell"] <= 1e-3, metric
        assert diverged.sum() <= max(st["n_poisoned"], 0) + 0.005 * npix, metric
    else:
        worst = {"relMSE": 0.0, "frac_within": 1.0}
        for e in range(E):
            for part in range(2):
                m = image_metrics(a[e, part].reshape(-1, 1, 3) / spp, b[e, part].reshape(-1, 1, 3) / spp)
                worst = {"relMSE": max(worst["relMSE"], m["relMSE"]), "frac_within": min(worst["frac_within"], m["frac_within"])}
        metric.update(worst_plane_relMSE=worst["relMSE"], worst_plane_frac_within=worst["frac_within"])
        print(f"light_group_planes[{case},{build}]: {metric}")
        record_metric(f"light_group_planes[{case},{build}]", metric)
        assert d_cnt.max() <= 4, metric
        assert diverged.sum() <= 0.2 * npix, metric
        assert worst["frac_within"] >= 0.995 and worst["relMSE"] <= 1e-4, metric


# ---------------------------------------------------------------- 2. sums and neighbours
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("tag,ov", [("features_b", {}), ("features_a", {}), ("cbox", {})])
def test_planes_sum_to_the_image(tag, ov, build, renderer, parsed):
    scene, spp = parsed(tag), 8
    E = len(scene[0])
    steady = renderer(scene, build, **KW, **ov)
    steady.render(n_spp=spp)
    img = steady.color.to_numpy().astype(np.float64)
    lg = renderer(scene, build, light_groups=True, **KW, **ov)
    lg.render(n_spp=spp)
    raw = lg.tile_light_groups().astype(np.float64)
    assert raw.shape == (E, 2, 48, 32, 4)
    assert lg.light_groups().shape == (E, 2, 48, 32, 3) and lg.light_group_counts().shape == (E, 2, 48, 32)
    st, sst = lg.stats(), steady.stats()
    for k in ("n_samples", "n_shade", "n_shadow", "n_draws", "n_poisoned"):      # the same random stream, the same paths
        assert st[k] == sst[k], (k, st[k], sst[k])
    assert st["n_stray_light"] == 0 and sst["n_stray_light"] == 0
    a, mag = raw[..., :3].sum((0, 1)), np.abs(raw[..., :3]).sum((0, 1))
    c = lg.color.to_numpy().astype(np.float64)
    fin = np.isfinite(c).all(axis=2)
    own = np.where(fin[..., None], np.abs(a - c) - 1e-5 * mag, 0.0).max()
    assert np.all(np.abs(a - c)[fin] <= 1e-5 * mag[fin] + 1e-12), own
    # against the steady image: a pixel-sample with a NaN MIS weight is dropped whole by the steady renderer, the planes drop only that
    # contribution: such pixels keep more energy in the planes, at most one pixel per poisoned vertex
    fin &= np.isfinite(img).all(axis=2)
    err = rel_err(a, img).max(axis=2)
    poisoned = fin & (err > 1e-5)
    record_metric(f"light_group_sum[{tag},{build}]", {"max_rel_vs_steady": float(err[fin & ~poisoned].max()), "pixels": int(fin.sum()),
                                                      "poisoned_pixels": int(poisoned.sum()), "n_poisoned": st["n_poisoned"], "own_framebuffer_excess": float(own)})
    assert err[fin & ~poisoned].max() <= 1e-5
    assert poisoned.sum() <= st["n_poisoned"] and np.all(a[poisoned].sum(-1) > img[poisoned].sum(-1))
    # the accessors: normalised like `pixels`; a cell is counted exactly when it holds something
    p = lg.light_groups().astype(np.float64)
    assert np.all(np.abs(p.sum((0, 1)) - lg.pixels.to_numpy())[fin] <= 1e-5 * mag[fin] / spp + 1e-12)
    cnt = lg.light_group_counts()
    assert np.array_equal(cnt > 0, np.any(raw[..., :3] != 0, axis=-1))
    assert cnt[:, 0].sum(0).max() <= spp * lg.max_bounce and cnt[:, 1].sum(0).max() <= spp * lg.max_bounce * max(1, lg.num_shadow_ray)
    if build == "exact":      # the same records in the same order: the framebuffer is a path-length render's, bit for bit
        pl = renderer(scene, build, path_lengths=True, **KW, **ov)
        pl.render(n_spp=spp)
        assert np.array_equal(lg.color.to_numpy(), pl.color.to_numpy(), equal_nan=True)
        # and both splits are splits of the same records: per part they agree in count, and in sum up to the order of the adds
        pr = pl.tile_path_lengths().astype(np.float64)
        assert np.array_equal(pr[..., 3].sum(0), raw[..., 3].sum(0))
        assert np.all(np.abs(pr[..., :3].sum(0) - raw[..., :3].sum(0)) <= 1e-5 * np.abs(raw[..., :3]).sum(0) + 1e-12)


def test_neighbours_are_not_disturbed(renderer, parsed):
    """exact build, features_b: a steady, a transient and a path-length renderer before a light-group one, and again after it - bit-identical"""
    scene, tw = parsed("features_b"), {"sample_count": 60, "min_time": 0.0, "interval": 1.0}
    keys = ("n_samples", "n_extend", "n_shade", "n_shadow", "n_shadow_traced", "n_lit", "n_draws", "n_poisoned")

    def one(**kw):
        r = renderer(scene, "exact", **KW, **kw)
        r.render(n_spp=8)
        extra = r.tile_transient() if "transient" in kw else (r.tile_path_lengths() if "path_lengths" in kw else None)
        return r.color.to_numpy(), {k: r.stats()[k] for k in keys}, r.info()["shade_variant"], extra

    def same(x, y):
        return np.array_equal(x[0], y[0], equal_nan=True) and x[1:3] == y[1:3] and (x[3] is None or np.array_equal(x[3], y[3]))

    before = [one(), one(transient=tw), one(path_lengths=True)]
    lg = renderer(scene, "exact", light_groups=True, **KW)
    lg.render(n_spp=8)
    assert lg.tile_light_groups().any() and before[1][3].any()
    again = renderer(scene, "exact", light_groups=True, **KW)
    again.render(n_spp=8)
    assert np.array_equal(lg.tile_light_groups(), again.tile_light_groups())      # repeated runs: bit-identical
    after = [one(), one(transient=tw), one(path_lengths=True)]
    assert all(same(x, y) for x, y in zip(before, after))
    # the same records in the same order: the light-group render's framebuffer is the transient and the path-length render's
    assert np.array_equal(lg.color.to_numpy(), before[1][0], equal_nan=True) and np.array_equal(lg.color.to_numpy(), before[2][0], equal_nan=True)
    assert {k: lg.stats()[k] for k in keys} == before[1][1] == before[2][1]


# ---------------------------------------------------------------- 3. relighting
@pytest.mark.parametrize("build", BUILDS)
def test_relit_images(build, case_ref, renderer):
    scene, rc, full, sums, counts = case_ref("features_b")
    w, h, spp, npix, E = 48, 32, 8, 48 * 32, 5
    r = renderer(scene, build, light_groups=True, **KW)
    r.render(n_spp=spp)
    raw = r.tile_light_groups()[..., :3]
    mag = np.abs(raw).astype(np.float64).sum((0, 1)) / spp
    planes = r.light_groups().astype(np.float64)
    # gains of one: the planes' sum; one-hot: that emitter's planes
    ones = r.relit(np.ones(E))
    assert ones.shape == (w, h, 3) and ones.dtype == np.float32
    assert np.all(np.abs(ones - planes.sum((0, 1))) <= 1e-6 * mag + 1e-12)
    assert np.all(np.abs(ones - r.pixels.to_numpy()) <= 1e-5 * mag + 1e-12)
    for e in range(E):
        hot = r.relit(np.eye(E, dtype=np.float32)[e])
        assert np.all(np.abs(hot - planes[e].sum(0)) <= 1e-6 * np.abs(planes[e]).sum(0) + 1e-12), e
    # the three forms of gains agree, ids resolve, emitters a dict leaves out keep gain 1
    relit = r.relit(GAINS)
    by_id = {i: tuple(g) for i, g in zip(r.emitter_ids[:4], GAINS[:4])}
    assert r.emitter_ids == ["quad", "ball", "pt", "spot", "beam"]
    assert np.array_equal(r.relit(by_id), relit)
    assert np.array_equal(r.relit({"pt": 0.5}), r.relit([1, 1, 0.5, 1, 1])) and np.array_equal(r.relit({"pt": 0.5}), r.relit(np.float32([[1] * 3, [1] * 3, [0.5] * 3, [1] * 3, [1] * 3])))
    with pytest.raises(KeyError, match="no emitter with id"):
        r.relit({"sun": 2.0})
    with pytest.raises(ValueError, match="per emitter"):
        r.relit([1.0, 2.0])
    ref_np = (planes * GAINS.astype(np.float64)[:, None, None, None, :]).sum((0, 1))
    assert np.all(np.abs(relit - ref_np) <= 1e-6 * (np.abs(planes) * GAINS[:, None, None, None, :]).sum((0, 1)) + 1e-12)
    # against renders of the scene whose emitters' intensities are multiplied by the gains, on the same stream: the device's own, and the oracle's
    emitters = copy.deepcopy(scene[0])
    for em, g in zip(emitters, GAINS):
        em.intensity = (np.float32(em.intensity) * g).astype(np.float32)
    scaled = renderer((emitters,) + tuple(scene[1:]), build, **KW)
    scaled.render(n_spp=spp)
    dev = scaled.pixels.to_numpy().astype(np.float64)
    fs = scaled_lights(pack_scene(*scene), GAINS)
    assert np.array_equal(fs.src_f, scaled.flat.src_f)
    acc, cnt, _ = ob.OracleScene(fs, rc.cam_t).render(rc, spp)
    orc = acc.astype(np.float64) / cnt
    keep, inf_pix = kept_pixels(r.color.to_numpy().reshape(npix, 3).astype(np.float64), full, npix)
    keep = keep.reshape(w, h)
    st = r.stats()
    for what, ref in (("device", dev), ("oracle", orc)):
        a, b = relit.astype(np.float64)[keep], ref[keep]
        m = image_metrics(a.reshape(-1, 1, 3), b.reshape(-1, 1, 3))
        rel, lit = rel_err(a, b), b != 0
        metric = dict(m, left_out=int((~keep).sum()), max_rel=float(rel.max()), within_1e_5=float(np.mean(rel[lit] <= 1e-5)))
        print(f"light_group_relit[{what},{build}]: {metric}")
        record_metric(f"light_group_relit[{what},{build}]", metric)
        if build == "exact":
            assert metric["within_1e_5"] >= 0.99 and metric["max_rel"] <= 1e-3, (what, metric)
            assert (~keep).sum() <= max(st["n_poisoned"], 0) + 0.005 * npix, (what, metric)
        else:
            assert (~keep).sum() <= 0.2 * npix, (what, metric)
            assert m["frac_within"] >= 0.995 and m["relMSE"] <= 1e-4, (what, metric)


# ---------------------------------------------------------------- 4. small shapes and bookkeeping
@pytest.mark.parametrize("build", BUILDS)
def test_small_shapes_and_batch_splits(build, renderer, parsed):
    scene = parsed("features_b")
    # 50 x 30 = 1500 pixels: no multiple of 64; three render() calls across batches; spp_per_batch 3 against 4
    kw = dict(width=50, height=30, light_groups=True)
    a = renderer(scene, build, spp_per_batch=4, **kw)
    b = renderer(scene, build, spp_per_batch=4, **kw)
    c = renderer(scene, build, spp_per_batch=3, **kw)
    a.render(n_spp=8)
    b.render(n_spp=2); b.render(n_spp=5); b.render(n_spp=1)
    c.render(n_spp=8)
    ta, tb, tc = a.tile_light_groups(), b.tile_light_groups(), c.tile_light_groups()
    assert ta.shape == (5, 2, 50, 30, 4) and all(ta[e, 1, ..., 3].any() for e in range(5)) and ta[0, 0, ..., 3].any()
    assert np.array_equal(tb[..., 3], ta[..., 3]) and np.array_equal(tc[..., 3], ta[..., 3])
    for name, t in (("calls", tb), ("batch", tc)):
        diff = rel_err(t[..., :3].astype(np.float64), ta[..., :3].astype(np.float64))
        record_metric(f"light_group_split[{name},{build}]", {"max_rel": float(diff.max())})
        assert diff.max() <= 1e-6, name
    assert a.stats()["n_stray_light"] == b.stats()["n_stray_light"] == c.stats()["n_stray_light"] == 0
    assert not renderer(scene, build, spp_per_batch=4, **kw).relit(GAINS).any()             # a fresh renderer relights zeros
    # max_bounce = 1: part 0 only from the camera rays' hits, part 1 only from the camera vertex - a path-length render's first two cells
    one = renderer(scene, build, spp_per_batch=4, max_bounce=1, **kw)
    one.render(n_spp=4)
    pl = renderer(scene, build, spp_per_batch=4, max_bounce=1, width=50, height=30, path_lengths=True)
    pl.render(n_spp=4)
    t1, p1 = one.tile_light_groups().astype(np.float64), pl.tile_path_lengths().astype(np.float64)
    assert p1.shape == (2, 2, 50, 30, 4) and not p1[0, 1].any() and not p1[1, 0].any()
    assert not t1[2:, 0].any() and t1[:2, 0].any()                                     # only the area lights can be hit
    for part, cell in ((0, p1[0, 0]), (1, p1[1, 1])):
        assert np.array_equal(t1[:, part, ..., 3].sum(0), cell[..., 3])
        assert np.all(np.abs(t1[:, part, ..., :3].sum(0) - cell[..., :3]) <= 1e-6 * np.abs(cell[..., :3]) + 1e-12)


@pytest.mark.parametrize("build", BUILDS)
def test_crop_checkpoint_and_clear(build, renderer, parsed):
    emitters, arrays, objects, prop = parsed("features_b")
    kw = dict(width=64, height=64, spp_per_batch=4, light_groups=True)
    full = renderer(parsed("features_b"), build, **kw)
    full.render(n_spp=4)
    cprop = dict(prop, film=dict(prop["film"], crop_x=30, crop_y=20, crop_rx=10, crop_ry=8))
    crop = renderer((emitters, arrays, objects, cprop), build, **kw)
    crop.render(n_spp=4)
    sx, ex, sy, ey = crop.start_x, crop.end_x, crop.start_y, crop.end_y
    cc, cf = crop.tile_light_groups(), full.tile_light_groups()
    assert (sx, ex, sy, ey) == (20, 40, 12, 28) and cc.shape == cf.shape
    assert np.array_equal(cc[:, :, sx:ex, sy:ey], cf[:, :, sx:ex, sy:ey]) and cc.any()
    outside = np.ones(cc.shape[2:4], bool); outside[sx:ex, sy:ey] = False
    assert not cc[:, :, outside].any() and cf[:, :, outside].any()
    assert not crop.relit(GAINS)[outside].any() and np.array_equal(crop.relit(GAINS)[sx:ex, sy:ey], full.relit(GAINS)[sx:ex, sy:ey])
    # checkpoint: the planes travel with the accumulation and the counter
    cp = full.get_check_point()
    assert cp["light_group_planes"].shape == (5, 2, 64, 64, 4)
    back = renderer(parsed("features_b"), build, **kw)
    back.load_check_point(cp)
    assert back.cnt[None] == 4 and np.array_equal(back.tile_light_groups(), full.tile_light_groups())
    assert np.array_equal(back.relit(GAINS), full.relit(GAINS))
    full.render(n_spp=4); back.render(n_spp=4)
    assert np.array_equal(back.tile_light_groups(), full.tile_light_groups())
    assert np.array_equal(back.color.to_numpy(), full.color.to_numpy(), equal_nan=True)
    # a checkpoint of another layout (another scene's emitters) leaves the planes alone
    other = renderer(parsed("textured"), build, **kw)
    other.render(n_spp=4)
    before = other.tile_light_groups()
    other.load_check_point(dict(other.get_check_point(), light_group_planes=cp["light_group_planes"]))
    assert np.array_equal(other.tile_light_groups(), before)
    full.clear()
    assert not full.tile_light_groups().any() and not full.light_group_counts().any() and full.cnt[None] == 0 and not full.relit(GAINS).any()
    full.render(n_spp=4)
    assert np.array_equal(full.tile_light_groups(), cf)


# ---------------------------------------------------------------- 5. refusals
def test_refused_configurations(renderer, parsed):
    from adapt_amd import _lib
    from adapt_amd.renderer import VolumeRenderer
    kw = dict(width=16, height=16, light_groups=True)
    with pytest.raises(_lib.AptError, match="light groups are a surface-renderer mode"):
        VolumeRenderer(*parsed("cbox"), **kw)
    with pytest.raises(_lib.AptError, match="light groups take at most 4 light samples"):
        renderer(parsed("cbox"), "fast", num_shadow_ray=5, **kw)
    with pytest.raises(_lib.AptError, match="light groups run on one rank"):
        renderer(parsed("cbox"), "fast", world_size=2, rank=0, **kw)
    with pytest.raises(_lib.AptError, match="light groups and transient rendering do not combine"):
        renderer(parsed("cbox"), "fast", transient={"sample_count": 1, "min_time": -1.0, "interval": 1e6}, **kw)
    with pytest.raises(_lib.AptError, match="light groups and path-length images do not combine"):
        renderer(parsed("cbox"), "fast", path_lengths=True, **kw)
    with pytest.raises(_lib.AptError, match="light groups and adaptive sampling do not combine"):
        renderer(parsed("cbox"), "fast", adaptive={"threshold": 0.05}, **kw)
    steady = renderer(parsed("cbox"), "fast", width=16, height=16)
    assert steady.emitter_ids == [e.id for e in parsed("cbox")[0]]
    for call in (steady.light_groups, steady.tile_light_groups, steady.light_group_counts, lambda: steady.relit([1.0]), lambda: steady.light_gains([1.0])):
        with pytest.raises(RuntimeError, match="light_groups=True"):
            call()
    # the C entry points on a renderer without the mode: APT_E_STATE, with the message
    buf = np.zeros(4, np.float32)
    p = buf.ctypes.data_as(_lib.f32p)
    for fn, args in (("apt_read_light_groups", (p,)), ("apt_set_light_groups", (p,)), ("apt_relight", (p, p))):
        assert getattr(steady.lib, fn)(steady.handle, *args) == -5
        assert b"light_groups = 0" in steady.lib.apt_last_error()
    assert "light_group_planes" not in steady.get_check_point()


# ---------------------------------------------------------------- 6. the CLI
def test_cli_writes_one_image_per_emitter(tmp_path):
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "render.py"), "--type", "pt", "--light_groups", "--light_gain", "pt=0.5", "--input_path", os.path.join(ROOT, "scenes"),
           "--scene", "test", "--name", "features_b.xml", "--iter_num", "3", "--width", "64", "--height", "64", "--spp_per_batch", "4",
           "--output_path", str(out) + os.sep, "--chkpt_path", str(tmp_path / "chk") + os.sep, "--no_gui", "--img_ext", "npy"]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    base = "pbr-features_b-pt"
    names = sorted(os.listdir(out))
    assert names == sorted([f"{base}.npy", f"{base}-lights.npy", f"{base}-relit.npy"] + [f"{base}-light{k:02d}.npy" for k in range(5)]), names
    planes, img = np.load(out / f"{base}-lights.npy"), np.load(out / f"{base}.npy")
    assert planes.shape == (5, 2, 64, 64, 3) and img.shape == (64, 64, 3) and img.any()
    mag = np.abs(planes).astype(np.float64).sum((0, 1))
    assert np.all(np.abs(planes.astype(np.float64).sum((0, 1)) - img) <= 1e-5 * mag + 1e-12)
    for k in range(5):
        assert np.array_equal(np.load(out / f"{base}-light{k:02d}.npy"), planes[k].sum(0))
    gains = np.float64([1, 1, 0.5, 1, 1])
    relit = np.load(out / f"{base}-relit.npy")
    assert np.all(np.abs(relit - (planes.astype(np.float64) * gains[:, None, None, None, None]).sum((0, 1))) <= 1e-6 * mag + 1e-12)
    assert np.abs(relit - img).max() > 0                         # the point light does light the scene
    assert "[light groups]" in p.stdout
