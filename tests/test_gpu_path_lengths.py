"""Path-length images on the device, on both builds of the library unless a case says otherwise: the planes cell by
cell against the oracle's per-contribution log split by the same rule (tests/path_length_cases.py path_length_sums, pinned on the CPU
by tests/test_path_lengths_host.py), their sum against the framebuffer and the steady image, small shapes and bookkeeping, the refusals
and the CLI, and the steady and transient renderers around a path-length one.

The bounds are the project's existing ones for the same renders through the same pipeline (tests/test_gpu_transient_oracle.py,
tests/test_gpu_transient.py; SURVEY 8(d) for the product build).  The measured figures are in profiles/r07_path_length_metrics.log."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, image_metrics, record_metric
from path_length_cases import CASES, path_length_sums
from adapt_amd.scene_pack import make_config, pack_scene
from oracle import binding as ob

pytestmark = pytest.mark.gpu

BUILDS = ["fast", "exact"]
KW = dict(width=48, height=32, spp_per_batch=4)


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
def case_log(parsed):
    """(scene, rc, records, per_sample) of a case: the oracle's log of the renderer's samples 1 .. spp, computed once per case"""
    scenes, cache = {}, {}

    def get(case):
        if case not in cache:
            name, w, h, spp, _, ov = CASES[case]
            if name not in scenes:
                if name == "bunnies_small":
                    from adapt_amd.synth import three_bunnies
                    scenes[name] = three_bunnies(levels=1)
                else:
                    scenes[name] = parsed(name)
            scene = scenes[name]
            rc = make_config(scene[3], width=w, height=h, **ov)
            sc = ob.OracleScene(pack_scene(*scene), rc.cam_t, build_bvh=bool(rc.use_bvh) and name == "bunnies_small")
            recs, per, _ = sc.contributions(rc, spp)
            assert recs.nbytes < 50e6
            cache[case] = (scene, rc, recs, per)
        return cache[case]
    return get


# ---------------------------------------------------------------- 1. the planes against the oracle log
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("case", list(CASES))
def test_planes_match_the_oracle_log(case, build, case_log, renderer, monkeypatch):
    name, w, h, spp, traversal, ov = CASES[case]
    scene, rc, recs, per = case_log(case)
    npix, L = w * h, rc.max_bounce + 1
    if traversal:
        monkeypatch.setenv("APT_TRAVERSAL", traversal)
    r = renderer(scene, build, width=w, height=h, spp_per_batch=4, path_lengths=True, **ov)
    if traversal:
        assert r.info()["traversal"] == traversal
    assert r.info()["shade_variant"].endswith(" [path lengths]")
    r.render(n_spp=spp)
    planes = r.tile_path_lengths()
    assert planes.shape == (L, 2, w, h, 4)
    planes = planes.reshape(L, 2, npix, 4).astype(np.float64)
    total = r.color.to_numpy().reshape(npix, 3).astype(np.float64)
    st = r.stats()
    dev_rgb, dev_cnt = planes[..., :3], planes[..., 3]
    assert np.array_equal(dev_cnt, np.round(dev_cnt))
    sums, counts = path_length_sums(recs, npix, rc.max_bounce)
    # the pixel's total does not depend on the split: where it matches the log's, the pixel's contributions are the oracle's
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
    d_cnt = np.abs(dev_cnt[:, :, keep] - counts[:, :, keep])
    metric = {"pixels": npix, "records": int(len(recs)), "planes": L, "left_out": int(diverged.sum()),
              "left_out_with_nan_sample": int((diverged & dropped_pix).sum()), "n_poisoned": st["n_poisoned"],
              "max_count_diff": float(d_cnt.max()), "cells_with_count_diff": int((d_cnt > 0).sum())}
    a, b = dev_rgb[:, :, keep], sums[:, :, keep]
    if build == "exact":
        rel = np.where(np.abs(a - b) <= 1e-12, 0.0, np.abs(a - b) / np.maximum(np.abs(b), 1e-30))
        lit = b != 0
        metric["max_rel_cell"] = float(rel.max()) if rel.size else 0.0
        metric["cells_within_1e-5"] = float(np.mean(rel[lit] <= 1e-5)) if lit.any() else 1.0
        record_metric(f"path_length_planes[{case},{build}]", metric)
        assert d_cnt.max() == 0, metric
        assert metric["cells_within_1e-5"] >= 0.99 and metric["max_rel_cell"] <= 1e-3, metric
        assert (diverged & ~dropped_pix).sum() <= max(st["n_poisoned"], 0) + 0.005 * npix, metric
    else:
        worst = {"relMSE": 0.0, "frac_within": 1.0}
        for l in range(L):
            m = image_metrics(a[l].reshape(-1, 1, 3) / spp, b[l].reshape(-1, 1, 3) / spp)
            worst = {"relMSE": max(worst["relMSE"], m["relMSE"]), "frac_within": min(worst["frac_within"], m["frac_within"])}
        metric.update(worst_plane_relMSE=worst["relMSE"], worst_plane_frac_within=worst["frac_within"])
        record_metric(f"path_length_planes[{case},{build}]", metric)
        assert d_cnt.max() <= 4, metric
        assert diverged.sum() <= 0.2 * npix, metric
        assert worst["frac_within"] >= 0.995 and worst["relMSE"] <= 1e-4, metric


# ---------------------------------------------------------------- 2. the planes sum to the framebuffer and to the steady image
SUM_CASES = [("cbox", None, {}), ("balls_mono", None, {}), ("glass_box", None, {}), ("cbox", "bvh", {}), ("cbox", None, {"max_bounce": 2})]


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("tag,traversal,ov", SUM_CASES)
def test_planes_sum_to_the_image(tag, traversal, ov, build, renderer, parsed, monkeypatch):
    if traversal:
        monkeypatch.setenv("APT_TRAVERSAL", traversal)
    scene, spp = parsed(tag), 8
    steady = renderer(scene, build, **KW, **ov)
    steady.render(n_spp=spp)
    img = steady.color.to_numpy().astype(np.float64)
    pl = renderer(scene, build, path_lengths=True, **KW, **ov)
    pl.render(n_spp=spp)
    raw = pl.tile_path_lengths().astype(np.float64)
    L = pl.max_bounce + 1
    assert raw.shape == (L, 2, 48, 32, 4)                            # no plane above what max_bounce allows
    assert pl.path_lengths().shape == (L, 2, 48, 32, 3) and pl.path_length_counts().shape == (L, 2, 48, 32)
    assert not raw[0, 1].any() and not raw[L - 1, 0].any()           # no light sample of length 1, no sampled ray beyond the last vertex
    st, sst = pl.stats(), steady.stats()
    for k in ("n_samples", "n_shade", "n_shadow", "n_draws", "n_poisoned"):      # the same random stream, the same paths
        assert st[k] == sst[k], (k, st[k], sst[k])
    a, mag = raw[..., :3].sum((0, 1)), np.abs(raw[..., :3]).sum((0, 1))
    c = pl.color.to_numpy().astype(np.float64)
    fin = np.isfinite(c).all(axis=2)
    own = np.where(fin[..., None], np.abs(a - c) - 1e-5 * mag, 0.0).max()
    assert np.all(np.abs(a - c)[fin] <= 1e-5 * mag[fin] + 1e-12), own
    # against the steady image: a pixel-sample with a NaN MIS weight is dropped whole by the steady renderer, the planes drop only that
    # contribution: such pixels keep more energy in the planes, at most one pixel per poisoned vertex
    fin &= np.isfinite(img).all(axis=2)
    err = np.where(np.abs(a - img) <= 1e-12, 0.0, np.abs(a - img) / np.maximum(np.abs(img), 1e-30)).max(axis=2)
    poisoned = fin & (err > 1e-5)
    record_metric(f"path_length_sum[{tag},{traversal},{ov},{build}]", {"max_rel_vs_steady": float(err[fin & ~poisoned].max()), "pixels": int(fin.sum()),
                                                                        "poisoned_pixels": int(poisoned.sum()), "n_poisoned": st["n_poisoned"],
                                                                        "own_framebuffer_excess": float(own)})
    assert err[fin & ~poisoned].max() <= 1e-5
    assert poisoned.sum() <= st["n_poisoned"] and np.all(a[poisoned].sum(-1) > img[poisoned].sum(-1))
    # the accessors: normalised like `pixels`, and the three named images are the planes
    p = pl.path_lengths().astype(np.float64)
    assert np.all(np.abs(p.sum((0, 1)) - pl.pixels.to_numpy())[fin] <= 1e-5 * mag[fin] / spp + 1e-12)
    assert np.array_equal(pl.emission(), pl.path_lengths()[0].sum(0)) and np.array_equal(pl.direct(), pl.path_lengths()[1].sum(0))
    assert np.array_equal(pl.indirect(), pl.path_lengths()[2:].sum((0, 1)))
    counts = pl.path_length_counts()
    assert np.array_equal(counts > 0, np.any(raw[..., :3] != 0, axis=-1))
    assert counts[:, 0].max() <= spp and counts[:, 1].max() <= spp * max(1, pl.num_shadow_ray)


# ---------------------------------------------------------------- 3. small shapes and bookkeeping
@pytest.mark.parametrize("build", BUILDS)
def test_small_shapes_and_batch_splits(build, renderer, parsed):
    scene = parsed("cbox")
    # 50 x 30 = 1500 pixels: no multiple of 64; three render() calls across batches; spp_per_batch 3 against 4
    kw = dict(width=50, height=30, path_lengths=True)
    a = renderer(scene, build, spp_per_batch=4, **kw)
    b = renderer(scene, build, spp_per_batch=4, **kw)
    c = renderer(scene, build, spp_per_batch=3, **kw)
    a.render(n_spp=8); b.render(n_spp=8)
    c.render(n_spp=2); c.render(n_spp=5); c.render(n_spp=1)
    ta, tb, tc = a.tile_path_lengths(), b.tile_path_lengths(), c.tile_path_lengths()
    assert ta.shape == (a.max_bounce + 1, 2, 50, 30, 4) and ta[..., 3].any()
    assert np.array_equal(ta, tb) and np.array_equal(a.color.to_numpy(), b.color.to_numpy())
    assert np.array_equal(tc[..., 3], ta[..., 3])
    diff = np.abs(tc[..., :3] - ta[..., :3]) / np.maximum(np.abs(ta[..., :3]), 1e-30)
    diff = np.where(np.abs(tc[..., :3] - ta[..., :3]) <= 1e-12, 0.0, diff)
    record_metric(f"path_length_batch_split[{build}]", {"max_rel": float(diff.max())})
    assert diff.max() <= 1e-6
    # max_bounce = 1: two planes, emission and the light samples of the camera vertex
    one = renderer(scene, build, spp_per_batch=4, max_bounce=1, **kw)
    one.render(n_spp=4)
    t1 = one.tile_path_lengths()
    assert t1.shape == (2, 2, 50, 30, 4) and not t1[0, 1].any() and not t1[1, 0].any() and t1[1, 1].any()
    assert not one.indirect().any()
    a4 = renderer(scene, build, spp_per_batch=4, **kw)
    a4.render(n_spp=4)
    assert np.array_equal(t1[0, 0], a4.tile_path_lengths()[0, 0]) and np.array_equal(t1[1, 1], a4.tile_path_lengths()[1, 1])      # the same first vertex
    # the feature buffers are a pass of their own
    steady = renderer(scene, build, spp_per_batch=4, width=50, height=30)
    steady.render(n_spp=4)
    fa, fs = a4.aov(), steady.aov()
    assert all(np.array_equal(fa[k], fs[k]) for k in fs)


@pytest.mark.parametrize("build", BUILDS)
def test_crop_checkpoint_and_clear(build, renderer, parsed):
    emitters, arrays, objects, prop = parsed("cbox")
    kw = dict(width=64, height=64, spp_per_batch=4, path_lengths=True)
    full = renderer(parsed("cbox"), build, **kw)
    full.render(n_spp=4)
    cprop = dict(prop, film=dict(prop["film"], crop_x=30, crop_y=20, crop_rx=10, crop_ry=8))
    crop = renderer((emitters, arrays, objects, cprop), build, **kw)
    crop.render(n_spp=4)
    sx, ex, sy, ey = crop.start_x, crop.end_x, crop.start_y, crop.end_y
    cc, cf = crop.tile_path_lengths(), full.tile_path_lengths()
    assert (sx, ex, sy, ey) == (20, 40, 12, 28) and cc.shape == cf.shape
    assert np.array_equal(cc[:, :, sx:ex, sy:ey], cf[:, :, sx:ex, sy:ey]) and cc.any()
    outside = np.ones(cc.shape[2:4], bool); outside[sx:ex, sy:ey] = False
    assert not cc[:, :, outside].any() and cf[:, :, outside].any()
    # checkpoint: the planes travel with the accumulation and the counter
    cp = full.get_check_point()
    L = full.max_bounce + 1
    assert cp["path_length_planes"].shape == (L, 2, 64, 64, 4)
    back = renderer(parsed("cbox"), build, **kw)
    back.load_check_point(cp)
    assert back.cnt[None] == 4 and np.array_equal(back.tile_path_lengths(), full.tile_path_lengths())
    full.render(n_spp=4); back.render(n_spp=4)
    assert np.array_equal(back.tile_path_lengths(), full.tile_path_lengths())
    assert np.array_equal(back.color.to_numpy(), full.color.to_numpy(), equal_nan=True)
    # a checkpoint of another layout leaves the planes alone
    other = renderer(parsed("cbox"), build, max_bounce=2, **kw)
    other.render(n_spp=4)
    before = other.tile_path_lengths()
    other.load_check_point(dict(other.get_check_point(), path_length_planes=cp["path_length_planes"]))
    assert np.array_equal(other.tile_path_lengths(), before)
    full.clear()
    assert not full.tile_path_lengths().any() and not full.path_length_counts().any() and full.cnt[None] == 0
    full.render(n_spp=4)
    assert np.array_equal(full.tile_path_lengths(), cf)


# ---------------------------------------------------------------- 4. refusals and the CLI
def test_refused_configurations(renderer, parsed):
    from adapt_amd import _lib
    from adapt_amd.renderer import VolumeRenderer
    kw = dict(width=16, height=16, path_lengths=True)
    with pytest.raises(_lib.AptError, match="path-length images are a surface-renderer mode"):
        VolumeRenderer(*parsed("cbox"), **kw)
    with pytest.raises(_lib.AptError, match="path-length images take at most 4 light samples"):
        renderer(parsed("cbox"), "fast", num_shadow_ray=5, **kw)
    with pytest.raises(_lib.AptError, match="path-length images run on one rank"):
        renderer(parsed("cbox"), "fast", world_size=2, rank=0, **kw)
    with pytest.raises(_lib.AptError, match="path-length images and transient rendering do not combine"):
        renderer(parsed("cbox"), "fast", transient={"sample_count": 1, "min_time": -1.0, "interval": 1e6}, **kw)
    with pytest.raises(_lib.AptError, match="path-length images and adaptive sampling do not combine"):
        renderer(parsed("cbox"), "fast", adaptive={"threshold": 0.05}, **kw)
    steady = renderer(parsed("cbox"), "fast", width=16, height=16)
    for call in (steady.path_lengths, steady.tile_path_lengths, steady.path_length_counts, steady.emission, steady.direct, steady.indirect):
        with pytest.raises(RuntimeError, match="path_lengths=True"):
            call()
    # the C entry points on a renderer without the mode: APT_E_STATE (-3 in include/adapt_mi.h's order is not assumed: non-zero, with the message)
    buf = np.zeros(4, np.float32)
    for fn in ("apt_read_path_lengths", "apt_set_path_lengths"):
        assert getattr(steady.lib, fn)(steady.handle, buf.ctypes.data_as(_lib.f32p)) != 0
        assert b"path_lengths = 0" in steady.lib.apt_last_error()
    assert "path_length_planes" not in steady.get_check_point()


def test_cli_writes_one_image_per_length(tmp_path, parsed):
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "render.py"), "--type", "pt", "--path_lengths", "--input_path", os.path.join(ROOT, "scenes"),
           "--scene", "cbox", "--name", "c2_cbox.xml", "--iter_num", "3", "--width", "64", "--height", "64", "--spp_per_batch", "4",
           "--output_path", str(out) + os.sep, "--chkpt_path", str(tmp_path / "chk") + os.sep, "--no_gui", "--img_ext", "npy"]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    L = int(parsed("cbox")[3]["max_bounce"]) + 1
    names = sorted(os.listdir(out))
    assert names == sorted(["pbr-c2_cbox-pt.npy", "pbr-c2_cbox-pt-lengths.npy"] + [f"pbr-c2_cbox-pt-len{n:02d}.npy" for n in range(1, L + 1)]), names
    planes, img = np.load(out / "pbr-c2_cbox-pt-lengths.npy"), np.load(out / "pbr-c2_cbox-pt.npy")
    assert planes.shape == (L, 2, 64, 64, 3) and img.shape == (64, 64, 3) and img.any()
    assert np.all(np.abs(planes.astype(np.float64).sum((0, 1)) - img) <= 1e-5 * np.abs(planes).astype(np.float64).sum((0, 1)) + 1e-12)
    for n in range(1, L + 1):
        assert np.array_equal(np.load(out / f"pbr-c2_cbox-pt-len{n:02d}.npy"), planes[n - 1].sum(0))
    assert "[path lengths]" in p.stdout


# ---------------------------------------------------------------- 5. nothing else moved
def test_neighbours_are_not_disturbed(renderer, parsed):
    """exact build, cbox: a steady and a transient renderer before a path-length one, and again after it - bit-identical pairs"""
    scene, tw = parsed("cbox"), {"sample_count": 60, "min_time": 11.0, "interval": 0.25}
    keys = ("n_samples", "n_extend", "n_shade", "n_shadow", "n_shadow_traced", "n_lit", "n_draws", "n_poisoned")

    def steady():
        r = renderer(scene, "exact", **KW)
        r.render(n_spp=8)
        return r.color.to_numpy(), {k: r.stats()[k] for k in keys}, r.info()["shade_variant"]

    def transient():
        r = renderer(scene, "exact", transient=tw, **KW)
        r.render(n_spp=8)
        return r.color.to_numpy(), {k: r.stats()[k] for k in keys}, r.tile_transient(), r.info()["shade_variant"]

    s0, t0 = steady(), transient()
    pl = renderer(scene, "exact", path_lengths=True, **KW)
    pl.render(n_spp=8)
    assert pl.tile_path_lengths().any()
    s1, t1 = steady(), transient()
    assert np.array_equal(s0[0], s1[0], equal_nan=True) and s0[1:] == s1[1:]
    assert np.array_equal(t0[0], t1[0], equal_nan=True) and t0[1] == t1[1] and np.array_equal(t0[2], t1[2]) and t0[3] == t1[3]
    # the same records in the same order: the path-length render's framebuffer is the transient render's, bit for bit
    assert np.array_equal(pl.color.to_numpy(), t0[0], equal_nan=True) and {k: pl.stats()[k] for k in keys} == t0[1]
