"""Adaptive sampling on the device, on both builds of the library unless a case says otherwise: the invariant (a pixel
with n_p samples holds the steady accumulation after n_p spp, bit for bit), the decisions against the numpy restatement of the rule, the
oracle's per-sample colours, call and batch splits, extreme thresholds, ranks, crop windows, checkpoints, the refusal of transient
renders and the CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, image_metrics, record_metric
from adaptive_cases import rule_error
from adapt_amd.scene_pack import make_config

pytestmark = pytest.mark.gpu

BUILDS = ["fast", "exact"]
W, H = 48, 40
MIN_SPP, STEP, N = 8, 4, 32


def _parse_extra(tag):
    from adapt_amd.parsers import scene_parsing
    where = {"cbox_fog": ("vpt", "cbox_fog.xml"), "media_a": ("test", "media_a.xml")}[tag]
    cwd = os.getcwd(); os.chdir(ROOT)
    try:
        return scene_parsing(os.path.join(ROOT, "scenes", where[0]), where[1])
    finally:
        os.chdir(cwd)


@pytest.fixture
def scene(parsed):
    def get(tag):
        return _parse_extra(tag) if tag in ("cbox_fog", "media_a") else parsed(tag)
    return get


@pytest.fixture
def renderer():
    """factory: Renderer / VolumeRenderer(*scene, exact=..., **kw); closed when the test ends"""
    from adapt_amd.renderer import Renderer, VolumeRenderer
    made = []

    def make(scene_, build, volumetric=False, **kw):
        r = (VolumeRenderer if volumetric else Renderer)(*scene_, exact=(build == "exact"), **kw)
        made.append(r)
        return r
    yield make
    for r in made:
        r.close()


def state(r):
    n, act = r.tile_sample_counts(with_mask=True)
    return r.tile_accum(), r.tile_moments(), n, act


def pick_threshold(renderer, scene_, build, volumetric, **kw):
    """a threshold that retires some pixels at the first decision and leaves others active: the 40 % quantile of e_p at min_spp over
    the pixels whose samples differ (a pixel whose samples are all equal - black background, say - has e_p = 0 and retires at any threshold)"""
    probe = renderer(scene_, build, volumetric, adaptive={"threshold": 1e-30, "min_spp": MIN_SPP, "step": STEP}, **kw)
    probe.render(n_spp=MIN_SPP)
    e = probe.relative_error()
    probe.close()
    return float(np.quantile(e[np.isfinite(e) & (e > 0)], 0.4))


def steady_snapshots(renderer, scene_, build, volumetric, **kw):
    """the steady renderer's accumulation after every STEP spp, up to N"""
    r = renderer(scene_, build, volumetric, **kw)
    snaps = {0: np.zeros((r.n_cols, r.h, 3), np.float32)}
    for k in range(STEP, N + 1, STEP):
        r.render(n_spp=STEP)
        snaps[k] = r.tile_accum()
    return snaps, r


# ---------------------------------------------------------------- 1. + 2. the invariant and the decisions
# (tag, volumetric, crop window or None, APT_TRAVERSAL); c2_cbox runs the traced kernel in the product build, C3 the class groups with
# four light samples, the cbox window the BVH walk
INVARIANT_CASES = [("cbox", False, None, None), ("glass_box", False, None, None), ("balls_mono", False, None, None),
                   ("cbox", False, (10, 36, 6, 30), "bvh"), ("cbox_fog", True, None, None), ("media_a", True, None, None)]


def _with_crop(scene_, crop):
    if crop is None:
        return scene_
    em, arr, objs, cfg = scene_
    cfg = dict(cfg)
    x0, x1, y0, y1 = crop
    cfg["film"] = {"width": W, "height": H, "crop_x": (x0 + x1) // 2, "crop_y": (y0 + y1) // 2, "crop_rx": (x1 - x0) // 2, "crop_ry": (y1 - y0) // 2}
    return em, arr, objs, cfg


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("tag,volumetric,crop,traversal", INVARIANT_CASES)
def test_adaptive_pixels_hold_the_steady_accumulation(tag, volumetric, crop, traversal, build, renderer, scene, monkeypatch):
    if traversal:
        monkeypatch.setenv("APT_TRAVERSAL", traversal)
    sc = _with_crop(scene(tag), crop)
    kw = dict(width=W, height=H, spp_per_batch=3)
    thr = pick_threshold(renderer, sc, build, volumetric, **kw)
    ad = renderer(sc, build, volumetric, adaptive={"threshold": thr, "min_spp": MIN_SPP, "step": STEP}, **kw)
    assert ad.info()["sampling"] == "adaptive" and "[adaptive]" in ad.info()["shade_variant"]
    if traversal:
        assert ad.info()["traversal"] == traversal
    ad.render(n_spp=N)
    acc, s2, n, act = state(ad)
    snaps, steady = steady_snapshots(renderer, sc, build, volumetric, **kw)
    inside = ad._crop_mask()
    # some pixels retired, some still sample; an active pixel has every sample, a retired one a decision point's worth
    assert (inside & ~act).any() and act.any(), (thr, act.mean())
    assert np.all(n[act] == N) and np.all(n[~inside] == 0) and not act[~inside].any()
    assert set(np.unique(n[inside])) <= set(range(MIN_SPP, N + 1, STEP))
    for k in np.unique(n):
        sel = n == k
        assert np.array_equal(acc[sel].view(np.uint32), snaps[int(k)][sel].view(np.uint32)), (tag, build, int(k))
    assert ad.cnt[None] == N and ad.stats()["n_samples"] == int(n.sum())
    # pixels: each divided by its own count (0 where it has none); the active ones equal the steady image
    px = ad.pixels.to_numpy()
    assert np.array_equal(px[~inside], np.zeros_like(px[~inside]))
    assert np.array_equal(px[act], steady.pixels.to_numpy()[act])
    # 2. the decisions follow the numpy rule on every pixel (but those within 1e-9 of the threshold)
    e = rule_error(acc, s2, n)
    thr32 = np.float64(np.float32(thr))
    near = np.abs(e - thr32) <= 1e-9 * thr32
    want_retired = (n >= MIN_SPP) & (e <= thr32)
    assert np.array_equal((~act & inside)[~near], want_retired[~near]), (tag, build)
    assert not np.any(inside & ~act & (n < MIN_SPP))
    assert np.array_equal(np.isfinite(ad.relative_error()), np.isfinite(e))
    record_metric(f"adaptive_invariant[{tag},{build}]", {"threshold": thr, "active": float(act[inside].mean()), "mean_spp": float(n[inside].mean()), "near": int(near.sum())})


# ---------------------------------------------------------------- 3. against the oracle's per-sample colours (exact build)
@pytest.mark.parametrize("tag", ["cbox", "glass_box", "balls_mono"])
def test_adaptive_accumulation_matches_the_oracle_per_sample_colours(tag, renderer, parsed, oracle_scene):
    sc = parsed(tag)
    kw = dict(width=W, height=H)
    thr = pick_threshold(renderer, sc, "exact", False, **kw)
    ad = renderer(sc, "exact", adaptive={"threshold": thr, "min_spp": MIN_SPP, "step": STEP}, **kw)
    ad.render(n_spp=N)
    acc, _, n, act = state(ad)
    assert (~act).any() and act.any()
    rc = make_config(sc[3], width=W, height=H)
    _, per, _ = oracle_scene(tag).contributions(rc, N)
    col = np.nan_to_num(per[..., :3], nan=0.0).astype(np.float32)          # (w, h, N, 3): the steady colour of each sample
    ref = np.zeros((W, H, 3), np.float32)
    for s in range(N):                                                    # summed in sample order, up to each pixel's n_p
        ref = np.where((s < n)[..., None], ref + col[:, :, s], ref).astype(np.float32)
    nn = np.maximum(n, 1)[..., None].astype(np.float32)
    m = image_metrics(acc / nn, ref / nn)
    record_metric(f"adaptive_oracle[{tag}]", m)
    assert m["frac_within"] >= 0.995 and m["relMSE"] <= 1e-4, m


# ---------------------------------------------------------------- 4. call and batch splits
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("tag,volumetric", [("cbox", False), ("balls_mono", False), ("cbox_fog", True)])
def test_call_and_batch_splits_give_identical_state(tag, volumetric, build, renderer, scene):
    sc = scene(tag)
    thr = pick_threshold(renderer, sc, build, volumetric, width=W, height=H)
    ad = {"threshold": thr, "min_spp": MIN_SPP, "step": STEP}
    runs = []
    for spb, calls in ((0, [N + 3]), (2, [5, 11, 3, 1, 15]), (7, [9, 9, 17])):
        r = renderer(sc, build, volumetric, adaptive=ad, width=W, height=H, spp_per_batch=spb)
        for c in calls:
            r.render(n_spp=c)
        runs.append(state(r) + (r.stats()["n_samples"], r.cnt[None]))
        r.close()
    a = runs[0]
    assert (~a[3]).any() and a[3].any()
    for b in runs[1:]:
        for x, y in zip(a[:4], b[:4]):
            assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
        assert a[4:] == b[4:]


# ---------------------------------------------------------------- 5. extreme thresholds
@pytest.mark.parametrize("build", BUILDS)
def test_huge_threshold_stops_every_pixel_at_min_spp(build, renderer, parsed):
    sc = parsed("cbox")
    ad = renderer(sc, build, adaptive={"threshold": 1e30, "min_spp": MIN_SPP, "step": STEP}, width=W, height=H)
    ad.render(n_spp=N)
    n, act = ad.tile_sample_counts(with_mask=True)
    assert np.all(n == MIN_SPP) and not act.any() and ad.active_fraction() == 0.0
    steady = renderer(sc, build, width=W, height=H)
    steady.render(n_spp=MIN_SPP)
    assert np.array_equal(ad.color.to_numpy(), steady.color.to_numpy()) and np.array_equal(ad.pixels.to_numpy(), steady.pixels.to_numpy())
    before = ad.stats()
    ad.render(n_spp=2 * STEP + 1)                                        # nothing left to sample: no launch, cnt still advances
    after = ad.stats()
    assert after["n_samples"] == before["n_samples"] == W * H * MIN_SPP and ad.cnt[None] == N + 2 * STEP + 1
    assert after["launches"] == before["launches"]
    assert np.array_equal(ad.color.to_numpy(), steady.color.to_numpy())


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("tag,volumetric", [("cbox", False), ("cbox_fog", True)])
def test_tiny_threshold_is_the_steady_render(tag, volumetric, build, renderer, scene):
    sc = scene(tag)
    ad = renderer(sc, build, volumetric, adaptive={"threshold": 1e-30, "min_spp": MIN_SPP, "step": STEP}, width=W, height=H)
    ad.render(n_spp=N)
    steady = renderer(sc, build, volumetric, width=W, height=H)
    steady.render(n_spp=N)
    acc, s2, n, act = state(ad)
    # every pixel whose samples differ takes every sample and holds the steady accumulation; only pixels whose samples were all equal at
    # a decision (e_p = 0: black background, say) retire, as they do at any threshold
    e = rule_error(acc, s2, n)
    assert np.all(n[act] == N) and np.all(e[~act] == 0.0) and np.all(e[act] > 0.0) and act.mean() > 0.5, act.mean()
    sacc = steady.color.to_numpy()
    assert np.array_equal(acc[act].view(np.uint32), sacc[act].view(np.uint32))
    assert np.array_equal(ad.pixels.to_numpy()[act], steady.pixels.to_numpy()[act])
    assert ad.stats()["n_samples"] == int(n.sum()) and steady.stats()["n_samples"] == W * H * N


# ---------------------------------------------------------------- 6. ranks
@pytest.mark.parametrize("tag", ["cbox", "balls_mono"])
def test_four_ranks_assemble_to_one_rank(tag, renderer, parsed):
    from adapt_amd.tiles import TilePlan, assemble
    sc = parsed(tag)
    w, h = 64, 40
    thr = pick_threshold(renderer, sc, "fast", False, width=w, height=h)
    ad = {"threshold": thr, "min_spp": MIN_SPP, "step": STEP}
    one = renderer(sc, "fast", adaptive=ad, width=w, height=h)
    one.render(n_spp=N)
    acc, n = one.color.to_numpy(), one.sample_counts()
    assert (n < N).any() and (n == N).any()
    tiles, counts = [], []
    for rank in range(4):
        r = renderer(sc, "fast", adaptive=ad, width=w, height=h, rank=rank, world_size=4, band_width=8)
        r.render(n_spp=13); r.render(n_spp=N - 13)
        tiles.append(r.tile_accum()); counts.append(r.tile_sample_counts())
        r.close()
    plan = TilePlan(w, h, 8, 4)
    assert np.array_equal(assemble(plan, tiles).view(np.uint32), acc.view(np.uint32))
    assert np.array_equal(assemble(plan, counts), n)


# ---------------------------------------------------------------- 7. crop, checkpoints, refusal
@pytest.mark.parametrize("build", BUILDS)
def test_checkpoint_resume_equals_uninterrupted(build, renderer, parsed):
    sc = parsed("glass_box")
    thr = pick_threshold(renderer, sc, build, False, width=W, height=H)
    ad = {"threshold": thr, "min_spp": MIN_SPP, "step": STEP}
    a = renderer(sc, build, adaptive=ad, width=W, height=H)
    a.render(n_spp=14)                                                   # mid-round
    ck = a.get_check_point()
    assert {"sample_counts", "moments", "active", "adaptive"} <= set(ck) and ck["counter"] == 14
    a.render(n_spp=N - 14)
    b = renderer(sc, build, adaptive=ad, width=W, height=H)
    b.load_check_point(ck)
    assert b.cnt[None] == 14 and np.array_equal(b.sample_counts(), ck["sample_counts"])
    b.render(n_spp=N - 14)
    for x, y in zip(state(a), state(b)):
        assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
    # a steady renderer refuses the adaptive checkpoint, an adaptive renderer a steady one
    steady = renderer(sc, build, width=W, height=H)
    with pytest.raises(ValueError):
        steady.load_check_point(ck)
    steady.render(n_spp=4)
    with pytest.raises(ValueError):
        b.load_check_point(steady.get_check_point())
    with pytest.raises(RuntimeError):
        b.cnt[None] = 3


def test_crop_window_samples_inside_only(renderer, parsed):
    sc = _with_crop(parsed("cbox"), (8, 30, 4, 24))
    ad = renderer(sc, "fast", adaptive={"threshold": 1e-30, "min_spp": MIN_SPP, "step": STEP}, width=W, height=H)
    ad.render(n_spp=12)
    n = ad.sample_counts()
    inside = ad._crop_mask()
    assert np.all(n[inside] >= MIN_SPP) and np.all(n[~inside] == 0) and ad.stats()["n_samples"] == int(n.sum())
    assert not ad.color.to_numpy()[~inside].any() and not ad.pixels.to_numpy()[~inside].any()
    _, act = ad.tile_sample_counts(with_mask=True)
    assert not act[~inside].any() and ad.active_fraction() == act[inside].mean() > 0.5


def test_transient_with_adaptive_is_refused(renderer, parsed):
    from adapt_amd._lib import AptError
    sc = parsed("cbox")
    with pytest.raises(AptError, match="transient"):
        renderer(sc, "fast", transient={"sample_count": 4, "min_time": 0.0, "interval": 1.0}, adaptive={"threshold": 0.05}, width=16, height=16)


# ---------------------------------------------------------------- 8. CLI
def test_cli_writes_image_and_spp_map_of_a_direct_run(tmp_path, renderer, parsed):
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "render.py"), "--type", "pt", "--input_path", os.path.join(ROOT, "scenes"), "--scene", "cbox",
           "--name", "glass_box.xml", "--iter_num", str(N - 1), "--width", str(W), "--height", str(H), "--noise_threshold", "0.05",
           "--min_spp", str(MIN_SPP), "--adaptive_step", str(STEP), "--output_path", str(out) + os.sep, "--chkpt_path", str(tmp_path / "chk") + os.sep,
           "--no_gui", "--img_ext", "npy"]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "converged" in p.stdout and "mean spp" in p.stdout
    img = np.load(out / "pbr-glass_box-pt.npy")
    spp = np.load(out / "pbr-glass_box-pt-spp.npy")
    r = renderer(parsed("glass_box"), "fast", adaptive={"threshold": 0.05, "min_spp": MIN_SPP, "step": STEP}, width=W, height=H)
    r.render(n_spp=N)
    assert spp.dtype == np.int32 and np.array_equal(spp, r.sample_counts())
    assert np.array_equal(img, r.pixels.to_numpy())
