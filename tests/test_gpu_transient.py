"""Transient (time-resolved) rendering on the device (DESIGN.md "Transient rendering"), on both builds of the library unless a case
says otherwise: the bins against the steady image, the fast and exact arrivals of direct light, ior weighting, the time window,
determinism, checkpoints and the CLI export."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, image_metrics, record_metric
from transient_cases import _direct_light_scene, _predicted_times
from adapt_amd.scene_pack import make_config

pytestmark = pytest.mark.gpu

BUILDS = ["fast", "exact"]
ALL_TIME = {"sample_count": 1, "min_time": -1.0, "interval": 1e6}      # one bin that holds every path


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


# ---------------------------------------------------------------- 1. the bins sum to the steady image
SUM_CASES = [("cbox", None), ("balls_mono", None), ("glass_box", None), ("cbox", "bvh")]


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("tag,traversal", SUM_CASES)
def test_bins_sum_to_steady_image(tag, traversal, build, renderer, parsed, monkeypatch):
    if traversal:
        monkeypatch.setenv("APT_TRAVERSAL", traversal)
    scene = parsed(tag)
    kw = dict(width=64, height=64, spp_per_batch=8)
    steady = renderer(scene, build, **kw)
    steady.render(n_spp=16)
    img = steady.color.to_numpy()
    tr = renderer(scene, build, transient=ALL_TIME, **kw)
    assert "[transient]" in tr.info()["shade_variant"]
    if traversal:
        assert tr.info()["traversal"] == traversal and steady.info()["traversal"] == traversal
    tr.render(n_spp=16)
    cube, counts = tr.transient(), tr.transient_counts()
    assert cube.shape == (1, 64, 64, 3) and counts.shape == (1, 64, 64)
    st, sst = tr.stats(), steady.stats()
    for k in ("n_samples", "n_shade", "n_shadow", "n_draws", "n_poisoned"):      # the same random stream, the same paths
        assert st[k] == sst[k], (k, st[k], sst[k])
    a, b = cube[0].astype(np.float64) * 16, img.astype(np.float64)
    fin = np.isfinite(b).all(axis=2)
    err = np.where(np.abs(a - b) <= 1e-12, 0.0, np.abs(a - b) / np.maximum(np.abs(b), 1e-30)).max(axis=2)
    # A pixel-sample whose light sample has a NaN MIS weight is dropped whole by the steady renderer (stages.hpp k_finalize); the bins drop
    # only that contribution (DESIGN.md "Transient rendering"): such pixels keep more energy in the bins, at most one pixel per poisoned vertex.
    poisoned = fin & (err > 1e-5)
    record_metric(f"transient_sum_vs_steady[{tag},{traversal},{build}]", {"max_rel": float(err[fin & ~poisoned].max()), "pixels": int(fin.sum()),
                                                                          "poisoned_pixels": int(poisoned.sum()), "n_poisoned": st["n_poisoned"]})
    assert err[fin & ~poisoned].max() <= 1e-5
    assert poisoned.sum() <= st["n_poisoned"] and np.all(a[poisoned].sum(-1) > b[poisoned].sum(-1))
    # the transient renderer's own framebuffer is the same sum, bounce by bounce
    c = tr.color.to_numpy().astype(np.float64)
    assert np.all(np.abs(c - a)[fin] <= 1e-5 * np.abs(a)[fin] + 1e-12)
    # counts: integral, and zero exactly where nothing arrived
    assert np.array_equal(counts, np.round(counts)) and counts.max() <= 16 * (1 + tr.num_shadow_ray) * tr.max_bounce
    assert np.array_equal(counts[0] > 0, np.any(cube[0] != 0, axis=2))
    # a steady renderer made after the transient one renders today's image bit for bit
    again = renderer(scene, build, **kw)
    again.render(n_spp=16)
    assert np.array_equal(again.color.to_numpy(), img, equal_nan=True)


# ---------------------------------------------------------------- 2. exact build against the oracle
@pytest.mark.parametrize("tag", ["cbox", "balls_mono"])
def test_exact_bins_match_oracle_same_stream(tag, renderer, parsed, oracle_scene):
    w, h, spp = 64, 48, 16
    r = renderer(parsed(tag), "exact", width=w, height=h, transient=ALL_TIME, spp_per_batch=8)
    r.render(n_spp=spp)
    steady = renderer(parsed(tag), "exact", width=w, height=h, spp_per_batch=8)
    steady.render(n_spp=spp)
    ref, _, _ = oracle_scene(tag).render(make_config(parsed(tag)[3], width=w, height=h), spp)
    a, b = r.transient()[0], steady.pixels.to_numpy()
    # pixels with a poisoned pixel-sample (see test_bins_sum_to_steady_image) are left out: there the steady image is the oracle's
    poisoned = np.any(np.abs(a - b) > 1e-5 * np.abs(b) + 1e-12, axis=2)
    assert poisoned.sum() <= r.stats()["n_poisoned"]
    m = image_metrics(a[~poisoned][:, None], (ref / spp)[~poisoned][:, None])
    record_metric(f"transient_exact_vs_oracle[{tag}]", {**m, "poisoned_pixels": int(poisoned.sum())})
    assert m["frac_within"] >= 0.995 and m["relMSE"] <= 1e-4, m


# ---------------------------------------------------------------- 3./4. analytic arrival times of direct light
def _check_arrivals(cube, t_pred, lo, step, name):
    """every pixel's energy in the bin of its predicted time; the neighbour only within 1e-4 * interval of an edge"""
    n = cube.shape[0]
    energy = cube.sum(-1)                                    # (n, W, H)
    lit = energy.sum(0) > 0
    x = (t_pred - lo) / step
    b = np.floor(x).astype(np.int64)
    frac = x - b
    ok = np.zeros_like(energy, dtype=bool)
    W, H = t_pred.shape
    ii, jj = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
    for k, allow in ((b, np.ones_like(lit)), (b - 1, frac < 1e-4), (b + 1, 1.0 - frac < 1e-4)):
        m = allow & (k >= 0) & (k < n)
        ok[k[m], ii[m], jj[m]] = True
    stray = np.where(ok, 0.0, energy)
    near_edge = np.minimum(frac, 1 - frac)[lit]
    record_metric(name, {"lit_pixels": int(lit.sum()), "stray_energy": float(stray.sum()), "min_edge_distance_bins": float(near_edge.min())})
    assert lit.mean() > 0.9, lit.mean()
    assert stray.sum() == 0.0, np.argwhere(stray > 0)[:5]
    return lit, b


@pytest.mark.parametrize("build", BUILDS)
def test_direct_light_arrives_at_predicted_time(build, renderer):
    w = h = 48
    lo, step, n = 5.0, 1.0, 40
    scene = _direct_light_scene(w, h, slab=False)
    r = renderer(scene, build, width=w, height=h, transient={"sample_count": n, "min_time": lo, "interval": step}, spp_per_batch=4)
    r.render(n_spp=4)
    rc = make_config(scene[3], width=w, height=h)
    t, _ = _predicted_times(rc, (2.78, 2.73, 6.0), slab=False)
    _check_arrivals(r.transient(), t, lo, step, f"transient_direct_arrival[{build}]")


@pytest.mark.parametrize("build", BUILDS)
def test_glass_slab_delays_by_half_the_inslab_length(build, renderer):
    """ior 1.5: the path through the slab arrives 0.5 x (in-slab length) later than its geometric length; a renderer that took the
    slab's ior as 1 puts most pixels' energy into another bin (the slab is 5 bins thick)"""
    w = h = 48
    lo, step, n = 5.0, 1.0, 40
    scene = _direct_light_scene(w, h, slab=True)
    r = renderer(scene, build, width=w, height=h, transient={"sample_count": n, "min_time": lo, "interval": step}, spp_per_batch=4)
    r.render(n_spp=4)
    rc = make_config(scene[3], width=w, height=h)
    t_ior, t_geo = _predicted_times(rc, (2.78, 2.73, 6.0), slab=True)
    lit, b = _check_arrivals(r.transient(), t_ior, lo, step, f"transient_slab_arrival[{build}]")
    b_geo = np.floor((t_geo - lo) / step).astype(np.int64)
    assert np.mean(b_geo[lit] != b[lit]) > 0.9


# ---------------------------------------------------------------- 5. window, determinism, batch split, crop, checkpoint
@pytest.mark.parametrize("build", BUILDS)
def test_bin_width_halving_sums_in_pairs(build, renderer, parsed):
    scene, kw = parsed("cbox"), dict(width=64, height=64, spp_per_batch=4)
    a = renderer(scene, build, transient={"sample_count": 40, "min_time": 11.0, "interval": 0.5}, **kw)
    b = renderer(scene, build, transient={"sample_count": 80, "min_time": 11.0, "interval": 0.25}, **kw)
    a.render(n_spp=4); b.render(n_spp=4)
    ca, cb = a.transient(), b.transient()
    pairs = cb[0::2] + cb[1::2]
    diff = np.abs(ca - pairs) / (1 + np.abs(ca))
    record_metric(f"transient_halving[{build}]", {"max_diff": float(diff.max())})
    assert diff.max() <= 1e-6
    assert np.array_equal(a.transient_counts(), b.transient_counts()[0::2] + b.transient_counts()[1::2])


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("tag", ["cbox", "balls_mono"])
def test_runs_are_bit_identical_and_batch_splits_agree(tag, build, renderer, parsed):
    scene, tw = parsed(tag), {"sample_count": 60, "min_time": 11.0, "interval": 0.25}
    a = renderer(scene, build, width=48, height=48, spp_per_batch=4, transient=tw)
    b = renderer(scene, build, width=48, height=48, spp_per_batch=4, transient=tw)
    c = renderer(scene, build, width=48, height=48, spp_per_batch=3, transient=tw)
    a.render(n_spp=8); b.render(n_spp=8); c.render(n_spp=5); c.render(n_spp=3)
    assert np.array_equal(a.tile_transient(), b.tile_transient())
    diff = np.abs(c.transient() - a.transient()) / (1 + np.abs(a.transient()))
    record_metric(f"transient_batch_split[{tag},{build}]", {"max_diff": float(diff.max())})
    assert diff.max() <= 1e-6
    assert np.array_equal(c.transient_counts(), a.transient_counts())


@pytest.mark.parametrize("build", BUILDS)
def test_crop_and_checkpoint(build, renderer, parsed):
    emitters, arrays, objects, prop = parsed("cbox")
    tw, kw = {"sample_count": 50, "min_time": 11.0, "interval": 0.2}, dict(width=64, height=64, spp_per_batch=4)
    full = renderer(parsed("cbox"), build, transient=tw, **kw)
    full.render(n_spp=4)
    cprop = dict(prop, film=dict(prop["film"], crop_x=30, crop_y=20, crop_rx=10, crop_ry=8))
    crop = renderer((emitters, arrays, objects, cprop), build, transient=tw, **kw)
    crop.render(n_spp=4)
    sx, ex, sy, ey = crop.start_x, crop.end_x, crop.start_y, crop.end_y
    cc, cf = crop.transient(), full.transient()
    assert (sx, ex, sy, ey) == (20, 40, 12, 28) and cc.shape == cf.shape
    assert np.array_equal(cc[:, sx:ex, sy:ey], cf[:, sx:ex, sy:ey])
    outside = np.ones(cc.shape[1:3], bool); outside[sx:ex, sy:ey] = False
    assert not cc[:, outside].any() and not crop.transient_counts()[:, outside].any() and cf[:, outside].any()
    # checkpoint: the bins travel with the accumulation and the counter
    cp = full.get_check_point()
    assert cp["transient_bins"].shape == (50, 64, 64, 4)
    back = renderer(parsed("cbox"), build, transient=tw, **kw)
    back.load_check_point(cp)
    assert back.cnt[None] == 4 and np.array_equal(back.tile_transient(), full.tile_transient())
    full.render(n_spp=4); back.render(n_spp=4)
    assert np.array_equal(back.tile_transient(), full.tile_transient())
    full.clear()
    assert not full.tile_transient().any() and full.cnt[None] == 0


def test_refused_configurations(renderer, parsed):
    from adapt_amd import _lib
    from adapt_amd.renderer import VolumeRenderer
    with pytest.raises(_lib.AptError, match="at most 4 light samples"):
        renderer(parsed("cbox"), "fast", width=16, height=16, num_shadow_ray=5, transient=ALL_TIME)
    with pytest.raises(_lib.AptError, match="surface-renderer"):
        VolumeRenderer(*parsed("cbox"), width=16, height=16, transient=ALL_TIME)
    with pytest.raises(_lib.AptError, match="one rank"):
        renderer(parsed("cbox"), "fast", width=16, height=16, world_size=2, rank=0, transient=ALL_TIME)
    steady = renderer(parsed("cbox"), "fast", width=16, height=16)
    with pytest.raises(RuntimeError):
        steady.transient()


# ---------------------------------------------------------------- 6. CLI end to end
def test_cli_writes_frames_and_cube(tmp_path, renderer):
    from adapt_amd.parsers import scene_parsing
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "render.py"), "--type", "pt", "--transient", "--input_path", os.path.join(ROOT, "scenes"),
           "--scene", "cbox", "--name", "transient_cbox.xml", "--iter_num", "3", "--width", "64", "--height", "64", "--spp_per_batch", "4",
           "--output_path", str(out) + os.sep, "--chkpt_path", str(tmp_path / "chk") + os.sep, "--no_gui", "--img_ext", "png"]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    folder = out / "transient_cbox"
    frames = sorted(f for f in os.listdir(folder) if f.startswith("img_") and f.endswith(".png"))
    assert len(frames) == 400 and frames[0] == "img_001.png" and frames[-1] == "img_400.png"
    cube = np.load(folder / "transient.npy")
    r = renderer(scene_parsing(os.path.join(ROOT, "scenes", "cbox"), "transient_cbox.xml"), "fast", width=64, height=64, spp_per_batch=4,
                 transient=True)
    r.render(n_spp=4)
    assert cube.shape == (400, 64, 64, 3) and np.array_equal(cube, r.transient())
    assert cube.any()
