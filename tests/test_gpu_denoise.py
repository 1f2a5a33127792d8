"""The denoiser on the device, both builds: the firefly filter against its float32 model, the a-trous filter against
the float64 model on the device's own read-back inputs, run-to-run identity, and the command line end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest

import denoise_model as dm
from conftest import ROOT, image_metrics, record_metric

pytestmark = pytest.mark.gpu

BUILDS = ["fast", "exact"]
FILMS = [(64, 48), (50, 30)]


@pytest.fixture
def renderer():
    from adapt_amd.renderer import Renderer
    made = []

    def make(scene, build, **kw):
        r = Renderer(*scene, exact=(build == "exact"), **kw)
        made.append(r)
        return r
    yield make
    for r in made:
        r.close()


# ---------------------------------------------------------------- 6. firefly filter
@pytest.mark.parametrize("build", BUILDS)
def test_firefly_filter_matches_the_model(build, renderer, parsed):
    """A rendered glass_box frame with a planted 1e4 pixel, the same frame with non-finite components, and the renderer's own pixels:
    every output pixel equals the float32 model's, bit for bit, except where a neighbour's distance lies within 1e-6 of the threshold
    (relative) - there the verdict may fall either way; those pixels are counted, at most 3."""
    w, h, thr = 50, 30, 0.4
    r = renderer(parsed("glass_box"), build, width=w, height=h)
    r.render(n_spp=8)
    base = r.pixels.to_numpy()
    planted = np.where(np.isfinite(base), base, np.float32(0)); planted[20, 17] = 1e4; planted[0, 29] = 1e4          # (one inside, one in a corner)
    broken = planted.copy(); broken[5, 5, 1] = np.inf; broken[6, 7] = np.nan; broken[49, 0, 2] = -np.inf
    for name, img in (("planted", planted), ("non-finite", broken), ("pixels", None)):
        got = r.firefly_filtered(thr, colour=img)
        want, keep, margin = dm.firefly(base if img is None else img, thr, with_margin=True)
        close = margin < 1e-6 * thr
        differ = np.any(got != want, axis=2)
        record_metric(f"firefly_vs_model[{name},{build}]", {"replaced": int((~keep).sum()), "near_threshold": int(close.sum()), "differ": int(differ.sum())})
        assert got.shape == (w, h, 3) and np.isfinite(got).all()
        assert not (differ & ~close).any(), np.argwhere(differ & ~close)[:5]
        assert close.sum() <= 3
        assert (~keep).sum() > 0                                       # some pixel was replaced ...
        assert np.array_equal(got[~keep & ~close], want[~keep & ~close])          # ... by the model's value, bit for bit
        if img is not None:
            assert not keep[20, 17] and not keep[0, 29] and got[20, 17].max() < 100
    assert np.array_equal(r.firefly_filtered(thr, colour=planted), r.firefly_filtered(thr, colour=planted))


# ---------------------------------------------------------------- 7. a-trous filter
ATROUS_CASES = {"defaults": {}, "K=1": {"iterations": 1}, "K=5": {"iterations": 5}, "no colour term": {"sigma_c": 0.0}, "sigma_c<0": {"sigma_c": -1.0},
                "no demodulation": {"demodulate": False}, "with firefly stage": {"firefly_threshold": 0.4}}


def _hold_to_model(r, cfg, window, label):
    """the device's denoised frame against the float64 model on the device's own pixels and guides: SURVEY 8(d)'s image criterion
    (every pass is a convex combination of its input: float32 rounding does not grow), and two runs bit-identical"""
    pixels, aov = r.pixels.to_numpy(), r.aov()
    got = r.denoised(**cfg)
    want = dm.denoise(pixels, aov, window=window, **cfg)
    m = image_metrics(got, want)
    record_metric(f"atrous_vs_model[{label}]", m)
    assert got.shape == pixels.shape and np.isfinite(got).all()
    assert m["frac_within"] >= 0.99 and m["relMSE"] <= 1e-4, (label, m)
    assert np.array_equal(got, r.denoised(**cfg)), label
    return got, pixels


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("film", FILMS, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("tag", ["cbox", "textured"])
def test_atrous_filter_matches_the_float64_model(tag, film, build, renderer, parsed):
    w, h = film
    r = renderer(parsed(tag), build, width=w, height=h)
    r.render(n_spp=16)
    for name, cfg in ATROUS_CASES.items():
        got, pixels = _hold_to_model(r, cfg, None, f"{tag},{w}x{h},{build},{name}")
        assert np.abs(got - pixels).max() > 1e-3                       # (the filter did something)
    assert np.array_equal(r.denoised(sigma_c=0.0), r.denoised(sigma_c=-1.0))


@pytest.mark.parametrize("build", BUILDS)
def test_atrous_filter_on_a_crop_window_and_a_tiny_film(build, renderer, parsed):
    em, arr, objs, prop = parsed("cbox")
    crop_prop = dict(prop); crop_prop["film"] = {"width": 50, "height": 30, "crop_x": 24, "crop_y": 14, "crop_rx": 9, "crop_ry": 6}
    r = renderer((em, arr, objs, crop_prop), build)
    assert r.do_crop
    r.render(n_spp=16)
    window = (r.start_x, r.end_x, r.start_y, r.end_y)
    inside = np.zeros((r.w, r.h), bool); inside[window[0]:window[1], window[2]:window[3]] = True
    for name, cfg in (("defaults", {}), ("K=1", {"iterations": 1})):
        got, pixels = _hold_to_model(r, cfg, window, f"cbox,crop,{build},{name}")
        assert not got[~inside].any() and np.abs(got - pixels)[inside].max() > 1e-3
    tiny = renderer(parsed("cbox"), build, width=3, height=2)       # every tap beyond the first ring falls outside
    tiny.render(n_spp=16)
    for name, cfg in (("defaults", {}), ("no colour term", {"sigma_c": 0.0})):
        _hold_to_model(tiny, cfg, None, f"cbox,3x2,{build},{name}")


# ---------------------------------------------------------------- 9. command line
def test_cli_writes_the_denoised_frame_and_the_feature_buffers(tmp_path, renderer, parsed):
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "render.py"), "--type", "pt", "--denoise", "--save_aov", "--firefly_threshold", "0.4",
           "--input_path", os.path.join(ROOT, "scenes"), "--scene", "cbox", "--name", "c2_cbox.xml", "--iter_num", "2", "--width", "64", "--height", "64",
           "--output_path", str(out) + os.sep, "--chkpt_path", str(tmp_path / "chk") + os.sep, "--no_gui", "--img_ext", "npy", "--img_name", "t"]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    for f in ("t-c2_cbox-pt.npy", "t-c2_cbox-pt-denoised.npy", "t-c2_cbox-pt-aov.npz"):
        assert (out / f).exists(), (f, os.listdir(out))
    r = renderer(parsed("cbox"), "fast", width=64, height=64)
    r.render(n_spp=3)
    assert np.array_equal(np.load(out / "t-c2_cbox-pt.npy"), r.pixels.to_numpy(), equal_nan=True)
    assert np.array_equal(np.load(out / "t-c2_cbox-pt-denoised.npy"), r.denoised(firefly_threshold=0.4))
    aov, mine = np.load(out / "t-c2_cbox-pt-aov.npz"), r.aov()
    assert set(aov.files) == set(mine) and all(np.array_equal(aov[k], mine[k]) for k in mine)
    # --denoise is a surface-renderer switch
    p = subprocess.run(cmd[:2] + ["--type", "vpt", "--denoise", "--no_gui"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 2 and "--type pt" in p.stderr
