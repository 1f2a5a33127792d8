"""The camera vertex shaded by the kernel that traces the camera ray (csrc/shade_stage.hpp shade_traced CAM) on the device:
every render that takes the camera-fed launch (APT_CAMERA_FUSE=1, the default: steady full-film renders with rays traced in place) gives
the same accumulation and the same counters, bit for bit, as k_generate_trace + the queue-fed bounce 0 (APT_CAMERA_FUSE=0) - every bundled
scene, C1, a film of odd size, one rank of two, several render() calls over several lane-batches, one bounce, every ray through the
reference-order code.  Cropped and adaptive renders keep the two-launch form whatever the switch says."""
import os

import numpy as np
import pytest

from conftest import ALL_TAGS

pytestmark = pytest.mark.gpu

COUNTERS = ("n_samples", "n_extend", "n_shade", "n_shadow", "n_shadow_traced", "n_lit", "n_draws", "n_poisoned")


def _render(tup, fuse, w, h, spp, max_bounce=None, unsorted=False, calls=1, defer_all=False, **kw):
    """unsorted: APT_SORTED=0 and one light sample per vertex - the scenes of several material classes then take the traced kernels too.
    -> shade variant, the rank's accumulation, counters, per-pixel sample counts (adaptive renders; else None), camera_fused()"""
    from adapt_amd.renderer import Renderer
    env = {"APT_CAMERA_FUSE": str(fuse)}                # read at renderer creation
    if unsorted: env["APT_SORTED"] = "0"                # read at renderer creation
    if defer_all: env["APT_FLAT_DEFER_ALL"] = "1"       # read at scene creation
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        r = Renderer(*tup, width=w, height=h, exact=False, max_bounce=max_bounce, num_shadow_ray=1 if unsorted else None, **kw)
    finally:
        for k, v in old.items():
            if v is None: os.environ.pop(k)
            else: os.environ[k] = v
    try:
        for _ in range(calls):
            r.render(n_spp=spp)
        counts = r.tile_sample_counts().copy() if kw.get("adaptive") else None
        return r.info()["shade_variant"], r.tile_accum().copy(), r.stats(), counts, r.camera_fused()
    finally:
        r.close()


def _same(a, b, what, fused=True):
    """a: APT_CAMERA_FUSE=1, b: =0.  fused: whether a is expected to have taken the camera-fed launch (b never does)"""
    name1, acc1, st1, n1, f1 = a
    name0, acc0, st0, n0, f0 = b
    assert name0 == name1
    assert f1 is fused and f0 is False, (what, f1, f0)
    assert np.array_equal(acc0.view(np.uint32), acc1.view(np.uint32)), (what, float(np.nanmax(np.abs(acc0 - acc1))))
    for k in COUNTERS:
        assert st0[k] == st1[k], (what, k, st0[k], st1[k])
    if n1 is not None: assert np.array_equal(n0, n1), what
    # the fused form launches no generate kernel; the two-launch form one per lane-batch
    assert (st1["launches"]["generate"] == 0) is fused and st0["launches"]["generate"] > 0, (what, st1["launches"], st0["launches"])


@pytest.mark.parametrize("unsorted", [False, True])
def test_camera_fuse_leaves_every_traced_scene_bit_identical(parsed, unsorted):
    traced = []
    for tag in ALL_TAGS:
        tup = parsed(tag)
        on = _render(tup, 1, 64, 64, 8, unsorted=unsorted)
        if "[rays traced in place]" not in on[0]:
            assert on[4] is False, tag                  # nothing to fuse outside the traced path
            continue
        _same(on, _render(tup, 0, 64, 64, 8, unsorted=unsorted), tag)
        assert on[2]["n_extend"] > 0 and on[2]["n_shade"] > 0, tag
        traced.append(tag)
    assert "cbox" in traced, traced
    if unsorted: assert len(traced) > 1, traced         # (by default only the Cornell box takes the traced kernels)


def test_camera_fuse_leaves_c1_bit_identical(parsed):
    """C1: the Cornell box at 256 x 256, 4 bounces (bench.py's c1), with more samples per pixel"""
    tup = parsed("cbox")
    on = _render(tup, 1, 256, 256, 16, max_bounce=4)
    assert "[rays traced in place]" in on[0]
    _same(on, _render(tup, 0, 256, 256, 16, max_bounce=4), "c1")


def test_camera_fuse_leaves_a_film_of_odd_size_bit_identical(parsed):
    """npix = 50 x 30 = 1500 is not a multiple of 64: a wave's rays straddle strips and wrap from one sample into the next, and the last wave
    of the id space is partly empty"""
    tup = parsed("cbox")
    on = _render(tup, 1, 50, 30, 24)
    assert "[rays traced in place]" in on[0]
    assert on[2]["n_samples"] == 50 * 30 * 24
    _same(on, _render(tup, 0, 50, 30, 24), "50x30")


def test_camera_fuse_leaves_one_rank_of_two_bit_identical(parsed):
    """world_size = 2, rank 1 with bench.py's band width, on one device: the rank's local pixels are every other band of four columns"""
    tup = parsed("cbox")
    kw = dict(rank=1, world_size=2, band_width=4)
    on = _render(tup, 1, 128, 64, 16, **kw)
    assert "[rays traced in place]" in on[0]
    assert on[1].shape[0] == 64                         # the rank's columns
    _same(on, _render(tup, 0, 128, 64, 16, **kw), "rank 1 of 2")


def test_camera_fuse_leaves_consecutive_renders_bit_identical(parsed):
    """three render() calls of 200 spp: each is split into several lane-batches (the sample counter and the counters' rotation carry over
    from batch to batch and from call to call)"""
    tup = parsed("cbox")
    on = _render(tup, 1, 96, 80, 200, calls=3)
    assert "[rays traced in place]" in on[0]
    assert on[2]["n_samples"] == 96 * 80 * 600
    assert on[2]["launches"]["finalize"] >= 6           # several lane-batches per call
    _same(on, _render(tup, 0, 96, 80, 200, calls=3), "3 x 200 spp")


def test_camera_fuse_leaves_a_one_bounce_render_bit_identical(parsed):
    """max_bounce = 1: the camera-fed launch is the only bounce (no continuation ray, the light samples it defers go to the closing fix-up)"""
    tup = parsed("cbox")
    on = _render(tup, 1, 64, 64, 16, max_bounce=1)
    assert "[rays traced in place]" in on[0]
    _same(on, _render(tup, 0, 64, 64, 16, max_bounce=1), "max_bounce=1")


def test_camera_fuse_with_every_ray_through_the_reference_order_code(parsed):
    """APT_FLAT_DEFER_ALL=1: the camera-fed launch stages every camera ray, the bounce-0 launch behind it resolves and shades them all, and
    every continuation ray and light sample goes through the lists as well: same image, same counters, sample count exact"""
    tup = parsed("cbox")
    on = _render(tup, 1, 64, 48, 12, defer_all=True)
    assert "[rays traced in place]" in on[0]
    assert on[2]["n_samples"] == 64 * 48 * 12
    _same(on, _render(tup, 0, 64, 48, 12, defer_all=True), "defer all")
    plain = _render(tup, 1, 64, 48, 12)
    assert plain[2]["n_samples"] == on[2]["n_samples"]


def test_a_cropped_render_keeps_the_two_launch_form(parsed):
    emitters, arrays, objects, cfg = parsed("cbox")
    cfg = dict(cfg); cfg["film"] = {"width": 128, "height": 128, "crop_x": 70, "crop_y": 40, "crop_rx": 30, "crop_ry": 20}
    tup = (emitters, arrays, objects, cfg)
    on = _render(tup, 1, None, None, 16)
    assert "[rays traced in place]" in on[0]
    assert on[2]["n_samples"] == 60 * 40 * 16
    _same(on, _render(tup, 0, None, None, 16), "crop", fused=False)


def test_an_adaptive_render_keeps_the_two_launch_form(parsed):
    tup = parsed("cbox")
    ad = {"threshold": 0.05, "min_spp": 8, "step": 4}
    on = _render(tup, 1, 64, 64, 12, calls=4, adaptive=ad)
    assert "[rays traced in place]" in on[0] and "[adaptive]" in on[0]
    _same(on, _render(tup, 0, 64, 64, 12, calls=4, adaptive=ad), "adaptive", fused=False)
