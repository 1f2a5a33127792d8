"""The camera vertex shaded by the kernel that traces the camera ray (csrc/shade_stage.hpp shade_traced CAM) on the device:
every render that takes the camera-fed launch (APT_CAMERA_FUSE=1, the default: steady full-film renders with rays traced in place) gives
the same accumulation and the same counters, bit for bit, as k_generate_trace + the queue-fed bounce 0 (APT_CAMERA_FUSE=0) - every bundled
scene, C1, a film of odd size, one rank of two, several render() calls over several lane-batches, one bounce, every ray through the
reference-order code.  Cropped and adaptive renders keep the two-launch form whatever the switch says."""
import pytest

from gpu_ab import assert_same_run, render_run, traced_pairs

pytestmark = pytest.mark.gpu

ON, OFF = {"APT_CAMERA_FUSE": "1"}, {"APT_CAMERA_FUSE": "0"}


def _same(a, b, what, fused=True):
    """a: APT_CAMERA_FUSE=1, b: =0.  fused: whether a is expected to have taken the camera-fed launch (b never does)"""
    assert a.fused is fused and b.fused is False, (what, a.fused, b.fused)
    assert_same_run(a, b, what)
    # the fused form launches no generate kernel; the two-launch form one per lane-batch
    la, lb = a.stats["launches"], b.stats["launches"]
    assert (la["generate"] == 0) is fused and lb["generate"] > 0, (what, la, lb)


@pytest.mark.parametrize("unsorted", [False, True])
def test_camera_fuse_leaves_every_traced_scene_bit_identical(parsed, unsorted):
    def untraced(tag, on):
        assert on.fused is False, tag                   # nothing to fuse outside the traced path
    for tag, on, _ in traced_pairs(parsed, unsorted, ON, OFF, same=_same, untraced=untraced):
        assert on.stats["n_extend"] > 0 and on.stats["n_shade"] > 0, tag


def test_camera_fuse_leaves_c1_bit_identical(parsed):
    """C1: the Cornell box at 256 x 256, 4 bounces (bench.py's c1), with more samples per pixel"""
    tup = parsed("cbox")
    on = render_run(tup, 256, 256, 16, max_bounce=4, env=ON)
    assert on.traced
    _same(on, render_run(tup, 256, 256, 16, max_bounce=4, env=OFF), "c1")


def test_camera_fuse_leaves_a_film_of_odd_size_bit_identical(parsed):
    """npix = 50 x 30 = 1500 is not a multiple of 64: a wave's rays straddle strips and wrap from one sample into the next, and the last wave
    of the id space is partly empty"""
    tup = parsed("cbox")
    on = render_run(tup, 50, 30, 24, env=ON)
    assert on.traced
    assert on.stats["n_samples"] == 50 * 30 * 24
    _same(on, render_run(tup, 50, 30, 24, env=OFF), "50x30")


def test_camera_fuse_leaves_one_rank_of_two_bit_identical(parsed):
    """world_size = 2, rank 1 with bench.py's band width, on one device: the rank's local pixels are every other band of four columns"""
    tup = parsed("cbox")
    kw = dict(rank=1, world_size=2, band_width=4)
    on = render_run(tup, 128, 64, 16, env=ON, **kw)
    assert on.traced
    assert on.accum.shape[0] == 64                      # the rank's columns
    _same(on, render_run(tup, 128, 64, 16, env=OFF, **kw), "rank 1 of 2")


def test_camera_fuse_leaves_consecutive_renders_bit_identical(parsed):
    """three render() calls of 200 spp: each is split into several lane-batches (the sample counter and the counters' rotation carry over
    from batch to batch and from call to call)"""
    tup = parsed("cbox")
    on = render_run(tup, 96, 80, 200, calls=3, env=ON)
    assert on.traced
    assert on.stats["n_samples"] == 96 * 80 * 600
    assert on.stats["launches"]["finalize"] >= 6        # several lane-batches per call
    _same(on, render_run(tup, 96, 80, 200, calls=3, env=OFF), "3 x 200 spp")


def test_camera_fuse_leaves_a_one_bounce_render_bit_identical(parsed):
    """max_bounce = 1: the camera-fed launch is the only bounce (no continuation ray, the light samples it defers go to the closing fix-up)"""
    tup = parsed("cbox")
    on = render_run(tup, 64, 64, 16, max_bounce=1, env=ON)
    assert on.traced
    _same(on, render_run(tup, 64, 64, 16, max_bounce=1, env=OFF), "max_bounce=1")


def test_camera_fuse_with_every_ray_through_the_reference_order_code(parsed):
    """APT_FLAT_DEFER_ALL=1: the camera-fed launch stages every camera ray, the bounce-0 launch behind it resolves and shades them all, and
    every continuation ray and light sample goes through the lists as well: same image, same counters, sample count exact"""
    tup = parsed("cbox")
    on = render_run(tup, 64, 48, 12, env=dict(ON, APT_FLAT_DEFER_ALL="1"))
    assert on.traced
    assert on.stats["n_samples"] == 64 * 48 * 12
    _same(on, render_run(tup, 64, 48, 12, env=dict(OFF, APT_FLAT_DEFER_ALL="1")), "defer all")
    plain = render_run(tup, 64, 48, 12, env=ON)
    assert plain.stats["n_samples"] == on.stats["n_samples"]


def test_a_cropped_render_keeps_the_two_launch_form(parsed):
    *scene, cfg = parsed("cbox")
    tup = (*scene, dict(cfg, film={"width": 128, "height": 128, "crop_x": 70, "crop_y": 40, "crop_rx": 30, "crop_ry": 20}))
    on = render_run(tup, None, None, 16, env=ON)
    assert on.traced
    assert on.stats["n_samples"] == 60 * 40 * 16
    _same(on, render_run(tup, None, None, 16, env=OFF), "crop", fused=False)


def test_an_adaptive_render_keeps_the_two_launch_form(parsed):
    tup = parsed("cbox")
    ad = {"threshold": 0.05, "min_spp": 8, "step": 4}
    on = render_run(tup, 64, 64, 12, calls=4, adaptive=ad, env=ON)
    assert on.traced and "[adaptive]" in on.variant
    _same(on, render_run(tup, 64, 64, 12, calls=4, adaptive=ad, env=OFF), "adaptive", fused=False)
