"""Strip lists of the camera rays (csrc/flat_build.cpp camera_strips) on the device: every bundled scene that the product
build renders with rays traced in place (stages.hpp k_generate_trace) gives the same accumulation and the same counters, bit for bit,
with the lists (APT_CAMERA_CULL=1, the default) and with the full stream for every strip (APT_CAMERA_CULL=0) - also cropped, adaptive,
and as one rank of two."""
import pytest

from gpu_ab import assert_same_run, render_run, traced_pairs

pytestmark = pytest.mark.gpu

ON, OFF = {"APT_CAMERA_CULL": "1"}, {"APT_CAMERA_CULL": "0"}


@pytest.mark.parametrize("unsorted", [False, True])
def test_strip_lists_leave_every_traced_scene_bit_identical(parsed, unsorted):
    for tag, on, _ in traced_pairs(parsed, unsorted, ON, OFF):
        assert on.stats["n_extend"] > 0 and on.stats["n_shade"] > 0, tag


def test_strip_lists_leave_c1_bit_identical(parsed):
    """C1: the Cornell box at 256 x 256, 4 bounces (bench.py's c1), with more samples per pixel"""
    tup = parsed("cbox")
    on = render_run(tup, 256, 256, 16, max_bounce=4, env=ON)
    assert on.traced
    assert_same_run(on, render_run(tup, 256, 256, 16, max_bounce=4, env=OFF), "c1")


def test_strip_lists_leave_a_film_of_odd_size_bit_identical(parsed):
    """npix = 50 x 30 = 1500 is not a multiple of 64: a wave's entries straddle blocks and wrap from one sample into the next"""
    tup = parsed("cbox")
    on = render_run(tup, 50, 30, 24, env=ON)
    assert on.traced
    assert_same_run(on, render_run(tup, 50, 30, 24, env=OFF), "50x30")


def test_strip_lists_leave_a_cropped_render_bit_identical(parsed):
    *scene, cfg = parsed("cbox")
    tup = (*scene, dict(cfg, film={"width": 128, "height": 128, "crop_x": 70, "crop_y": 40, "crop_rx": 30, "crop_ry": 20}))
    on = render_run(tup, None, None, 16, env=ON)
    assert on.traced
    assert on.stats["n_samples"] == 60 * 40 * 16
    assert_same_run(on, render_run(tup, None, None, 16, env=OFF), "crop")


def test_strip_lists_leave_an_adaptive_render_bit_identical(parsed):
    tup = parsed("cbox")
    ad = {"threshold": 0.05, "min_spp": 8, "step": 4}
    on = render_run(tup, 64, 64, 12, calls=4, adaptive=ad, env=ON)
    assert on.traced and "[adaptive]" in on.variant
    assert_same_run(on, render_run(tup, 64, 64, 12, calls=4, adaptive=ad, env=OFF), "adaptive")


def test_strip_lists_leave_one_rank_of_two_bit_identical(parsed):
    """world_size = 2, rank 1 with bench.py's band width, on one device: the rank's local pixels are every other band of four columns"""
    tup = parsed("cbox")
    kw = dict(rank=1, world_size=2, band_width=4)
    on = render_run(tup, 128, 64, 16, env=ON, **kw)
    assert on.traced
    assert on.accum.shape[0] == 64                      # the rank's columns
    assert_same_run(on, render_run(tup, 128, 64, 16, env=OFF, **kw), "rank 1 of 2")
