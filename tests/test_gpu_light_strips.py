"""Strip masks of the camera vertex's light samples (csrc/flat_build.cpp light_strips, traverse.hpp flat_any1's mask) on
the device: every render that takes the camera-fed launch gives the same accumulation and the same counters, bit for bit, with the masks
(the default) and with every pair of every strip swept (APT_LIGHT_STRIPS=0) - every scene that takes the traced kernels, C2's scene with
four bounces, a film of odd size, one bounce, every ray through the reference-order code, the camera lists off, two point lights, several
render() calls, one rank of two.  Cropped and adaptive renders keep the two-launch form and report that no masks are in use."""
import copy

import numpy as np
import pytest

from gpu_ab import assert_same_run, open_renderer, run_of, traced_pairs

pytestmark = pytest.mark.gpu

ON, OFF = {"APT_LIGHT_STRIPS": "1"}, {"APT_LIGHT_STRIPS": "0"}


def _run(tup, w, h, spp, env, calls=1, **kw):
    """-> Run, light_strips() of the renderer"""
    with open_renderer(tup, w, h, env=env, **kw) as r:
        return run_of(r, spp, calls), r.light_strips()


def _pair(tup, w, h, spp, what, env=None, masks=True, calls=1, **kw):
    """The same render with the masks and without.  masks: whether the first is expected to sweep against masks that leave pairs out"""
    (on, m_on), (off, m_off) = (_run(tup, w, h, spp, dict(sw, **(env or {})), calls, **kw) for sw in (ON, OFF))
    assert on.traced, what
    assert m_on is masks and m_off is False, (what, m_on, m_off)
    assert_same_run(on, off, what)
    return on


@pytest.mark.parametrize("unsorted", [False, True])
def test_light_strips_leave_every_traced_scene_bit_identical(parsed, unsorted):
    for tag, on, _ in traced_pairs(parsed, unsorted, ON, OFF, film=(64, 64, 4)):
        assert on.stats["n_shadow_traced"] > 0, tag


def test_the_cornell_box_renders_with_masks_in_use(parsed):
    """C2's scene, 128 x 128 x 2 spp, 4 bounces"""
    on = _pair(parsed("cbox"), 128, 128, 2, "c2 scene", max_bounce=4)
    assert on.fused and on.stats["n_lit"] > 0 and on.stats["n_lit"] < on.stats["n_shadow_traced"]      # samples reach the light, and some are blocked


def test_light_strips_leave_a_film_of_odd_size_bit_identical(parsed):
    """npix = 50 x 30 = 1500 is not a multiple of 64: a wave's rays straddle strips and wrap from one sample into the next"""
    on = _pair(parsed("cbox"), 50, 30, 8, "50x30")
    assert on.stats["n_samples"] == 50 * 30 * 8


def test_light_strips_leave_a_one_bounce_render_bit_identical(parsed):
    _pair(parsed("cbox"), 64, 64, 4, "max_bounce=1", max_bounce=1)


def test_light_strips_with_every_ray_through_the_reference_order_code(parsed):
    _pair(parsed("cbox"), 64, 48, 4, "defer all", env={"APT_FLAT_DEFER_ALL": "1"})


def test_light_strips_do_not_depend_on_the_camera_lists(parsed):
    _pair(parsed("cbox"), 64, 64, 4, "camera cull off", env={"APT_CAMERA_CULL": "0"})


def test_light_strips_with_two_point_lights(parsed):
    """a second light near the floor beside the tall block: each emitter has its own row of masks, and a wave whose lanes sampled both sweeps its full list"""
    emitters, arrays, objects, prop = parsed("cbox")
    second = copy.deepcopy(emitters[0])
    second.pos = np.float32([1.0, 0.6, 1.2])
    _pair(([emitters[0], second], arrays, objects, prop), 64, 64, 4, "two lights")


def test_light_strips_over_consecutive_renders(parsed):
    on = _pair(parsed("cbox"), 96, 80, 3, "3 renders", calls=3)
    assert on.stats["n_samples"] == 96 * 80 * 9


def test_light_strips_on_one_rank_of_two(parsed):
    on = _pair(parsed("cbox"), 128, 64, 4, "rank 1 of 2", rank=1, world_size=2, band_width=4)
    assert on.accum.shape[0] == 64


def test_a_cropped_render_uses_no_masks(parsed):
    *scene, cfg = parsed("cbox")
    tup = (*scene, dict(cfg, film={"width": 128, "height": 128, "crop_x": 70, "crop_y": 40, "crop_rx": 30, "crop_ry": 20}))
    on = _pair(tup, None, None, 4, "crop", masks=False)
    assert on.fused is False


def test_an_adaptive_render_uses_no_masks(parsed):
    on = _pair(parsed("cbox"), 64, 64, 12, "adaptive", masks=False, calls=2, adaptive={"threshold": 0.05, "min_spp": 8, "step": 4})
    assert on.fused is False and "[adaptive]" in on.variant
