"""Strip lists of the camera rays (csrc/flat_build.cpp camera_strips) on the device: every bundled scene that the product
build renders with rays traced in place (stages.hpp k_generate_trace) gives the same accumulation and the same counters, bit for bit,
with the lists (APT_CAMERA_CULL=1, the default) and with the full stream for every strip (APT_CAMERA_CULL=0) - also cropped, adaptive,
and as one rank of two."""
import os

import numpy as np
import pytest

from conftest import ALL_TAGS

pytestmark = pytest.mark.gpu

COUNTERS = ("n_samples", "n_extend", "n_shade", "n_shadow", "n_shadow_traced", "n_lit", "n_draws", "n_poisoned")


def _render(tup, cull, w, h, spp, max_bounce=None, unsorted=False, calls=1, **kw):
    """unsorted: APT_SORTED=0 and one light sample per vertex - the scenes of several material classes then take the traced kernels too.
    -> shade variant, the rank's accumulation, counters, per-pixel sample counts (adaptive renders; else None)"""
    from adapt_amd.renderer import Renderer
    env = {"APT_CAMERA_CULL": str(cull)}                # read at renderer creation
    if unsorted: env["APT_SORTED"] = "0"                # read at renderer creation
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
        return r.info()["shade_variant"], r.tile_accum().copy(), r.stats(), counts
    finally:
        r.close()


def _same(a, b, what):
    name1, acc1, st1, n1 = a
    name0, acc0, st0, n0 = b
    assert name0 == name1
    assert np.array_equal(acc0.view(np.uint32), acc1.view(np.uint32)), (what, float(np.nanmax(np.abs(acc0 - acc1))))
    for k in COUNTERS:
        assert st0[k] == st1[k], (what, k, st0[k], st1[k])
    if n1 is not None: assert np.array_equal(n0, n1), what


@pytest.mark.parametrize("unsorted", [False, True])
def test_strip_lists_leave_every_traced_scene_bit_identical(parsed, unsorted):
    traced = []
    for tag in ALL_TAGS:
        tup = parsed(tag)
        on = _render(tup, 1, 64, 64, 8, unsorted=unsorted)
        if "[rays traced in place]" not in on[0]:
            continue
        _same(on, _render(tup, 0, 64, 64, 8, unsorted=unsorted), tag)
        assert on[2]["n_extend"] > 0 and on[2]["n_shade"] > 0, tag
        traced.append(tag)
    assert "cbox" in traced, traced
    if unsorted: assert len(traced) > 1, traced         # (by default only the Cornell box takes the traced kernels)


def test_strip_lists_leave_c1_bit_identical(parsed):
    """C1: the Cornell box at 256 x 256, 4 bounces (bench.py's c1), with more samples per pixel"""
    tup = parsed("cbox")
    on = _render(tup, 1, 256, 256, 16, max_bounce=4)
    assert "[rays traced in place]" in on[0]
    _same(on, _render(tup, 0, 256, 256, 16, max_bounce=4), "c1")


def test_strip_lists_leave_a_film_of_odd_size_bit_identical(parsed):
    """npix = 50 x 30 = 1500 is not a multiple of 64: a wave's entries straddle blocks and wrap from one sample into the next"""
    tup = parsed("cbox")
    on = _render(tup, 1, 50, 30, 24)
    assert "[rays traced in place]" in on[0]
    _same(on, _render(tup, 0, 50, 30, 24), "50x30")


def test_strip_lists_leave_a_cropped_render_bit_identical(parsed):
    emitters, arrays, objects, cfg = parsed("cbox")
    cfg = dict(cfg); cfg["film"] = {"width": 128, "height": 128, "crop_x": 70, "crop_y": 40, "crop_rx": 30, "crop_ry": 20}
    tup = (emitters, arrays, objects, cfg)
    on = _render(tup, 1, None, None, 16)
    assert "[rays traced in place]" in on[0]
    assert on[2]["n_samples"] == 60 * 40 * 16
    _same(on, _render(tup, 0, None, None, 16), "crop")


def test_strip_lists_leave_an_adaptive_render_bit_identical(parsed):
    tup = parsed("cbox")
    ad = {"threshold": 0.05, "min_spp": 8, "step": 4}
    on = _render(tup, 1, 64, 64, 12, calls=4, adaptive=ad)
    assert "[rays traced in place]" in on[0] and "[adaptive]" in on[0]
    _same(on, _render(tup, 0, 64, 64, 12, calls=4, adaptive=ad), "adaptive")


def test_strip_lists_leave_one_rank_of_two_bit_identical(parsed):
    """world_size = 2, rank 1 with bench.py's band width, on one device: the rank's local pixels are every other band of four columns"""
    tup = parsed("cbox")
    kw = dict(rank=1, world_size=2, band_width=4)
    on = _render(tup, 1, 128, 64, 16, **kw)
    assert "[rays traced in place]" in on[0]
    assert on[1].shape[0] == 64                         # the rank's columns
    _same(on, _render(tup, 0, 128, 64, 16, **kw), "rank 1 of 2")
