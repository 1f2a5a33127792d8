"""Occluder lists of the light samples (csrc/flat_build.cpp flat_occluders) on the device: every bundled scene that the
product build renders with the traced shade kernel (shade_stage.hpp k_shade_traced) gives the same accumulation and the same counters,
bit for bit, with the lists (APT_SHADOW_CULL=1, the default) and with the full stream for every emitter (APT_SHADOW_CULL=0)."""
import pytest

from gpu_ab import assert_same_run, render_run, traced_pairs

pytestmark = pytest.mark.gpu

ON, OFF = {"APT_SHADOW_CULL": "1"}, {"APT_SHADOW_CULL": "0"}


@pytest.mark.parametrize("unsorted", [False, True])
def test_occluder_lists_leave_every_traced_scene_bit_identical(parsed, flat, unsorted):
    traced = []
    for tag, on, _ in traced_pairs(parsed, unsorted, ON, OFF):
        assert on.stats["n_shadow_traced"] > 0 and on.stats["n_lit"] > 0, tag
        traced.append(tag)
    if not unsorted: return                             # (by default only the Cornell box takes the traced kernel)
    fs = {tag: flat(tag) for tag in traced}
    assert any((f.src_i[:, 0] == 1).any() for f in fs.values()), f"no area-light scene took the traced kernel: {sorted(traced)}"
    assert any(f.src_i.shape[0] > 1 for f in fs.values()), f"no multi-emitter scene took the traced kernel: {sorted(traced)}"


def test_occluder_lists_leave_c1_bit_identical(parsed):
    """C1: the Cornell box at 256 x 256, 4 bounces (bench.py's c1), with more samples per pixel"""
    tup = parsed("cbox")
    on = render_run(tup, 256, 256, 16, env=ON, max_bounce=4)
    assert on.traced
    assert_same_run(on, render_run(tup, 256, 256, 16, env=OFF, max_bounce=4), "c1")
