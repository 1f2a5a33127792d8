"""What the GPU tests of the A/B switches share (test_gpu_shadow_cull, _camera_cull, _camera_fuse, _draw_window, _settings_matrix): render
under a set of environment switches, collect the render as a `Run`, and the one definition of "the same render, bit for bit".  Not collected
by pytest (no `test_` prefix).  adapt_amd is imported inside the functions: the draw-window child imports this module to render with its library."""
import contextlib
import os
from collections import namedtuple

import numpy as np

from conftest import ALL_TAGS

COUNTERS = ("n_samples", "n_extend", "n_shade", "n_shadow", "n_shadow_traced", "n_lit", "n_draws", "n_poisoned")
TRACED = "[rays traced in place]"


@contextlib.contextmanager
def switches(env):
    """Set the environment switches of `env` for the body; afterwards, also on an exception, restore the values they had and remove the
    ones that were unset.  APT_SHADOW_CULL and APT_FLAT_DEFER_ALL are read once, at scene creation; APT_CAMERA_CULL, APT_CAMERA_FUSE,
    APT_SORTED, APT_FUSED and APT_TRAVERSAL at renderer creation.  A Renderer creates its scene, so creating it inside the body covers
    both; nothing reads them at render()."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


@contextlib.contextmanager
def open_renderer(tup, w, h, *, env=None, exact=False, volumetric=False, unsorted=False, **kw):
    """A renderer of the parsed scene `tup`, created under switches(env) and closed on exit.
    unsorted: APT_SORTED=0 and one light sample per vertex - the scenes of several material classes then take the traced kernels too"""
    from adapt_amd.renderer import Renderer, VolumeRenderer
    env = dict(env or {})
    if unsorted: env["APT_SORTED"], kw["num_shadow_ray"] = "0", 1
    with switches(env):
        r = (VolumeRenderer if volumetric else Renderer)(*tup, width=w, height=h, exact=exact, **kw)
    try:
        yield r
    finally:
        r.close()


class Run(namedtuple("Run", "variant traversal accum stats counts fused")):
    """One render: shade variant and traversal of info(), a copy of the rank's accumulation tile, stats(), a copy of the per-pixel sample
    counts (adaptive renders; else None), camera_fused()"""
    __slots__ = ()
    traced = property(lambda self: TRACED in self.variant)


def run_of(r, spp, calls=1):
    """`calls` render() calls of `spp` samples each on the renderer r -> Run"""
    for _ in range(calls):
        r.render(n_spp=spp)
    info, counts = r.info(), r.tile_sample_counts().copy() if r.adaptive else None
    return Run(info["shade_variant"], info["traversal"], r.tile_accum().copy(), r.stats(), counts, r.camera_fused())


def render_run(tup, w, h, spp, *, calls=1, **open_kwargs):
    with open_renderer(tup, w, h, **open_kwargs) as r:
        return run_of(r, spp, calls)


def differences(a, b):
    """What keeps two runs from being the same render, bit for bit: the accumulations compared as uint32 (so +0 differs from -0, and a NaN
    equals a NaN of the same bits), each counter of COUNTERS, the per-pixel sample counts where there are any.
    -> [("accumulation", max |a - b|), (counter, a's, b's), ("sample counts",)], empty if nothing does"""
    bad = []
    if not np.array_equal(a.accum.view(np.uint32), b.accum.view(np.uint32)):
        bad.append(("accumulation", float(np.nanmax(np.abs(a.accum - b.accum))) if a.accum.shape == b.accum.shape else float("inf")))
    bad += [(k, a.stats[k], b.stats[k]) for k in COUNTERS if a.stats[k] != b.stats[k]]
    if (a.counts is None) != (b.counts is None) or (a.counts is not None and not np.array_equal(a.counts, b.counts)):
        bad.append(("sample counts",))
    return bad


def assert_same_run(a, b, what):
    assert a.variant == b.variant, (what, a.variant, b.variant)
    assert not differences(a, b), (what, differences(a, b))


def traced_pairs(parsed, unsorted, on_env, off_env, film=(64, 64, 8), same=assert_same_run, untraced=None):
    """Every bundled scene rendered under on_env; the scenes that take the traced kernels once more under off_env, held to `same`
    (assert_same_run, or a module's own on top of it): yields (tag, on, off) for those.  The others go to untraced(tag, on), if given.
    The Cornell box must be among the traced ones, and with `unsorted` more than one scene (by default it is the only one)."""
    traced = []
    for tag in ALL_TAGS:
        tup = parsed(tag)
        on = render_run(tup, *film, env=on_env, unsorted=unsorted)
        if not on.traced:
            if untraced: untraced(tag, on)
            continue
        off = render_run(tup, *film, env=off_env, unsorted=unsorted)
        same(on, off, tag)
        traced.append(tag)
        yield tag, on, off
    assert "cbox" in traced, traced
    if unsorted: assert len(traced) > 1, traced
