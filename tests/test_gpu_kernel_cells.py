"""Every shade kernel member against the oracle: one test per cell of tests/kernel_cells.py (surface model x emitter set x pipeline) and
build.  tests/test_kernel_cells_host.py holds the scenes to what makes a pass here mean something: another member's code on the object
would move the oracle's image of it by at least ten times the bound the product build gets below.

Per cell: the pipeline and variant of info() are the ones `kernel_cells.expected` declares; the exact build's image and counters meet
parity_bounds.EXACT against the oracle on the same Philox stream, over the whole film and over the object region; the product build's
counters meet gpu_cases.counters_within's defaults and its image relMSE(device, oracle seed 0) <= 0.02 x relMSE(oracle seed 1, oracle
seed 2), on the whole film and on the object region - the fraction tests/test_gpu_fast.py::test_no_systematic_difference_between_the_builds
holds between the two builds, of a noise that comes from the reference alone.  A transient cell's framebuffer is held to the same, and its
bins summed to that framebuffer (transient_cases.bins_sum_to_framebuffer); a traced cell renders once more with APT_CAMERA_FUSE=0, so
both the camera-fed and the queue-fed form run, and the two are the same render bit for bit (gpu_ab.assert_same_run).

Every run enters its cell into RAN; the last test holds RAN to the declared matrix.  All measured figures go through record_metric; the
log of record is profiles/kernel_cells_metrics.log."""
import numpy as np
import pytest

import kernel_cells as KC
import parity_bounds as PB
from conftest import record_metric
from gpu_ab import Run, assert_same_run, open_renderer, render_run
from gpu_cases import _rel, counters_within, image_within, render_with_oracle
from transient_cases import ALL_TIME, bins_sum_to_framebuffer

pytestmark = pytest.mark.gpu

BUILDS = ("exact", "fast")
W, H, SPP = KC.FILM
RAN = {b: set() for b in BUILDS}

# (No product cell misses the 0.02 x noise bound: there is no fallback list.  profiles/NOTES.md has the largest ratio per pipeline.)


def _cell_id(cell):
    return "-".join(cell)


def _check_pipeline(r, cell, build):
    info = r.info()
    variant_ok, traversals = KC.expected(cell, build)
    assert info["arithmetic"] == build and variant_ok(info["shade_variant"]) and info["traversal"] in traversals, (cell, build, info["shade_variant"], info["traversal"])
    return info


def _on(mask, img):
    """the pixels of `mask` as an image of one column (what conftest.image_metrics takes)"""
    return img[mask][:, None, :]


def _hold(cell, build, ref, acc, st):
    """clauses 2 - 5: the accumulation `acc` and the counters `st` of the device against the cell's reference: the oracle's steady
    render on the same stream - for a transient cell the sum of the oracle's contribution log on that stream (Reference.log_sum)"""
    ref_accum, ref_img = ref.log_sum() if cell[2] == KC.TRANSIENT else (ref.accum, ref.cpu[0])
    label = f"kernel cell {_cell_id(cell)} {build}"
    ost, areas = ref.stats, (("film", np.ones_like(ref.region)), ("object", ref.region))
    assert st["n_samples"] == ost["n_samples"] == W * H * SPP, (label, st["n_samples"], ost["n_samples"])
    img = acc.astype(np.float64) / SPP
    ratios = {name: _rel(img[m], ref_img[m]) / ref.noise(m) for name, m in areas}
    dev = {k: abs(st[k] - ost[k]) / max(1, ost[k]) for k in ("n_shade", "n_shadow", "n_draws")}
    record_metric(label, {**{f"same_seed_over_noise_{n}": v for n, v in ratios.items()}, **{f"noise_{n}": ref.noise(m) for n, m in areas},
                          **{f"{k}_rel_dev": v for k, v in dev.items()}, "n_shade": st["n_shade"], "n_shadow": st["n_shadow"], "n_draws": st["n_draws"]})
    if build == "exact":
        for name, m in areas:
            image_within(_on(m, acc), _on(m, ref_accum), SPP, PB.EXACT.within, PB.EXACT.rel, label=(label, name),
                         report=lambda mm, a, b, fin, name=name: record_metric(f"{label} {name}", mm))
        counters_within(st, ost, PB.EXACT.counters, 0, label=label)
        return
    counters_within(st, ost, label=label)
    for name, v in ratios.items():
        assert v <= KC.PRODUCT_FRACTION_OF_NOISE, (label, name, v)


@pytest.mark.parametrize("build,cell", [(b, c) for b in BUILDS for c in KC.cells_of(b)], ids=lambda x: x if isinstance(x, str) else _cell_id(x))
def test_cell(build, cell):
    ref = KC.reference(KC.scene_key(cell))
    env, pipeline = KC.SWITCHES[cell[2]], cell[2]
    kw = {"transient": ALL_TIME} if pipeline == KC.TRANSIENT else {}
    with open_renderer(ref.tup, W, H, env=env, exact=(build == "exact"), volumetric=KC.is_volumetric(cell), **kw) as r:
        info = _check_pipeline(r, cell, build)
        acc, st, _, _ = render_with_oracle(r, ref, ref.rc, SPP)
        if pipeline == KC.TRANSIENT:
            cube = r.transient()
            assert cube.shape == (1, W, H, 3)
            bins_sum_to_framebuffer(cube.astype(np.float64).sum(axis=0) * SPP, acc.astype(np.float64))
        if pipeline == KC.TRACED:
            fed = Run(info["shade_variant"], info["traversal"], r.tile_accum().copy(), r.stats(), None, r.camera_fused())
    if pipeline == KC.TRACED:
        queue_fed = render_run(ref.tup, W, H, SPP, env=dict(env, APT_CAMERA_FUSE="0"))
        assert fed.fused is True and queue_fed.fused is False and queue_fed.traced, (cell, fed.fused, queue_fed.fused, queue_fed.variant)
        assert_same_run(fed, queue_fed, cell)
    _hold(cell, build, ref, acc, st)
    RAN[build].add(cell)


def test_every_declared_cell_ran_on_the_kernel_it_was_declared_for():
    """reads what the tests above entered into RAN: run the whole module (an `-k` selection of this test alone has nothing to read)"""
    missing = {b: sorted(set(KC.cells_of(b)) - RAN[b]) for b in BUILDS}
    assert not any(missing.values()), missing
