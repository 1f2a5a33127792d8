"""What makes the cells of tests/kernel_cells.py meaningful, on the oracle alone (no device): each scene has the shape its cell needs,
the object under test fills enough of the film, every emitter reaches it, and - the condition that keeps the device test from passing a
wrong kernel member - the oracle's image of the object changes by at least ten times the product build's bound when the object's model is
swapped for another member of the same group kernel.

Smallest sensitivity ratio found (swapped-vs-right relMSE over the object region / the oracle's seed-1-vs-seed-2 relMSE there; the
condition asks >= 0.2): 0.716 at the film of kernel_cells.FILM (SMALLEST_RATIO below, asserted)."""
import numpy as np
import pytest

import kernel_cells as KC
from gpu_cases import _rel

SURFACE_SCENES = [(m, s) for m in KC.CLASSES for s in KC.EMITTER_SETS]          # the scenes of the sorted cells
ALL_KEYS = sorted({KC.scene_key(c) for c in KC.CELLS})
MIN_COVERAGE = 0.15
REACH_SPP = 32              # the single-emitter renders ask whether any light arrives, not how much
SMALLEST_RATIO = 0.7162        # the Oren-Nayar object under all five emitter kinds, shaded as Lambertian


def _types(tup):
    return tuple({0: "point", 1: "area", 2: "spot", 4: "collimated"}[int(e.pack()[0][0])] for e in tup[0])


@pytest.mark.parametrize("key", ALL_KEYS, ids=lambda k: "-".join(str(x) for x in k))
def test_scene_has_the_shape_and_coverage_its_cells_need(key):
    model, emitter_set, volumetric, grid = key
    ref = KC.reference(key)
    fs = ref.packed
    assert fs.n_prims <= 96, fs.n_prims                                     # the product build takes the flat sweep
    assert _types(ref.tup) == KC.EMITTER_TYPES[emitter_set]
    assert fs.has_volume == grid and (int(fs.med_i[-1]) >= 0) == volumetric
    kinds = {(int(i[2]), int(i[0]), bool((f[3:6] == 0).all())) for i, f in zip(fs.bxdf_i, fs.bxdf_f)}      # (bsdf, type, k_s == 0)
    classes = {(b, t if not (b == 0 and t == 0) else (t, no_ks)) for b, t, no_ks in kinds}
    assert len(classes) == len(KC.class_names(model)) == (8 if model == KC.ALL_MODELS else 2), classes
    assert ref.region.mean() >= MIN_COVERAGE, ref.region.mean()
    assert all(np.isfinite(img).all() for img in ref.cpu.values())
    assert ref.noise() > 0 and ref.noise(ref.region) > 0


@pytest.mark.parametrize("key", ALL_KEYS, ids=lambda k: "-".join(str(x) for x in k))
def test_every_emitter_reaches_the_object(key):
    """Each emitter alone (the others' intensity zero, the streams unchanged) lights the object region.  The collimated beam is the
    exception the reference itself makes: a beam of radius > 0 is no delta position, its sample carries pdf 0 (oracle/pt_oracle.c
    src_sample_hit, `s->type == 4`; upstream emitters/collimated.py), and the balance heuristic weighs a light sample of pdf 0 with 0 - with
    MIS on, as every cell renders, the beam's samples are taken, traced and evaluated, and add nothing.  So for the beam the region is held
    to exactly that, and to being lit by it once MIS is off: the beam does point at the object."""
    ref = KC.reference(key)
    region = ref.region
    for k, kind in enumerate(KC.EMITTER_TYPES[key[1]]):
        alone = KC.Reference(key, only_emitter=k, seeds=(0,), spp=REACH_SPP)
        assert alone.stats["n_shadow"] > 0, (key, k)
        if kind == "collimated":
            assert alone.cpu[0][region].max() == 0.0, (key, k)
            alone = KC.Reference(key, only_emitter=k, seeds=(0,), spp=REACH_SPP, use_mis=False)
        assert 0 < alone.cpu[0][region].mean(), (key, k)


@pytest.mark.parametrize("model,emitter_set", [(m, s) for m in KC.CLASSES for s in KC.EMITTER_SETS])
def test_the_contribution_log_sums_to_the_steady_image(model, emitter_set):
    """the reference of the transient cells (Reference.log_sum holds the log to the steady image wherever no sample's colour is NaN)"""
    ref = KC.reference((model, emitter_set, False, False))
    total, img = ref.log_sum()
    assert np.isfinite(total).all() and (ref.nan_colour_samples > 0 or np.allclose(img, ref.cpu[0], rtol=1e-5, atol=1e-6))


_swapped = {}


def _swapped_image(model, emitter_set, walls):
    k = (model, emitter_set, walls)
    if k not in _swapped:
        _swapped[k] = KC.Reference((model, emitter_set, False, False), walls=walls, seeds=(0,)).cpu[0]
    return _swapped[k]


def sensitivity_ratios(model, emitter_set):
    ref = KC.reference((model, emitter_set, False, False))
    reg, noise = ref.region, ref.noise(ref.region)
    return {other: _rel(_swapped_image(other, emitter_set, KC.walls_of(model))[reg], ref.cpu[0][reg]) / noise for other in KC.swap_partners(model)}


@pytest.mark.parametrize("model,emitter_set", SURFACE_SCENES)
def test_a_wrong_member_moves_the_object_by_ten_times_the_product_bound(model, emitter_set):
    ratios = sensitivity_ratios(model, emitter_set)
    print(model, emitter_set, {k: round(v, 2) for k, v in ratios.items()})
    assert min(ratios.values()) >= KC.SENSITIVITY_FACTOR * KC.PRODUCT_FRACTION_OF_NOISE, ratios


def test_the_smallest_sensitivity_ratio_is_the_recorded_one():
    smallest = min(min(sensitivity_ratios(m, s).values()) for m, s in SURFACE_SCENES)
    print("smallest sensitivity ratio", smallest)
    assert smallest == pytest.approx(SMALLEST_RATIO, rel=1e-3)


def test_the_matrix_is_complete_and_has_no_duplicates():
    cells = KC.CELLS
    assert len(set(cells)) == len(cells)
    classes = ["lambertian", "blinn-phong", "oren-nayar", "delta", "mod-phong", "fresnel-blend", "thin-coat", "lambert-trans", "microfacet",
               "blinn-phong(no lobe)"]                                      # csrc/api.hip kClass's names, restated once
    for pipeline in (KC.SORTED, KC.TRANSIENT):
        assert {(m, s) for m, s, p in cells if p == pipeline} == {(m, s) for m in classes for s in ("P+A", "ALL", "P+S")}
    for pipeline in (KC.VOLUMETRIC, KC.VOLUMETRIC_GRID):
        have = {(m, s) for m, s, p in cells if p == pipeline}
        assert have == {(m, s) for m in classes[:9] + [KC.ALL_MODELS] for s in ("P+A", "ALL")}          # the nine volumetric classes, and the one-queue scene
    for pipeline in (KC.STAGED, KC.TRACED):
        have = [(m, s) for m, s, p in cells if p == pipeline]
        assert ("blinn-phong", "P+A") in have and ("delta", "P+A") in have and ("glass", "P+A") in have
        assert {m for m, s in have if s == "ALL"} == set(classes[2:9]) - {"delta"}
    assert all(set(KC.swap_partners(m)) <= set(classes) for m in classes)
    assert sorted(sum(KC.GROUPS, ())) == sorted(classes) == sorted(sum(KC.VGROUPS, ()))
    assert set(KC.cells_of("fast")) == set(cells) and set(cells) - set(KC.cells_of("exact")) == {c for c in cells if c[2] == KC.TRACED}
