"""tests/gpu_cases.py and tests/parity_bounds.py without a device: the criteria the GPU parity bodies hold their renders to - counters,
image, other seed - pass and raise exactly where they say, on hand-made 8 x 6 x 3 images and counter dicts; and the bounds table is
consistent with the scenes it names."""
import math

import numpy as np
import pytest

import parity_bounds as PB
from conftest import SCENES
from gpu_cases import COUNTER_KEYS, counters_within, image_within, other_seed_criterion, other_seed_criterion_exact

W, H, SPP = 8, 6, 4


@pytest.fixture(autouse=True)
def _no_metrics_log(monkeypatch):
    monkeypatch.delenv("APT_TEST_METRICS_LOG", raising=False)


# ---------------------------------------------------------------- counters_within
# oracle count, rel, floor (None: the defaults, parity_bounds.COUNTER_TOL): the floor active (a small oracle count) and inactive, and no floor
@pytest.mark.parametrize("oracle,rel,floor", [(1000, None, None), (1000000, None, None), (40000, 2e-4, 0), (90, 5e-4, 150)])
@pytest.mark.parametrize("key", COUNTER_KEYS)
@pytest.mark.parametrize("sign", [1, -1])
def test_counters_pass_at_the_bound_and_raise_one_count_beyond(oracle, rel, floor, key, sign):
    kw = {} if rel is None else {"rel": rel, "floor": floor}
    rel, floor = PB.COUNTER_TOL if rel is None else (rel, floor)
    bound = math.floor(max(rel * oracle, floor))
    assert (bound == floor) == (floor >= rel * oracle) and bound > 0
    ost = {k: oracle for k in COUNTER_KEYS}
    counters_within(dict(ost), ost, **kw)
    counters_within(dict(ost, **{key: oracle + sign * bound}), ost, **kw)
    with pytest.raises(AssertionError, match=key) as e:
        counters_within(dict(ost, **{key: oracle + sign * (bound + 1)}), ost, label="synthetic", **kw)
    assert e.value.args[0] == ("synthetic", key, oracle + sign * (bound + 1), oracle)


def test_counters_check_the_keys_they_are_given():
    ost = {"n_shade": 10, "n_shadow": 10, "n_draws": 1000}
    counters_within({"n_draws": 1002}, ost, 2e-3, 0, keys=("n_draws",))
    with pytest.raises(AssertionError, match="n_draws"):
        counters_within({"n_draws": 1003}, ost, 2e-3, 0, keys=("n_draws",))


# ---------------------------------------------------------------- image_within
def _images():
    """an oracle accumulation of SPP samples and an equal device accumulation"""
    ref = np.linspace(0.5, 9.0, W * H * 3).reshape(W, H, 3) * SPP
    return ref.copy(), ref


def test_equal_images_pass_and_one_pixel_just_outside_costs_one_48th():
    acc, ref = _images()
    m = image_within(acc, ref, SPP, 1.0, 0.0)
    assert m["frac_within"] == 1.0 and m["relMSE"] == 0.0 and m["max_abs"] == 0.0
    x = ref[5, 2, 1] / SPP
    acc[5, 2, 1] = (x + 0.999e-3 * (1 + x)) * SPP                       # just inside 1e-3 (1 + |x|)
    assert image_within(acc, ref, SPP, 1.0, 1e-6)["frac_within"] == 1.0
    acc[5, 2, 1] = (x + 1.001e-3 * (1 + x)) * SPP                       # just outside
    m = image_within(acc, ref, SPP, 47 / 48, 1e-6)
    assert m["frac_within"] == 47 / 48
    with pytest.raises(AssertionError, match="frac_within") as e:
        image_within(acc, ref, SPP, 0.98, 1e-6, label="synthetic")
    assert e.value.args[0] == ("synthetic", m)
    with pytest.raises(AssertionError, match="relMSE"):                  # and the relMSE bound holds on its own
        image_within(acc, ref, SPP, 47 / 48, 0.5 * m["relMSE"])


def test_a_report_sees_the_metrics_before_a_bound_fails():
    acc, ref = _images()
    acc[0, 0] += 1.0
    seen = []
    with pytest.raises(AssertionError):
        image_within(acc, ref, SPP, 1.0, 1.0, report=lambda m, a, b, fin: seen.append((m, a.shape, fin)))
    assert len(seen) == 1 and seen[0][0]["frac_within"] == 47 / 48 and seen[0][1] == (W, H, 3) and seen[0][2] is None


@pytest.mark.parametrize("mode", ["identical", "explained"])
def test_a_pixel_that_is_not_finite_in_both_images_is_left_out(mode):
    acc, ref = _images()
    acc[2, 3, 0] = ref[2, 3, 0] = np.inf
    acc[2, 3, 1] += 100.0                                               # whatever else that pixel holds is not compared
    with pytest.raises(AssertionError), np.errstate(invalid="ignore"):   # as they are: inf - inf is a NaN, no bound holds
        image_within(acc, ref, SPP, 0.0, 1.0)
    seen = []
    m = image_within(acc, ref, SPP, 1.0, 0.0, mode, explain=lambda a, b: pytest.fail("the maps agree: nothing to explain"),
                     report=lambda m, a, b, fin: seen.append(fin))
    assert m["frac_within"] == 1.0 and m["relMSE"] == 0.0
    assert seen[0].sum() == W * H - 1 and not seen[0][2, 3]


def test_identical_raises_on_a_pixel_that_is_not_finite_in_one_image_only():
    acc, ref = _images()
    acc[1, 1, 2] = np.inf
    with pytest.raises(AssertionError, match="finite components differ"):
        image_within(acc, ref, SPP, 0.0, 1.0, "identical", label="synthetic")


def test_explained_hands_such_a_pixel_to_the_callback():
    acc, ref = _images()
    acc[1, 1, 2] = np.inf
    calls = []

    def explain(a, b, ok=True):
        calls.append((np.argwhere(np.isfinite(a) != np.isfinite(b)).tolist(), a is acc, b is ref))
        return ok, ["pixel (1, 1)"]
    m = image_within(acc, ref, SPP, 1.0, 0.0, "explained", explain)      # the pixel itself is left out of the metrics
    assert m["frac_within"] == 1.0 and calls == [([[1, 1, 2]], True, True)]
    with pytest.raises(AssertionError, match=r"pixel \(1, 1\)"):
        image_within(acc, ref, SPP, 1.0, 0.0, "explained", lambda a, b: explain(a, b, ok=False))
    with pytest.raises(AssertionError):
        image_within(acc, ref, SPP, 1.0, 0.0, "no such option")


# ---------------------------------------------------------------- the other-seed criteria
def _seeds():
    """oracle images of three seeds: seed 0 flat, seeds 1 and 2 a checkerboard of +-0.1 around it, in opposite phase"""
    e = np.where(np.indices((W, H, 3)).sum(axis=0) % 2 == 0, 0.1, -0.1)
    base = np.ones((W, H, 3))
    return {0: base, 1: base + e, 2: base - e}


def _rel(a, b):
    return float(np.mean((a - b) ** 2 / (b ** 2 + 1e-2)))


CRITERIA = [pytest.param(lambda label, hip, cpu, frac: other_seed_criterion_exact(label, hip, cpu), id="exact"),
            pytest.param(other_seed_criterion, id="product")]


@pytest.mark.parametrize("criterion", CRITERIA)
def test_the_same_estimator_on_seed_0_passes(criterion):
    cpu = _seeds()
    criterion("synthetic", cpu[0].copy(), cpu, None)
    criterion("synthetic", cpu[0] + 0.005, cpu, None)                   # same-seed distance 2.5e-5: inside 8(d)'s 1e-4


@pytest.mark.parametrize("criterion", CRITERIA)
def test_an_image_far_from_both_other_seeds_raises(criterion):
    cpu = _seeds()
    hip = cpu[0] + 0.5
    pair = max(_rel(cpu[1], cpu[2]), _rel(cpu[0], cpu[1]), _rel(cpu[0], cpu[2]))
    assert min(_rel(hip, cpu[1]), _rel(hip, cpu[2])) > 1.5 * pair
    with pytest.raises(AssertionError) as e:
        criterion("synthetic", hip, cpu, None)
    assert e.value.args[0][:2] == ("synthetic", _rel(hip, cpu[1]))       # the first assertion: the distance to seed 1 leads its message


@pytest.mark.parametrize("criterion", CRITERIA)
def test_a_same_seed_distance_above_its_bound_raises(criterion):
    cpu = _seeds()
    hip = cpu[0] + 0.03
    noise, same = _rel(cpu[1], cpu[2]), _rel(hip, cpu[0])
    assert 1e-4 < same < noise and _rel(hip, cpu[1]) <= 1.5 * _rel(cpu[0], cpu[1]) and _rel(hip, cpu[2]) <= 1.5 * _rel(cpu[0], cpu[2])
    with pytest.raises(AssertionError) as e:
        criterion("synthetic", hip, cpu, None)
    assert e.value.args[0] == ("synthetic", same, noise)


def test_the_product_criterion_takes_its_same_seed_bound_as_a_fraction_of_the_noise():
    cpu = _seeds()
    hip = cpu[0] + 0.03
    noise, same = _rel(cpu[1], cpu[2]), _rel(hip, cpu[0])
    assert 1e-2 * noise < same <= 5e-2 * noise
    other_seed_criterion("synthetic", hip, cpu, 5e-2)
    with pytest.raises(AssertionError) as e:
        other_seed_criterion("synthetic", hip, cpu, 1e-2)
    assert e.value.args[0] == ("synthetic", same, noise)
    hip[3, 3] = np.nan                                                   # a pixel that is not finite is left out of every distance
    other_seed_criterion("synthetic", hip, cpu, 5e-2)


# ---------------------------------------------------------------- the bounds table
def test_the_bounds_table_names_scenes_that_exist():
    tags = [row[0] for row in PB.PRODUCT_IMAGE_CASES]
    assert set(tags) <= set(SCENES)
    assert set(PB.SAME_SEED_FRACTION_OF_NOISE) <= set(tags)
    for tag, w, h, spp, ov, min_within, max_rel in PB.PRODUCT_IMAGE_CASES:
        assert 0 < min_within < 1 and 0 < max_rel < 1 and w * h * spp > 0 and isinstance(ov, dict)


def test_the_survey_rows_are_the_survey_s():
    """SURVEY 8(d), restated once on purpose"""
    assert tuple(PB.EXACT) == (0.995, 1e-4, 2e-4)
    assert tuple(PB.REFERENCE_RUN) == (0.99, 2e-4, 2e-3)
