"""Adaptive sampling, host side: the retirement rule restated in numpy and held against the library's host statement,
the round schedule of a render call, the renderer's settings, the C-ABI fields and the CLI.  No device needed."""
import numpy as np
import pytest

from adapt_amd import _lib
from adaptive_cases import rule_error
from adapt_amd.renderer import adaptive_config, adaptive_segments, relative_error


def retires(s1, s2, n, threshold, min_spp):
    """the retirement rule: n_p >= min_spp and e_p <= threshold (the threshold as the float32 the C-ABI carries)"""
    return (np.asarray(n) >= min_spp) & (rule_error(s1, s2, n) <= np.float64(np.float32(threshold)))


def moments_of(samples):
    """S1 as k_finalize sums it (float32, in order, NaN components dropped), S2 in float64 the same way; samples (k, 3) float32"""
    s1 = np.zeros(3, np.float32); s2 = np.zeros(3, np.float64)
    for c in np.asarray(samples, np.float32):
        s1 = s1 + np.where(np.isnan(c), np.float32(0), c).astype(np.float32)
        s2 = s2 + np.where(np.isnan(c), 0.0, np.float64(c) * np.float64(c))
    return s1, s2


def test_estimator_matches_the_textbook_standard_error():
    rs = np.random.RandomState(3)
    x = rs.gamma(2.0, 0.3, size=(40, 3)).astype(np.float32)
    s1, s2 = moments_of(x)
    se = np.std(x.astype(np.float64), axis=0, ddof=1) / np.sqrt(40)
    want = np.max(se / (x.astype(np.float64).mean(0) + 1e-3))
    assert np.isclose(rule_error(s1[None], s2[None], [40])[0], want, rtol=1e-6)
    assert np.isclose(relative_error(s1[None], s2[None], [40])[0], want, rtol=1e-6)


def test_estimator_below_two_samples_is_infinite():
    s1 = np.float32([[0.5, 0.5, 0.5], [0, 0, 0]]); s2 = np.float64([[0.25, 0.25, 0.25], [0, 0, 0]])
    assert np.all(np.isinf(rule_error(s1, s2, [1, 0]))) and np.all(np.isinf(relative_error(s1, s2, [1, 0])))
    assert not retires(s1, s2, [1, 0], 1e9, 1).any()


def test_estimator_zero_mean_and_constant_pixels_retire():
    s1 = np.float32([[0, 0, 0], [3.2, 3.2, 3.2]]); s2 = np.float64([[0, 0, 0], [0.32, 0.32, 0.32]])     # all-zero; ten samples of 0.32
    e = relative_error(s1, s2, [10, 10])
    assert e[0] == 0.0 and e[1] <= 1e-7
    assert np.array_equal(e, rule_error(s1, s2, [10, 10]))
    assert retires(s1, s2, [10, 10], 1e-3, 8).all() and not retires(s1, s2, [10, 10], 1e-3, 11).any()


def test_estimator_infinite_sample_keeps_the_pixel_active():
    x = np.float32([[0.1, 0.2, 0.3]] * 7 + [[np.inf, 0.2, 0.3]])
    s1, s2 = moments_of(x)
    assert np.isinf(s1[0]) and np.isinf(s2[0])
    assert np.isinf(relative_error(s1[None], s2[None], [8])[0]) and np.isinf(rule_error(s1[None], s2[None], [8])[0])
    assert not retires(s1[None], s2[None], [8], 1e30, 1).any()


def test_estimator_drops_nan_components_as_finalize_does():
    x = np.float32([[0.1, 0.2, 0.3], [np.nan, 0.25, 0.3], [0.12, np.nan, 0.31], [0.11, 0.2, 0.29]])
    s1, s2 = moments_of(x)
    assert np.all(np.isfinite(s1)) and np.all(np.isfinite(s2))
    clean = np.where(np.isnan(x), 0, x)                        # the dropped component counts as a zero sample, as in the image
    s1c, s2c = moments_of(clean)
    assert np.array_equal(s1, s1c) and np.array_equal(s2, s2c)
    e = relative_error(s1[None], s2[None], [4])
    assert np.isfinite(e[0]) and np.array_equal(e, rule_error(s1[None], s2[None], [4]))


def test_library_rule_agrees_with_the_restatement_on_random_moments():
    rs = np.random.RandomState(11)
    n = rs.randint(0, 300, size=(24, 17))
    x = rs.exponential(0.4, size=(24, 17, 3))
    s1 = (x * n[..., None]).astype(np.float32)
    s2 = (x * x * n[..., None] * rs.uniform(0.9, 3.0, size=(24, 17, 3)))
    s1[0, 0, 1] = np.inf; s2[0, 0, 1] = np.inf
    a, b = relative_error(s1, s2, n), rule_error(s1, s2, n)
    assert np.array_equal(np.isinf(a), np.isinf(b)) and np.allclose(a[np.isfinite(a)], b[np.isfinite(b)], rtol=1e-12, atol=0)


@pytest.mark.parametrize("min_spp,step", [(64, 32), (50, 32), (1, 1), (7, 5), (200, 16)])
def test_round_schedule_does_not_depend_on_the_call_split(min_spp, step):
    total = 333
    rs = np.random.RandomState(min_spp + step)
    whole = adaptive_segments(0, total, min_spp, step)
    decisions = [last for first, last, d in whole if d]
    assert all(d % step == 0 and d >= min_spp for d in decisions)
    assert decisions == [m for m in range(1, total + 1) if m % step == 0 and m >= min_spp]
    assert whole[0][0] == 1 and whole[-1][1] == total and all(b[0] == a[1] + 1 for a, b in zip(whole, whole[1:]))
    for _ in range(5):
        cuts = np.sort(rs.choice(np.arange(1, total), size=rs.randint(1, 12), replace=False))
        calls = np.diff(np.concatenate([[0], cuts, [total]]))
        cnt, pieces = 0, []
        for k in calls:
            pieces += adaptive_segments(cnt, int(k), min_spp, step)
            cnt += int(k)
        assert [last for _, last, d in pieces if d] == decisions          # the same decision points, whatever the split
        assert sum(last - first + 1 for first, last, _ in pieces) == total
    assert adaptive_segments(5, 0, min_spp, step) == []


def test_adaptive_config_defaults_and_refusals():
    assert adaptive_config(None) is None and adaptive_config(False) is None
    assert adaptive_config({"threshold": 0.05}) == {"threshold": 0.05, "min_spp": 64, "step": 32}
    assert adaptive_config({"threshold": 0.1, "min_spp": 8, "step": 4}) == {"threshold": 0.1, "min_spp": 8, "step": 4}
    for bad in ({"threshold": 0}, {"threshold": -1}, {"threshold": float("nan")}, {"threshold": 0.1, "step": 0}, {"threshold": 0.1, "min_spp": -2},
                {"threshold": 0.1, "steps": 4}):
        with pytest.raises(ValueError):
            adaptive_config(bad)
    with pytest.raises(TypeError):
        adaptive_config(0.1)


def test_render_cfg_carries_the_adaptive_fields():
    names = [n for n, _ in _lib.RenderCfg._fields_]
    assert names[-6:-3] == ["adaptive_threshold", "adaptive_min_spp", "adaptive_step"]         # before the transient block, which stays last
    assert _lib.RenderCfg().adaptive_threshold == 0.0                                          # zero-initialised configs sample uniformly
    for sym in ("apt_read_sample_counts", "apt_read_moments", "apt_set_adaptive_state"):
        assert sym in _lib.SYMBOLS


def test_cli_parses_adaptive_flags():
    from adapt_amd.cli import get_options
    o = get_options([])
    assert (o.noise_threshold, o.min_spp, o.adaptive_step) == (0.0, 64, 32)
    o = get_options(["--noise_threshold", "0.02", "--min_spp", "16", "--adaptive_step", "8"])
    assert (o.noise_threshold, o.min_spp, o.adaptive_step) == (0.02, 16, 8)


def test_cli_rejects_transient_with_adaptive(capsys):
    from adapt_amd.cli import main
    assert main(["--type", "pt", "--transient", "--noise_threshold", "0.05", "--scene", "cbox", "--name", "transient_cbox.xml", "--no_gui"]) == 2
    err = capsys.readouterr().err
    assert "--transient" in err and "adaptive" in err


@pytest.mark.parametrize("argv", [["--noise_threshold", "-0.1"], ["--noise_threshold", "0.1", "--min_spp", "0"], ["--noise_threshold", "0.1", "--adaptive_step", "-4"]])
def test_cli_rejects_bad_adaptive_settings(argv):
    from adapt_amd.cli import main
    assert main(["--type", "pt", "--no_gui"] + argv) == 2
