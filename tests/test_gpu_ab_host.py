"""tests/gpu_ab.py without a device: `switches` leaves the environment as it found it, and `differences` / `assert_same_run` - the
bit-identity criterion the GPU tests of the A/B switches share - report exactly what differs between hand-made runs."""
import os

import numpy as np
import pytest

from gpu_ab import COUNTERS, Run, assert_same_run, differences, switches


@pytest.mark.parametrize("raises", [False, True])
def test_switches_restore_the_environment(monkeypatch, raises):
    monkeypatch.setenv("APT_TEST_WAS_SET", "before")
    monkeypatch.delenv("APT_TEST_WAS_UNSET", raising=False)
    try:
        with switches({"APT_TEST_WAS_SET": "inside", "APT_TEST_WAS_UNSET": "1"}):
            assert os.environ["APT_TEST_WAS_SET"] == "inside" and os.environ["APT_TEST_WAS_UNSET"] == "1"
            if raises: raise KeyError("from the body")
    except KeyError:
        assert raises
    assert os.environ["APT_TEST_WAS_SET"] == "before" and "APT_TEST_WAS_UNSET" not in os.environ


def _run(at=None, bits=0, **changes):
    """a run of a 4 x 3 x 3 accumulation; at, bits: that component's bit pattern is replaced"""
    accum = np.linspace(0.25, 9.0, 36, dtype=np.float32).reshape(4, 3, 3)
    if at: accum.view(np.uint32)[at] = bits
    return Run("lambertian/point [rays traced in place]", "flat", accum, {k: 100 + i for i, k in enumerate(COUNTERS)}, None, True)._replace(**changes)


def test_the_accumulation_is_compared_bit_by_bit():
    a = _run()
    assert differences(a, _run()) == [] and a.traced and not _run(variant="lambertian/point").traced
    assert_same_run(a, _run(), "equal")
    with pytest.raises(AssertionError, match="variant"):
        assert_same_run(a, _run(variant="lambertian/point"), "variant")
    b = _run((2, 1, 0), a.accum.view(np.uint32)[2, 1, 0] ^ 1)                # one mantissa bit of 5.5
    assert differences(a, b) == [("accumulation", 2.0 ** -21)]
    with pytest.raises(AssertionError, match="one bit.*accumulation"):
        assert_same_run(a, b, "one bit")
    plus, minus = _run((0, 0, 0), 0x00000000), _run((0, 0, 0), 0x80000000)
    assert plus.accum[0, 0, 0] == minus.accum[0, 0, 0]
    assert differences(plus, minus) == [("accumulation", 0.0)]
    nan = _run((3, 2, 2), 0x7fc00001)
    assert np.isnan(nan.accum[3, 2, 2]) and differences(nan, _run((3, 2, 2), 0x7fc00001)) == []
    assert [d[0] for d in differences(nan, _run((3, 2, 2), 0x7fc00002))] == ["accumulation"]


@pytest.mark.parametrize("counter", COUNTERS)
def test_a_counter_off_by_one_is_reported_under_its_name(counter):
    a = _run()
    b = _run(stats=dict(a.stats, **{counter: a.stats[counter] + 1}))
    assert differences(a, b) == [(counter, a.stats[counter], a.stats[counter] + 1)]
    with pytest.raises(AssertionError, match=counter):
        assert_same_run(a, b, "counter")


def test_sample_counts_are_compared_where_there_are_any():
    n = np.full((4, 3), 12, np.int32)
    m = n.copy(); m[1, 2] = 16
    assert differences(_run(counts=n), _run(counts=n.copy())) == []
    assert differences(_run(counts=n), _run(counts=m)) == differences(_run(counts=n), _run()) == [("sample counts",)]
    assert differences(_run(counts=None), _run(counts=None)) == []
