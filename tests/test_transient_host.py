"""Transient (time-resolved) rendering, host side: the sensor's transient keys -> RenderConfig, the C-ABI fields, the float32 bin
index, and the CLI's refusal outside `--type pt`.  No device needed."""
import os

import numpy as np
import pytest

from conftest import ROOT
from adapt_amd import _lib
from adapt_amd.scene_pack import make_config, transient_bin_index, transient_config


@pytest.fixture(scope="module")
def trans_prop():
    from adapt_amd.parsers import scene_parsing
    return scene_parsing(os.path.join(ROOT, "scenes", "cbox"), "transient_cbox.xml")[3]


def test_transient_scene_carries_upstream_keys(trans_prop):
    assert trans_prop["decomposition"] == "transient_cam"
    assert (trans_prop["sample_count"], trans_prop["min_time"], trans_prop["interval"]) == (400, 11.0, 0.1)


def test_decomposition_alone_leaves_the_mode_off(trans_prop):
    rc = make_config(trans_prop)
    assert (rc.transient_bins, rc.transient_min_time, rc.transient_interval) == (0, 0.0, 0.0)
    assert make_config(trans_prop, transient=False).transient_bins == 0


def test_transient_true_reads_the_sensor(trans_prop):
    rc = make_config(trans_prop, transient=True)
    assert (rc.transient_bins, rc.transient_min_time, rc.transient_interval) == (400, 11.0, 0.1)


def test_transient_defaults_are_upstreams():
    """bdpt.py:47,98-99: sample_count 1, min_time 0.0, interval 0.1 when the sensor does not say"""
    assert transient_config({}, True) == (1, 0.0, 0.1)


def test_transient_dict_overrides(trans_prop):
    rc = make_config(trans_prop, transient={"sample_count": 8, "interval": 0.5})
    assert (rc.transient_bins, rc.transient_min_time, rc.transient_interval) == (8, 11.0, 0.5)
    with pytest.raises(ValueError):
        transient_config(trans_prop, {"bins": 3})


@pytest.mark.parametrize("interval", [0.0, -0.1])
def test_non_positive_interval_raises(trans_prop, interval):
    """bdpt.py:107-108"""
    with pytest.raises(ValueError):
        make_config(trans_prop, transient={"interval": interval})
    with pytest.raises(ValueError):
        transient_config({"interval": interval}, True)


def test_abi_fields_are_appended():
    names = [n for n, _ in _lib.RenderCfg._fields_]
    assert names[-3:] == ["transient_bins", "transient_min_time", "transient_interval"]
    assert "apt_read_transient" in _lib.SYMBOLS and "apt_set_transient" in _lib.SYMBOLS
    assert _lib.RenderCfg().transient_bins == 0                 # zero-initialised configs render in steady state


def test_bin_index_matches_upstream_formula_on_edges():
    """bdpt.py:164-165 in float32: a contribution counts when min < t < min + interval * n, its bin is int((t - min) / interval)"""
    lo, step, n = np.float32(11.0), np.float32(0.1), 400
    hi = np.float32(float(lo) + float(step) * n)
    edges = lo + step * np.arange(n + 1, dtype=np.float32)
    t = np.concatenate([edges, np.nextafter(edges, np.float32(-np.inf)), np.nextafter(edges, np.float32(np.inf)),
                        np.float32([lo, hi, 0.0, -1.0, 1e9, np.nan, np.inf])]).astype(np.float32)
    got = transient_bin_index(t, 11.0, 0.1, n)
    for ti, g in zip(t, got):
        if lo < ti < hi:
            want = min(int(np.float32(ti - lo) / step), n - 1)
        else:
            want = -1
        assert g == want, (float(ti), g, want)
    assert transient_bin_index(np.float32([lo]), 11.0, 0.1, n)[0] == -1          # the window is open at both ends
    assert transient_bin_index(np.float32([hi]), 11.0, 0.1, n)[0] == -1
    assert transient_bin_index(np.nextafter(lo, np.float32(1e9)), 11.0, 0.1, n) == 0
    assert transient_bin_index(np.nextafter(hi, np.float32(0)), 11.0, 0.1, n) == n - 1


def test_cli_rejects_transient_outside_pt(capsys):
    from adapt_amd.cli import main
    assert main(["--type", "vpt", "--transient", "--scene", "cbox", "--name", "transient_cbox.xml", "--no_gui"]) == 2
    assert "--type pt" in capsys.readouterr().err


def test_cli_parses_transient_flag():
    from adapt_amd.cli import get_options
    assert get_options(["--transient"]).transient is True
    assert get_options([]).transient is False
