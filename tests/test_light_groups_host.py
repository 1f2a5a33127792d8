"""Light groups, the host side.  CPU only: the premise tests/test_gpu_light_groups.py rests on - the oracle's log of the
scene with every emitter but k at zero intensity is emitter k's share of the full log, record for record - then the configuration plumbing
and the command line's parsing and refusals."""
import numpy as np
import pytest

from light_group_cases import HOST_CASES, light_group_sums, record_keys, single_lit
from adapt_amd.scene_pack import make_config
from oracle import binding as ob

W, H, SPP = 48, 32, 8


@pytest.fixture(scope="module")
def host_logs(parsed, flat):
    cache = {}

    def get(case):
        if case not in cache:
            tag, ov = HOST_CASES[case]
            rc, fs = make_config(parsed(tag)[3], width=W, height=H, **ov), flat(tag)
            full, per, _ = ob.OracleScene(fs, rc.cam_t).contributions(rc, SPP)
            singles = [ob.OracleScene(single_lit(fs, k), rc.cam_t).contributions(rc, SPP)[0] for k in range(fs.n_sources)]
            cache[case] = (rc, fs, full, per, singles)
        return cache[case]
    return get


@pytest.mark.parametrize("case", list(HOST_CASES))
def test_single_lit_logs_partition_the_full_log(case, host_logs):
    rc, fs, full, per, singles = host_logs(case)
    assert len(singles) == fs.n_sources >= 2
    keys = record_keys(full)
    assert len(np.unique(keys, axis=0)) == len(keys)                     # (pixel, sample, bounce, kind) names one record
    parts = np.concatenate(singles)
    pkeys = record_keys(parts)
    assert len(parts) == len(full) and len(np.unique(pkeys, axis=0)) == len(pkeys)      # no key in two single-lit logs, none twice in one
    order = np.lexsort(pkeys.T[::-1])                                    # the full log's order: pixel, sample, bounce, kind
    assert np.array_equal(pkeys[order], keys)                            # the same key set
    assert np.array_equal(parts["rgb"][order].view(np.uint32), full["rgb"].view(np.uint32))      # and every record's rgb, bit for bit
    # what the device tests assume of these cases: no non-finite record, no poisoned weight; and no NaN sample, except with the
    # Trowbridge-Reitz model (the `microfacet` tag parses with it switched on: 331 samples whose colour upstream zeroes after a NaN
    # throughput, their logged records all finite; parsed as Lambertian, as the model's switch leaves it by default, there is none)
    assert np.isfinite(full["rgb"]).all() and not per[..., 3].any()
    assert case == "microfacet" or not per[..., 4].any()
    # and the rule built on them adds up to the full log's pixel totals
    sums, counts = light_group_sums(singles, W * H)
    assert sums.shape == (fs.n_sources, 2, W * H, 3) and counts.sum() == len(full)
    total = np.zeros((W * H, 3))
    np.add.at(total, full["pixel"], full["rgb"].astype(np.float64))
    assert np.abs(sums.sum((0, 1)) - total).max() <= 1e-9 * max(1.0, np.abs(total).max())
    print(f"light_group_premise[{case}]: records per emitter {[len(s) for s in singles]}, total {len(full)}")


def test_features_b_has_records_for_every_emitter(host_logs):
    rc, fs, full, per, singles = host_logs("features_b")
    assert fs.n_sources == 5 and all(len(s) > 0 for s in singles), [len(s) for s in singles]
    # only the two area lights can be hit by a sampled ray
    hit = [int((s["kind"] == 0).sum()) for s in singles]
    assert hit[0] > 0 and hit[1] > 0 and hit[2:] == [0, 0, 0], hit


def test_config_plumbing(parsed):
    from adapt_amd import _lib
    from adapt_amd.cli import get_options, parse_light_gains
    assert _lib.RenderCfg().light_groups == 0
    names = [n for n, _ in _lib.RenderCfg._fields_]
    assert names[names.index("light_groups") + 1:] == ["path_lengths", "adaptive_threshold", "adaptive_min_spp", "adaptive_step", "transient_bins",
                                                       "transient_min_time", "transient_interval"]      # directly before the tail the older tests pin
    assert [n for n, _ in _lib.Stats._fields_][-1] == "n_stray_light"
    prop = parsed("features_b")[3]
    assert make_config(prop).light_groups is False
    rc = make_config(prop, light_groups=True)
    assert rc.light_groups is True and rc.path_lengths is False and rc.transient_bins == 0
    assert {"apt_read_light_groups", "apt_set_light_groups", "apt_relight"} <= set(_lib.SYMBOLS)
    o = get_options([])
    assert o.light_groups is False and o.light_gain == []
    o = get_options(["--type", "pt", "--light_groups", "--light_gain", "pt=0.5", "--light_gain", "spot=1,0.5,0.25"])
    assert o.light_groups is True and o.light_gain == ["pt=0.5", "spot=1,0.5,0.25"]
    assert parse_light_gains(o.light_gain) == {"pt": 0.5, "spot": (1.0, 0.5, 0.25)}
    for bad in ("pt", "=2", "pt=", "pt=1,2", "pt=a", "pt=nan"):
        with pytest.raises(ValueError, match="id=g or id=r,g,b"):
            parse_light_gains([bad])


@pytest.mark.parametrize("argv,message", [
    (["--type", "vpt", "--light_groups"], "surface renderer only"),
    (["--type", "pt", "--light_groups", "--transient", "--name", "transient_cbox.xml"], "--transient do not combine"),
    (["--type", "pt", "--light_groups", "--path_lengths"], "--path_lengths do not combine"),
    (["--type", "pt", "--light_groups", "--noise_threshold", "0.05"], "adaptive sampling and --light_groups do not combine"),
])
def test_cli_refusals(argv, message, capsys):
    from adapt_amd.cli import main
    assert main(argv + ["--scene", "cbox", "--no_gui"]) == 2
    err = capsys.readouterr().err
    assert "--light_groups" in err and message in err


@pytest.mark.parametrize("argv,message", [
    (["--type", "pt", "--light_gain", "pt=0.5"], "give --light_groups as well"),
    (["--type", "pt", "--light_groups", "--light_gain", "pt=1,2"], "id=g or id=r,g,b"),
])
def test_cli_light_gain_refusals(argv, message, capsys):
    from adapt_amd.cli import main
    assert main(argv + ["--scene", "cbox", "--no_gui"]) == 2
    err = capsys.readouterr().err
    assert "--light_gain" in err and message in err
