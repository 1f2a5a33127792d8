"""The ambient-occlusion renderer without a device: the C-ABI's new fields and symbol, the settings' defaults, the numpy
model (tests/ao_model.py) against every fixture the reference's ssao.py produced (tests/golden/ao_*.npz), the edge vectors of
rasterize_pinhole, splat_camera and the smooth step, and the condition tests/test_gpu_ao.py relies on: fragile pixel-samples stay rare."""
import os
import re

import numpy as np
import pytest

import ao_model as AM
from adapt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
_runs = {}


def model_run(name, parsed, build):
    """(model, run, fixture or None) of a GPU case, computed once per session"""
    key = (name, build)
    if key not in _runs:
        scene, kw, spp, fx = AM.case_scene(name, parsed)
        m = _runs[(name, None)][0] if (name, None) in _runs else AM.AoModel(scene, **kw)
        _runs[key] = (m, m.run(spp, build), fx)
    return _runs[key]


# ------------------------------------------------------------------ plumbing
def _members(struct):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "adapt_mi.h")).read(), flags=re.S)
    body = re.search(r"typedef struct " + struct + r"\s*\{(.*?)\}\s*" + struct + ";", text, flags=re.S).group(1)
    return [re.sub(r"\[.*?\]", "", part.strip().split()[-1].lstrip("*")) for decl in body.split(";") if decl.strip() for part in decl.strip().split(",")]


def test_the_ao_block_sits_directly_before_light_groups():
    block = ["ao", "ao_smp_hemisphere", "ao_depth_samples", "ao_sample_extent"]
    for names in (_members("apt_render_cfg"), [n for n, _ in _lib.RenderCfg._fields_]):
        k = names.index("light_groups")
        assert names[k - 4:k] == block and names[k - 5] == "volumetric"
        assert names[k:] == ["light_groups", "path_lengths", "adaptive_threshold", "adaptive_min_spp", "adaptive_step", "transient_bins", "transient_min_time", "transient_interval"]
    types = dict(_lib.RenderCfg._fields_)
    import ctypes as C
    assert [types[n] for n in block] == [C.c_int32, C.c_int32, C.c_int32, C.c_float]
    assert _members("apt_stats")[-1] == "n_stray_light" and _lib.Stats._fields_[-1][0] == "n_stray_light"


@pytest.mark.parametrize("variant", ["fast", "exact"])
def test_the_library_exports_the_depth_map_entry(variant):
    assert "apt_read_ao_depth" in _lib.SYMBOLS
    assert re.search(r"int apt_read_ao_depth\(apt_renderer\*, float\* out\);", open(os.path.join(ROOT, "include", "adapt_mi.h")).read())
    assert hasattr(_lib.load(variant), "apt_read_ao_depth")


def test_settings_come_from_the_sensor_then_upstreams_defaults():
    from adapt_amd.renderer import AO_DEFAULTS, AORenderer, SSAORenderer, Renderer, ao_settings
    import adapt_amd
    assert AO_DEFAULTS == {"smp_hemisphere": 32, "depth_samples": 64, "sample_extent": 0.1} == AM.AO_DEFAULTS
    assert ao_settings({}) == AO_DEFAULTS
    assert ao_settings({"smp_hemisphere": 5, "sample_extent": 0.25}) == {"smp_hemisphere": 5, "depth_samples": 64, "sample_extent": 0.25}
    assert ao_settings({"smp_hemisphere": 5}, smp_hemisphere=7, depth_samples=1) == {"smp_hemisphere": 7, "depth_samples": 1, "sample_extent": 0.1}
    with pytest.raises(ValueError, match="unknown"):
        ao_settings({}, samples=3)
    assert SSAORenderer is AORenderer and issubclass(AORenderer, Renderer) and adapt_amd.AORenderer is AORenderer and adapt_amd.SSAORenderer is AORenderer


def test_the_parser_hands_the_three_sensor_keys_through():
    import xml.etree.ElementTree as xet
    from adapt_amd.parsers.xml_parser import parse_global_sensor
    from adapt_amd.renderer import ao_settings
    sensor = xet.parse(os.path.join(ROOT, "scenes", "cbox", "c2_cbox.xml")).getroot().find("sensor")
    assert ao_settings(parse_global_sensor(sensor)) == {"smp_hemisphere": 32, "depth_samples": 64, "sample_extent": 0.1}
    for tag, name, value in (("integer", "smp_hemisphere", "5"), ("integer", "depth_samples", "7"), ("float", "sample_extent", "0.25")):
        xet.SubElement(sensor, tag, {"name": name, "value": value})
    prop = parse_global_sensor(sensor)
    assert ao_settings(prop) == {"smp_hemisphere": 5, "depth_samples": 7, "sample_extent": 0.25}


# ------------------------------------------------------------------ the model against the reference's fixtures
@pytest.mark.parametrize("name", list(AM.FIXTURES))
def test_model_reproduces_the_fixture_bit_for_bit(name, parsed):
    """depth map, the accumulation after every call, `pixels`, the draw counts of the depth pass and of every call: all equal, no tolerance
    (measured: every fixture bit for bit; profiles/ao_metrics.log)"""
    m, r, fx = model_run(name, parsed, None)
    assert np.array_equal(m.inv_cam_r, fx["inv_cam_r"]) and np.array_equal(m.cam_normal, fx["cam_normal"])
    assert (m.smp, m.depth_samples, m.extent) == (int(fx["smp_hemisphere"]), int(fx["depth_samples"]), F(fx["sample_extent"]))
    assert np.array_equal(r["depth"], fx["depth"])
    assert np.array_equal(r["depth_draws"], fx["depth_draws"]) and np.array_equal(r["draws"], fx["draws"])
    assert np.array_equal(r["accum"], fx["accum"])
    assert np.array_equal(r["pixels"], fx["pixels"])


def test_fixtures_show_the_semantics_they_were_chosen_for():
    fx = {n: AM.load_fixture(n) for n in AM.FIXTURES}
    c = fx["cbox"]
    assert (int(c["width"]), int(c["height"]), int(c["spp"])) == (32, 24, 3) and (int(c["smp_hemisphere"]), int(c["depth_samples"])) == (32, 64) and F(c["sample_extent"]) == F(0.1)
    for n, f in fx.items():
        hit_last = f["draws"][-1] > (2 if int(f["anti_alias"]) else 0)
        assert not f["accum"][..., 1].any() and all(np.array_equal(a[..., 2], f["depth"]) for a in f["accum"]), n      # channel 1 zero, channel 2 the depth map
        assert np.array_equal(f["pixels"][..., 0] != 0, hit_last & (f["accum"][-1][..., 0] != 0)), n                    # `pixels`: the last call's ray decides
        assert np.array_equal(f["pixels"][..., 0], f["pixels"][..., 1]) and np.array_equal(f["pixels"][..., 0], f["pixels"][..., 2])
        assert set(np.unique(f["draws"])) <= {0, 2 * int(f["anti_alias"]), 2 * int(f["anti_alias"]) + 2 * int(f["smp_hemisphere"])}, n
    crop = fx["cbox_crop"]
    sx, ex, sy, ey = crop["window"]
    outside = np.ones(crop["depth"].shape, bool); outside[sx:ex, sy:ey] = False
    assert int(crop["do_crop"]) and not crop["depth"][outside].any() and not crop["accum"][:, outside].any() and crop["depth"][~outside].any()
    assert int(fx["cbox_smp33"]["smp_hemisphere"]) == 33 and int(fx["cbox_smp1"]["smp_hemisphere"]) == 1 and int(fx["cbox_depth1"]["depth_samples"]) == 1
    assert not int(fx["cbox_no_aa"]["anti_alias"]) and not int(fx["cbox_no_strat"]["stratified"]) and int(fx["cbox_no_strat"]["anti_alias"])
    # a pixel whose last ray missed although an earlier one hit shows 0 in `pixels` with a non-zero accumulation: the last-call-missed rule is in the data
    assert any(((f["pixels"][..., 0] == 0) & (f["accum"][-1][..., 0] != 0)).any() for f in fx.values())


def test_stratified_jitter_of_the_depth_pass_stays_in_stratum_zero(parsed):
    """cnt is 0 while upstream's constructor runs: every depth sample's jitter lies in [0, 0.25)^2 - the quirk the model and the device keep"""
    m, _, fx = model_run("cbox_depth1", parsed, None)
    assert m.rc.stratified and m.rc.anti_alias
    i, j, script = 5, 7, [0.625, 0.375]
    at = lambda cnt: m.osc.pix2ray(m.rc, i, j, cnt, script)
    assert np.array_equal(at(0), at(16)) and not np.array_equal(at(0), at(1)) and not np.array_equal(at(0), at(4))      # counter 0 is stratum (0, 0), as 16 is
    # ... and the model's depth pass, which runs at counter 0, reproduces the fixture's one-sample depth map: the stratum is part of the data
    assert np.array_equal(m.depth_map()[0], fx["depth"])


# ------------------------------------------------------------------ edge vectors
CAM = dict(cam_normal=[0, 0, 1], inv_cam_r=np.eye(3, dtype=F), half_w=8.0, half_h=6.0, inv_focal=0.5)


def test_rasterize_truncates_toward_zero_and_tests_the_window():
    win = (0, 16, 0, 12)
    # fx = 9 - lx / 0.5: -0.2 truncates to 0 (a floor would give -1): a point just left of the film lands in column 0
    pi, pj, ok = AM.rasterize(8.0, 6.0, 0.5, win, F([4.6, 4.5, 5.0, 5.1, 1.0, -3.5, -3.49]), F([0.0] * 7))
    assert pi.tolist() == [0, 0, -1, -1, 7, 16, 15] and pj.tolist() == [7] * 7
    assert ok.tolist() == [True, True, False, False, True, False, True]
    # fy = 7 + ly / 0.5
    pi, pj, ok = AM.rasterize(8.0, 6.0, 0.5, win, F([0.0] * 5), F([-3.6, -4.0, 2.4, 2.5, -3.5]))
    assert pj.tolist() == [0, -1, 11, 12, 0] and ok.tolist() == [True, False, True, False, True]
    # a crop window: both borders, start inclusive, end exclusive
    pi, pj, ok = AM.rasterize(8.0, 6.0, 0.5, (4, 9, 3, 8), F([2.5, 2.51, 0.0, -0.01, 1.0, 1.0, 1.0, 1.0]), F([0.0, 0.0, 0.0, 0.0, -2.0, -2.01, 0.49, 0.5]))
    assert pi.tolist() == [4, 3, 9, 9, 7, 7, 7, 7] and pj.tolist() == [7, 7, 7, 7, 3, 2, 7, 8]
    assert ok.tolist() == [True, False, False, False, True, False, True, False]
    # values no int holds: refused, not wrapped
    assert not AM.rasterize(8.0, 6.0, 0.5, win, F([np.inf, -np.inf, np.nan, 3e30]), F([0.0] * 4))[2].any()


def test_splat_camera_gates():
    dm = np.arange(1, 16 * 12 + 1, dtype=F).reshape(16, 12)
    unit = lambda v: (np.asarray(v, F) / F(np.sqrt(np.dot(np.float64(v), np.float64(v))))).astype(F)
    ahead, behind, sideways = unit([0.1, -0.1, 1.0]), unit([0.1, -0.1, -1.0]), unit([1.0, 0.0, 0.0])
    test, (g1, g2, cell) = AM.splat_camera(np.stack([ahead, behind, sideways]), window=(0, 16, 0, 12), depth_map=dm, **CAM)
    assert g1.tolist() == [True, False, False] and g2.tolist() == [True, False, False]
    assert cell.tolist() == [8 * 12 + 6, -1, -1] and test.tolist() == [float(dm[8, 6]), 0.0, 0.0]
    # the two gates are different tests: a camera frame whose normal is not its inverse rotation's z row
    test, (g1, g2, cell) = AM.splat_camera(ahead[None], cam_normal=[0, 0, 1], inv_cam_r=-np.eye(3, dtype=F), half_w=8.0, half_h=6.0, inv_focal=0.5, window=(0, 16, 0, 12), depth_map=dm)
    assert g1.tolist() == [True] and g2.tolist() == [False] and test.tolist() == [0.0]
    # outside the crop window the lookup is 0 although the film has a value there
    test, (_, _, cell) = AM.splat_camera(ahead[None], window=(0, 8, 0, 12), depth_map=dm, **CAM)
    assert cell.tolist() == [-1] and test.tolist() == [0.0]


def test_smooth_step_and_the_compare_at_their_edges():
    assert AM.smooth_step(F([-1.0, 0.0, 0.5, 1.0, 7.0, np.inf, np.nan])).tolist() == [0.0, 0.0, 0.5, 1.0, 1.0, 1.0, 0.0]
    q = F(2.5) + F(1e-3)
    # queried == depth: extent / 0 is inf, the step saturates, the compare is >=: a full term
    term, behind = AM.occlusion_term(F([q, np.nextafter(q, F(0)), np.nextafter(q, F(9)), q + F(0.05), q + F(0.4)]), F([2.5] * 5), 0.1)
    assert behind.tolist() == [True, False, True, True, True]
    assert term[:4].tolist() == [1.0, 0.0, 1.0, 1.0] and 0.0 < term[4] < 0.2
    # nothing on the film there: queried = 0 + 1e-3, every point farther than a millimetre counts as behind (the sample_extent 2.0 fixture's branch)
    term, behind = AM.occlusion_term(F([5.0, 5e-4]), F([0.0, 0.0]), 2.0)
    assert behind.tolist() == [True, False] and term[0] == AM.smooth_step(F(2.0) / (F(5.0) - F(1e-3)))


# ------------------------------------------------------------------ what the GPU test relies on
@pytest.mark.parametrize("build", ["fast", "exact"])
@pytest.mark.parametrize("name", AM.GPU_CASES)
def test_fragile_samples_stay_under_the_cap(name, build, parsed):
    """A cap, not a measurement: the GPU test grants a fragile sample a whole term, so its bound only says something where few are.
    Measured (profiles/ao_metrics.log): product perturbation at most 0.17 % (balls_mono), exact perturbation none."""
    m, r, _ = model_run(name, parsed, build)
    hits = (r["draws"] > m.n_jitter).sum()
    assert hits > 0
    share = r["fragile"].sum() / float(hits * m.smp)
    print(f"{name} [{build}]: {int(r['fragile'].sum())} fragile of {int(hits * m.smp)} hemisphere samples = {share:.5f}")
    assert share <= AM.FRAGILE_CAP


def test_device_and_glibc_transcendentals_differ_by_one_ulp_at_most(parsed):
    """The exact build rounds a double cos / sin once (csrc/vec.hpp apt_sincos), the fixtures hold glibc's cosf / sinf.  On the azimuths the
    fixtures' last calls drew the two differ by at most 1 ulp - the size of the exact build's perturbation in tests/ao_model.py."""
    worst, n, n_diff = 0, 0, 0
    for name in ("cbox", "balls_mono", "cbox_smp33"):
        m, _, fx = model_run(name, parsed, None)
        phi = m.render_call(int(fx["spp"]), fx["depth"])["phi"]
        for lib, ref in ((AM.cosf, np.cos), (AM.sinf, np.sin)):
            a, b = lib(phi), ref(np.float64(phi)).astype(F)
            ulps = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
            worst, n, n_diff = max(worst, int(ulps.max())), n + ulps.size, n_diff + int((ulps > 0).sum())
    print(f"glibc float vs double rounded once: {n_diff} of {n} values differ, at most {worst} ulp")
    assert worst <= 1
