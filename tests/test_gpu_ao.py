"""The ambient-occlusion renderer on the device, both builds, against the fixtures the reference's ssao.py produced
(tests/golden/ao_*.npz) and, where there is no fixture, against the numpy model that reproduces them bit for bit (tests/ao_model.py).

The bound on the accumulation, per pixel: |device - reference| <= (the pixel's fragile hemisphere samples so far) / smp_hemisphere + ROUND.
A fragile sample (ao_model.py) may take the other side of an int() truncation or of the depth compare and move by a whole term; every
other sample differs by rounding only.  tests/test_ao_host.py caps the fragile share at 2 % on every case here.  ROUND is twice the
largest difference measured on non-fragile pixels of the fixture cases (profiles/ao_metrics.log):
  exact build  measured 2.03e-6 (cbox_smp1: one hemisphere sample per ray, a term on the smooth step's slope where the device's sin / cos,
               rounded once from double, and glibc's differ by an ulp); every other case <= 3.6e-7, most bit for bit
  product build measured 1.663e-5 (cbox, three calls at upstream's defaults; features_a 1.57e-5; fast division, float sin / cos, intersector t
               within 1e-5 relative)."""
import numpy as np
import pytest

import ao_model as AM
from adapt_amd import _lib
from adapt_amd._lib import AptError
from adapt_amd.renderer import AORenderer, Renderer

pytestmark = pytest.mark.gpu

BUILDS = ["exact", "fast"]
ROUND = {"exact": 2 * 2.03e-6, "fast": 2 * 1.663e-5}
DEPTH_REL = 1e-5                       # product build: the intersector's stated accuracy
_model, _device = {}, {}


def reference(name, build, parsed):
    """what the device is held to: the fixture where there is one, else the model's run; and the model's fragile counts for the build"""
    if (name, build) not in _model:
        scene, kw, spp, fx = AM.case_scene(name, parsed)
        m = _model[name] if name in _model else AM.AoModel(scene, **kw)
        _model[name] = m
        r = m.run(spp, build)
        ref = fx if fx is not None else r
        _model[(name, build)] = {"depth": ref["depth"], "accum": ref["accum"], "pixels": ref["pixels"], "fragile": r["fragile"], "smp": m.smp, "spp": spp,
                                 "depth_hits": r["depth_hits"], "scene": scene, "kw": kw}
    return _model[(name, build)]


def device_run(name, build, parsed, traversal=None, monkeypatch=None, **extra):
    """depth map, the accumulation after every call (one sample per call, as upstream is driven) and `pixels`, once per (case, build, traversal)"""
    key = (name, build, traversal, tuple(sorted(extra.items())))
    if key not in _device:
        ref = reference(name, build, parsed)
        if traversal:
            monkeypatch.setenv("APT_TRAVERSAL", traversal)
        rdr = AORenderer(*ref["scene"], exact=(build == "exact"), **ref["kw"], **extra)
        out = {"info": rdr.info(), "depth": rdr.depth_map(), "accum": []}
        for _ in range(ref["spp"]):
            rdr.render(0, 0, 0, 0, 0, 0)
            out["accum"].append(rdr.color.to_numpy())
        out["accum"] = np.stack(out["accum"])
        out["pixels"], out["cnt"] = rdr.pixels.to_numpy(), rdr.cnt[None]
        rdr.close()
        _device[key] = out
    return _device[key]


def hold(dev, ref, build, label):
    """the three comparisons of a case: depth map, accumulation after every call, `pixels`; prints the figures before it asserts"""
    exact = build == "exact"
    d, rd = dev["depth"], ref["depth"]
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(rd > 0, np.abs(d - rd) / rd, np.where(d > 0, np.inf, 0.0))
    acc, racc = dev["accum"], ref["accum"]
    swing = np.cumsum(ref["fragile"], 0) / float(ref["smp"])
    diff = np.abs(acc[..., 0] - racc[..., 0])
    calm = swing == 0
    print(f"{label} [{build}] {dev['info']['traversal']}: depth equal {np.array_equal(d, rd)}, max rel {rel.max():.3e} | accumulation: non-fragile max |d| {diff[calm].max():.3e}, "
          f"fragile pixels {int((~calm[-1]).sum())} with max |d| {diff[~calm].max() if (~calm).any() else 0:.3e}, max excess over the swing {np.maximum(diff - swing, 0).max():.3e} (ROUND {ROUND[build]:.2e})")
    assert np.array_equal(d > 0, rd > 0)                                     # the same pixels have a depth at all
    if exact:
        assert np.array_equal(d, rd)                                         # (every pixel's hit count matches: the traversal is the reference's loop)
    else:
        assert rel.max() <= DEPTH_REL
    assert not acc[..., 1].any() and all(np.array_equal(a[..., 2], d) for a in acc)      # channel 1 zero, channel 2 the depth map
    assert (diff[calm] <= ROUND[build]).all()
    assert (diff <= swing + ROUND[build]).all()
    cnt = float(ref["spp"])
    assert dev["cnt"] == ref["spp"]
    assert np.array_equal(dev["pixels"] == 0, ref["pixels"] == 0)           # the last call's ray decides, pixel by pixel
    assert (np.abs(dev["pixels"] - ref["pixels"]) <= (swing[-1] + ROUND[build])[..., None] / cnt + 1e-7).all()
    assert np.array_equal(dev["pixels"][..., 0], dev["pixels"][..., 1]) and np.array_equal(dev["pixels"][..., 0], dev["pixels"][..., 2])


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", list(AM.FIXTURES))
def test_fixture_case(name, build, parsed):
    dev = device_run(name, build, parsed)
    assert dev["info"]["pipeline"] == "ao" and "ambient occlusion" in dev["info"]["shade_variant"]
    hold(dev, reference(name, build, parsed), build, name)


def test_last_call_missed_rule_is_exercised(parsed):
    """some fixture pixel was hit by an earlier call and missed by the last: `pixels` is 0 there although channel 0 is not"""
    seen = 0
    for name in AM.FIXTURES:
        dev = device_run(name, "exact", parsed)
        seen += int(((dev["pixels"][..., 0] == 0) & (dev["accum"][-1][..., 0] != 0)).sum())
    assert seen > 0


@pytest.mark.parametrize("build,traversal", [("fast", "flat"), ("fast", "sweep"), ("fast", "tile"), ("fast", "bvh"), ("exact", "sweep"), ("exact", "tile"), ("exact", "bvh")])
def test_every_traversal_on_cbox(build, traversal, parsed, monkeypatch):
    dev = device_run("cbox", build, parsed, traversal=traversal, monkeypatch=monkeypatch)
    assert dev["info"]["traversal"] == traversal
    hold(dev, reference("cbox", build, parsed), build, f"cbox/{traversal}")


@pytest.mark.parametrize("build", BUILDS)
def test_bvh_walk_on_a_mesh_scene_against_the_model(build, parsed):
    dev = device_run("bunnies1", build, parsed)
    assert dev["info"]["traversal"] == "bvh"
    hold(dev, reference("bunnies1", build, parsed), build, "bunnies1")


@pytest.mark.parametrize("build", BUILDS)
def test_film_that_is_no_multiple_of_a_wave(build, parsed):
    hold(device_run("cbox_50x30", build, parsed), reference("cbox_50x30", build, parsed), build, "cbox_50x30")


@pytest.mark.parametrize("build", BUILDS)
def test_repeat_runs_and_batch_splits_give_the_same_bits(build, parsed):
    ref = reference("cbox_smp33", build, parsed)
    one_by_one = device_run("cbox_smp33", build, parsed)
    runs = []
    for per_batch in (1, 2, 0, 0):
        rdr = AORenderer(*ref["scene"], exact=(build == "exact"), spp_per_batch=per_batch, **ref["kw"])
        rdr.render(n_spp=ref["spp"])
        runs.append((rdr.depth_map(), rdr.color.to_numpy(), rdr.pixels.to_numpy()))
        rdr.close()
    for depth, accum, pixels in runs:
        assert np.array_equal(depth, one_by_one["depth"]) and np.array_equal(accum, one_by_one["accum"][-1]) and np.array_equal(pixels, one_by_one["pixels"])


@pytest.mark.parametrize("build", BUILDS)
def test_checkpoint_reset_and_clear(build, parsed):
    ref = reference("cbox_crop", build, parsed)
    whole = device_run("cbox_crop", build, parsed)
    make = lambda: AORenderer(*ref["scene"], exact=(build == "exact"), **ref["kw"])
    a = make()
    a.render(0, 0, 0, 0, 0, 0)
    ck = a.get_check_point()
    assert ck["counter"] == 1 and np.array_equal(ck["accumulation"], whole["accum"][0]) and "aov_sums" not in ck
    # upstream's reset is an empty kernel: nothing moves
    a.reset()
    assert a.cnt[None] == 1 and np.array_equal(a.color.to_numpy(), whole["accum"][0])
    # a checkpoint carries the depth map in channel 2: a renderer handed another map renders on with it
    b = make()
    moved = ck["accumulation"].copy(); moved[..., 2] *= np.float32(0.5)
    b.load_check_point({**ck, "accumulation": moved})
    assert np.array_equal(b.depth_map(), moved[..., 2]) and b.cnt[None] == 1
    b.load_check_point(ck)
    assert np.array_equal(b.depth_map(), whole["depth"]) and np.array_equal(b.pixels.to_numpy()[..., 0], whole["accum"][0][..., 0])      # (after a load every pixel shows)
    b.render(0, 0, 0, 0, 0, 0)
    assert b.cnt[None] == 2 and np.array_equal(b.color.to_numpy(), whole["accum"][1]) and np.array_equal(b.pixels.to_numpy(), whole["pixels"])
    # clear(): channel 0 and the counter start over, the depth map stays, and the render repeats bit for bit
    b.clear()
    zeroed = b.color.to_numpy()
    assert b.cnt[None] == 0 and not zeroed[..., :2].any() and np.array_equal(zeroed[..., 2], whole["depth"]) and not b.pixels.to_numpy().any()
    assert np.array_equal(b.depth_map(), whole["depth"])
    b.render(n_spp=2)
    assert np.array_equal(b.color.to_numpy(), whole["accum"][1]) and np.array_equal(b.pixels.to_numpy(), whole["pixels"])
    assert b.summary().startswith("SSAO SPP = 2")
    a.close(); b.close()


def test_refusals_name_their_limit(parsed):
    scene = parsed("cbox")
    kw = {"width": 16, "height": 12, "depth_samples": 1, "smp_hemisphere": 1}
    for extra, words in (({"volumetric": True}, "ambient occlusion is a surface-renderer mode"),
                         ({"transient": {"sample_count": 4, "min_time": 0.0, "interval": 1.0}}, "ambient occlusion and transient rendering do not combine"),
                         ({"path_lengths": True}, "ambient occlusion and path-length images do not combine"),
                         ({"light_groups": True}, "ambient occlusion and light groups do not combine"),
                         ({"adaptive": {"threshold": 0.05}}, "ambient occlusion and adaptive sampling do not combine"),
                         ({"world_size": 2, "rank": 0}, "depth-map lookups cross the column shards"),
                         ({"smp_hemisphere": 0}, "ao_smp_hemisphere > 0"),
                         ({"sample_extent": float("nan")}, "finite ao_sample_extent")):
        with pytest.raises(AptError, match=words):
            AORenderer(*scene, **{**kw, **extra})
    with pytest.raises(ValueError, match="aov_spp must be 0"):
        AORenderer(*scene, aov_spp=4, **kw)
    rdr = AORenderer(*scene, **kw)
    with pytest.raises(AptError, match=r"apt_render_aov: feature buffers and the denoiser belong to the path tracer \(ao = 0\)"):
        rdr.aov()
    rdr.close()


@pytest.mark.parametrize("cls", [Renderer])
def test_depth_map_entry_refuses_a_path_tracer(cls, parsed):
    import ctypes as C
    rdr = cls(*parsed("cbox"), width=16, height=12)
    out = np.zeros((16, 12), np.float32)
    rc = rdr.lib.apt_read_ao_depth(rdr.handle, out.ctypes.data_as(_lib.f32p))
    assert rc == -5 and rdr.lib.apt_last_error().decode() == "apt_read_ao_depth: the renderer was created with ao = 0"
    assert rdr.lib.apt_read_ao_depth(None, out.ctypes.data_as(_lib.f32p)) == -1
    assert "pipeline" not in rdr.info()
    rdr.close()
