"""The direct-light viewer on the device, both builds, against the fixtures the reference's direct_render.py produced
(tests/golden/direct_*.npz) and, where there is no fixture, against the numpy model that reproduces them bit for bit (tests/direct_model.py).

Exact build: depth map and normal map bit for bit, the set of occluded pixels equal to the model's, `pixels` within PIXEL_REL relative.
PIXEL_REL is 4 x the largest |device - fixture| / (|fixture| + 1e-30) measured over every fixture case, light position and traversal on an
MI355X: measured 0 - every word of every frame equal (the device's pow, evaluated in double and rounded once, and glibc's powf, which made
the fixtures, agree on every argument the fixtures hold) - so the bound is 0 as well: bit for bit.
Product build: depth within 1e-5 (1 + t), at least 99 % of a frame's pixels within 1e-3 (1 + x) per channel, relMSE <= 1e-4
over them.  tests/test_direct_host.py keeps the reference's own coin tosses (float32 against float64) below 0.25 % of every case's pixels."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import direct_model as DM
from adapt_amd import _lib
from adapt_amd._lib import AptError
from adapt_amd.renderer import BlinnPhongTracer, Renderer

pytestmark = pytest.mark.gpu

BUILDS = ["exact", "fast"]
PIXEL_REL = 4 * 0.0
_model, _device = {}, {}
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def case(name, parsed):
    """(scene for BlinnPhongTracer, positions (F, 3), what the device is held to: depth, normal, pixels (F, w, h, 3), occluded, lit)"""
    if name not in _model:
        if name in DM.FIXTURES:
            fx = DM.load_fixture(name)
            scene, pos = DM.scene_for(fx, parsed(DM.FIXTURES[name])), fx["positions"]
        else:                                                 # the BVH walk: tests/test_gpu_ao.py's mesh scene; no fixture, the model stands in
            from adapt_amd.synth import three_bunnies
            em, arr, objs, prop = three_bunnies(levels=1)
            prop = dict(prop); prop["film"] = dict(prop["film"], width=24, height=24)
            scene, fx = (DM.point_emitter((9.0, 10.0, 12.0)), arr, objs, prop), None
            cam = np.float32(prop["transform"][1])
            lo, hi = arr["primitives"].reshape(-1, 3).min(0), arr["primitives"].reshape(-1, 3).max(0)
            pos = np.float32([cam + np.float32([0.3, 0.4, 0.0]), (lo + hi) / 2 + np.float32([0.0, 0.45, 0.0]) * (hi - lo)])
        m = DM.DirectModel(*scene)
        parts = [m.render_parts(e) for e in pos]
        _model[name] = {"scene": scene, "positions": np.float32(pos), "depth": fx["depth_map"] if fx else m.depth_map, "normal": fx["norm_map"] if fx else m.norm_map,
                        "pixels": fx["pixels"] if fx else np.stack([p[0] for p in parts]), "occluded": np.stack([p[1] for p in parts]), "lit": np.stack([p[2] for p in parts])}
    return _model[name]


def device_run(name, build, parsed, traversal=None, monkeypatch=None):
    key = (name, build, traversal)
    if key not in _device:
        ref = case(name, parsed)
        if traversal:
            monkeypatch.setenv("APT_TRAVERSAL", traversal)
        bpt = BlinnPhongTracer(*ref["scene"], exact=(build == "exact"))
        before = bpt.pixels.to_numpy()
        frames = bpt.render_sweep(ref["positions"])
        _device[key] = {"info": bpt.info(), "depth": bpt.depth_map.to_numpy(), "normal": bpt.norm_map.to_numpy(), "frames": frames,
                        "last": bpt.pixels.to_numpy(), "before": before, "cnt": bpt.cnt[None]}
        bpt.close()
    return _device[key]


def hold(dev, ref, build, label):
    """the comparisons of a case; prints the figures before it asserts"""
    d, rd = dev["depth"], ref["depth"]
    rel_t = np.abs(d - rd) / (1 + rd)
    occ = np.stack([DM.occluded_in(f, lit)[0] for f, lit in zip(dev["frames"], ref["lit"])])
    decidable = np.stack([DM.occluded_in(f, lit)[1] for f, lit in zip(dev["frames"], ref["lit"])])
    flips = int(((occ != ref["occluded"]) & decidable).sum())
    a, b = dev["frames"].astype(np.float64), ref["pixels"].astype(np.float64)
    rel_px = (np.abs(a - b) / (np.abs(b) + 1e-30)).max()
    within = np.all(np.abs(a - b) <= 1e-3 * (1 + np.abs(b)), axis=-1)
    frac = within.reshape(len(a), -1).mean(1)
    rel_mse = [float(np.mean((x[w] - y[w]) ** 2 / (y[w] ** 2 + 1e-2))) for x, y, w in zip(a, b, within)]
    print(f"{label} [{build}] {dev['info']['traversal']}: depth equal {np.array_equal(d, rd)}, max |dt| / (1 + t) {rel_t.max():.3e}, normal equal {np.array_equal(dev['normal'], ref['normal'])} | "
          f"shadow flags that differ {flips} of {int(decidable.sum())} | pixels: max relative {rel_px:.3e}, within 1e-3 (1 + x) {frac.min():.4f}, relMSE over them {max(rel_mse):.3e}")
    assert dev["cnt"] == 0 and not dev["before"].any()                        # cnt never moves; before the first call the frame is zero
    assert np.array_equal(d > 0, rd > 0)
    assert np.array_equal(dev["last"], dev["frames"][-1])                     # apt_read_pixels holds the last frame
    if build == "exact":
        assert np.array_equal(d, rd) and np.array_equal(dev["normal"], ref["normal"])
        assert flips == 0
        assert rel_px <= PIXEL_REL
    else:
        assert rel_t.max() <= 1e-5
        assert np.abs(dev["normal"] - ref["normal"]).max() <= 1e-5            # (sphere normals come from the hit point)
        assert frac.min() >= 0.99 and max(rel_mse) <= 1e-4


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", list(DM.FIXTURES))
def test_fixture_case(name, build, parsed):
    dev = device_run(name, build, parsed)
    assert dev["info"]["pipeline"] == "direct" and "direct-light viewer" in dev["info"]["shade_variant"]
    hold(dev, case(name, parsed), build, name)


@pytest.mark.parametrize("build,traversal", [("fast", "flat"), ("fast", "sweep"), ("fast", "tile"), ("fast", "bvh"), ("exact", "sweep"), ("exact", "tile"), ("exact", "bvh")])
def test_every_traversal_on_cbox(build, traversal, parsed, monkeypatch):
    dev = device_run("cbox", build, parsed, traversal=traversal, monkeypatch=monkeypatch)
    assert dev["info"]["traversal"] == traversal
    hold(dev, case("cbox", parsed), build, f"cbox/{traversal}")


@pytest.mark.parametrize("build", BUILDS)
def test_bvh_walk_on_a_mesh_scene_against_the_model(build, parsed):
    dev = device_run("bunnies1", build, parsed)
    assert dev["info"]["traversal"] == "bvh"
    hold(dev, case("bunnies1", parsed), build, "bunnies1")


@pytest.mark.parametrize("build", BUILDS)
def test_sweeps_equal_single_calls_in_any_order(build, parsed, monkeypatch):
    ref = case("cbox", parsed)
    whole = device_run("cbox", build, parsed)
    pos = ref["positions"]
    bpt = BlinnPhongTracer(*ref["scene"], exact=(build == "exact"))
    single = []
    for e in pos:
        bpt.render(e)
        single.append(bpt.pixels.to_numpy())
    for f in range(len(pos)):
        assert np.array_equal(single[f], whole["frames"][f])
    for order in ([2], [4, 0], [3, 1, 4, 0, 2], [3, 1, 4, 0, 2]):            # 1, 2 and 5 positions; the last one twice: two runs are bit-identical
        out = bpt.render_sweep(pos[order])
        assert out.shape == (len(order), bpt.w, bpt.h, 3)
        assert all(np.array_equal(out[k], single[f]) for k, f in enumerate(order))
        assert np.array_equal(bpt.pixels.to_numpy(), single[order[-1]])
    assert np.array_equal(bpt.depth_map.to_numpy(), whole["depth"]) and bpt.cnt[None] == 0
    bpt.reset()
    assert np.array_equal(bpt.pixels.to_numpy(), single[2])                   # reset is a no-op, as upstream's
    with pytest.raises(NotImplementedError, match="Checkpoint saver is not implemented in TracerBase"):
        bpt.get_check_point()
    bpt.close()
    # a frame buffer that holds 2 frames: 5 positions in 3 launches, the same bits
    monkeypatch.setenv("APT_DIRECT_CHUNK", "2")
    bpt = BlinnPhongTracer(*ref["scene"], exact=(build == "exact"))
    out = bpt.render_sweep(pos)
    assert np.array_equal(out, whole["frames"]) and np.array_equal(bpt.pixels.to_numpy(), single[4])
    bpt.close()


def test_a_path_tracer_is_untouched_by_a_viewers_lifetime(parsed):
    scene = parsed("cbox")
    rdr = Renderer(*scene, width=32, height=24, spp_per_batch=2)
    rdr.render(n_spp=2)
    before = rdr.color.to_numpy()
    ref = case("cbox", parsed)
    bpt = BlinnPhongTracer(*ref["scene"])
    bpt.render(ref["positions"][0])
    rdr.render(n_spp=2)
    during = rdr.color.to_numpy()
    bpt.close()
    rdr.clear()
    rdr.render(n_spp=2)
    assert np.array_equal(rdr.color.to_numpy(), before)
    rdr.render(n_spp=2)
    assert np.array_equal(rdr.color.to_numpy(), during)
    rdr.close()


def test_refusals_name_their_limit(parsed):
    ref = case("cbox", parsed)
    em, arr, objs, prop = ref["scene"]

    class Odd(BlinnPhongTracer):
        extra = {}

        def _configure(self, cfg, prop):
            super()._configure(cfg, prop)
            for k, v in self.extra.items():
                setattr(cfg, k, v)

    for extra, words in (({"volumetric": 1}, "the direct-light viewer is a surface-renderer mode"),
                         ({"ao": 1, "ao_smp_hemisphere": 1, "ao_depth_samples": 1, "ao_sample_extent": 0.1}, "the direct-light viewer and ambient occlusion do not combine"),
                         ({"transient_bins": 4, "transient_interval": 1.0}, "the direct-light viewer and transient rendering do not combine"),
                         ({"path_lengths": 1}, "the direct-light viewer and path-length images do not combine"),
                         ({"light_groups": 1}, "the direct-light viewer and light groups do not combine"),
                         ({"adaptive_threshold": 0.05, "adaptive_min_spp": 8, "adaptive_step": 8}, "the direct-light viewer and adaptive sampling do not combine"),
                         ({"world_size": 2}, r"the direct-light viewer runs on one rank \(world_size = 1\)"),
                         ({"direct": 2}, r"direct must be 0 \(off\) or 1")):
        Odd.extra = extra
        with pytest.raises(AptError, match=words):
            Odd(em, arr, objs, prop)
    bpt = BlinnPhongTracer(em, arr, objs, prop)
    lib, h = bpt.lib, bpt.handle
    good = np.float32([[1.0, 2.0, 3.0]])
    film = np.zeros((bpt.w, bpt.h, 3), np.float32)
    for call, message in ((lambda: lib.apt_render(h, 1), "apt_render: a direct-light viewer takes no samples"),
                          (lambda: lib.apt_set_accum(h, film.ctypes.data_as(_lib.f32p), 0), "apt_set_accum: a direct-light viewer keeps no accumulation"),
                          (lambda: lib.apt_get_accum(h, film.ctypes.data_as(_lib.f32p), None), "apt_get_accum: a direct-light viewer keeps no accumulation")):
        assert call() == -5 and lib.apt_last_error().decode().startswith(message)
    for n, pos, message in ((0, good, "apt_render_direct: needs n >= 1 light positions"), (-1, good, "apt_render_direct: needs n >= 1 light positions"),
                            (1, np.float32([[0.0, float("nan"), 0.0]]), "apt_render_direct: a light position has a non-finite coordinate"),
                            (1, np.float32([[float("inf"), 0.0, 0.0]]), "apt_render_direct: a light position has a non-finite coordinate")):
        assert lib.apt_render_direct(h, pos.ctypes.data_as(_lib.f32p), n, None) == -1 and lib.apt_last_error().decode() == message
    assert lib.apt_render_direct(h, None, 1, None) == -1
    assert lib.apt_reset(h) == 0 and lib.apt_read_direct_maps(h, None, None) == 0
    with pytest.raises(AptError, match=r"belong to the path tracer \(direct = 0\)"):
        bpt.aov()
    bpt.close()
    # the viewer's entries on a path tracer
    rdr = Renderer(*parsed("cbox"), width=16, height=12)
    assert rdr.lib.apt_render_direct(rdr.handle, good.ctypes.data_as(_lib.f32p), 1, None) == -5
    assert rdr.lib.apt_last_error().decode() == "apt_render_direct: the renderer was created with direct = 0"
    assert rdr.lib.apt_read_direct_maps(rdr.handle, None, None) == -5
    assert rdr.lib.apt_last_error().decode() == "apt_read_direct_maps: the renderer was created with direct = 0"
    assert rdr.lib.apt_render_direct(None, good.ctypes.data_as(_lib.f32p), 1, None) == -1
    rdr.close()


def png_size(path):
    with open(path, "rb") as f:
        head = f.read(24)
    assert head[:8] == b"\x89PNG\r\n\x1a\n"
    return struct.unpack(">II", head[16:24])


@pytest.mark.parametrize("positions,names", [([], ["phong.png"]), (["2.78,4.5,3.0", "1.0,5.0,-1.0"], ["phong_000.png", "phong_001.png"])])
def test_command_line_end_to_end(positions, names, tmp_path):
    cmd = [sys.executable, "-m", "adapt_amd.direct_view", "--scene", "cbox", "--name", "c2_cbox.xml", "--input_path", os.path.join(ROOT, "scenes"),
           "--output_path", str(tmp_path), "--width", "32", "--height", "24"] + [a for p in positions for a in ("--emit_pos", p)]
    run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    assert sorted(os.listdir(tmp_path)) == sorted(names + ["depth.png", "normal.png"])
    for n in names + ["depth.png", "normal.png"]:
        assert png_size(os.path.join(tmp_path, n)) == (32, 24)
