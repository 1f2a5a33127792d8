"""The direct-light viewer without a device: the float32 numpy model (tests/direct_model.py) against every fixture the
reference's direct_render.py produced, the float64 model's verdict on how many pixels sit on an edge, and the host logic - what
BlinnPhongTracer refuses, what `python -m adapt_amd.direct_view` parses, and that the new kernels of the product build allocate no scratch."""
import os

import numpy as np
import pytest

import direct_model as DM

_models = {}


def model(name, parsed):
    if name not in _models:
        fx = DM.load_fixture(name)
        _models[name] = (DM.DirectModel(*DM.scene_for(fx, parsed(DM.FIXTURES[name]))), fx)
    return _models[name]


@pytest.mark.parametrize("name", list(DM.FIXTURES))
def test_float32_model_reproduces_the_fixture(name, parsed):
    m, fx = model(name, parsed)
    assert (m.w, m.h) == (fx["width"], fx["height"]) and fx["cnt"] == 0           # cnt never moves
    assert np.array_equal(m.depth_map, fx["depth_map"])
    assert np.array_equal(m.norm_map, fx["norm_map"])                             # (zero where nothing was hit: the field's initial value)
    for f, e in enumerate(fx["positions"]):
        px, _ = m.render(e)
        # bit for bit: the generator's pow is glibc's powf, which the model calls too (numpy's own float32 power differed by 1 ulp on 0.2 % of the values)
        assert np.array_equal(px, fx["pixels"][f]), (name, str(fx["position_names"][f]), float(np.abs(px - fx["pixels"][f]).max()))


@pytest.mark.parametrize("name", DM.SAME_AS_CBOX)
def test_crop_and_jitter_settings_change_nothing(name):
    """direct_render.py's loop has no crop test and TracerBase fixes anti_alias = False: the reference's own frames are the plain case's"""
    fx, plain = DM.load_fixture(name), DM.load_fixture("cbox")
    assert fx["crop"][2] > 0 or fx["anti_alias"]
    assert np.array_equal(fx["depth_map"], plain["depth_map"]) and np.array_equal(fx["norm_map"], plain["norm_map"])
    for f, e in enumerate(fx["positions"]):
        g = int(np.flatnonzero((plain["positions"] == e).all(1))[0])
        assert np.array_equal(fx["pixels"][f], plain["pixels"][g])


def test_fixtures_cover_what_they_are_there_for():
    cbox, tex, kg0, balls = (DM.load_fixture(n) for n in ("cbox", "textured", "features_a_kg0", "balls_mono"))
    assert list(cbox["position_names"]) == ["own", "wall", "outside", "behind", "graze"]
    wall = cbox["pixels"][1]
    assert wall.max() > 1e4 * cbox["pixels"][0].max()                             # 1 / (1e-5 + d^2) close to its cap next to the wall
    length = np.linalg.norm(tex["norm_map"], axis=-1)[tex["depth_map"] > 0]
    assert tex["has_vertex_normal"] and (np.abs(length - 1) > 1e-3).any()         # n_s is a mix of vertex normals, not normalised
    assert (kg0["kg"][:, 1:] == 0).any()                                          # a zero channel of k_g: pow(0, 0) = 1
    assert (cbox["depth_map"] == 0).any() and not cbox["norm_map"][cbox["depth_map"] == 0].any()
    assert 50 * 30 % 64 == 28 and DM.load_fixture("cbox_50x30")["depth_map"].shape == (50, 30)
    assert balls["depth_map"].shape == (24, 24)


def test_pow_of_zero_to_zero_is_one_in_the_model(parsed):
    """features_a_kg0: where dot(h, n_s) <= 0 a channel with k_g = 0 keeps spec = 1 - the pixel is lit although the highlight is off"""
    m, fx = model("features_a_kg0", parsed)
    objs = [int(k) for k in fx["kg"][:, 0]]
    seen = 0
    for f, e in enumerate(fx["positions"]):
        px = fx["pixels"][f]
        for k, row in zip(objs, fx["kg"]):
            on = m.obj_map == k
            zero_ch, pos_ch = np.flatnonzero(row[1:] == 0), np.flatnonzero(row[1:] > 0)
            if len(zero_ch) and len(pos_ch):
                seen += int(((px[on][:, zero_ch[0]] > 0) & (px[on][:, pos_ch[0]] == 0)).sum())
    assert seen > 0


@pytest.mark.parametrize("name", [n for n in DM.FIXTURES if n not in DM.SAME_AS_CBOX])
def test_float64_disagrees_on_few_pixels(name, parsed):
    """The share is taken over the case: the pixels of all its frames.  What is left are the reference's own coin tosses - a shadow ray that
    starts on a sphere, a rounding error inside it, and leaves at a grazing angle crosses the sphere again beyond the 1e-4 gate in float32
    (2-3 pixels of balls_mono under any light) - and silhouette pixels of shadow edges."""
    m, fx = model(name, parsed)
    n, bad = m.w * m.h * len(fx["positions"]), 0
    for f, e in enumerate(fx["positions"]):
        hit_d, sh_d = m.edges(e)
        print(f"{name}/{fx['position_names'][f]}: hit object differs on {int(hit_d.sum())}, shadow flag on {int(sh_d.sum())} of {m.w * m.h} pixels")
        bad += int(hit_d.sum() + sh_d.sum())
    assert bad <= DM.EDGE_CAP * n


def test_refusals_name_upstreams_limit(parsed):
    from adapt_amd.renderer import BlinnPhongTracer, light_positions
    em, arr, objs, prop = parsed("features_a")
    area = next(e for e in em if e.type == "area")
    with pytest.raises(ValueError, match=r"only supports one point source \(renderer/direct_render.py:30\), got a 'area' emitter"):
        BlinnPhongTracer(area, arr, objs, prop)
    with pytest.raises(ValueError, match=r"only supports one point source .* got 5 emitters"):
        BlinnPhongTracer(em, arr, objs, prop)
    with pytest.raises(ValueError, match="finite"):
        light_positions([0.0, float("nan"), 1.0])
    with pytest.raises(ValueError, match=r"expected \(3,\) or \(F, 3\)"):
        light_positions([[0.0, 1.0]])
    assert light_positions([1, 2, 3]).shape == (1, 3) and light_positions(np.zeros((4, 3))).dtype == np.float32


def test_direct_view_arguments():
    import argparse
    from adapt_amd import direct_view as dv
    o = dv.parse_args([])
    assert (o.scene, o.name, o.emit_pos, o.exact, o.width, o.device) == ("cbox", "c2_cbox.xml", [], False, None, 0)
    o = dv.parse_args(["--emit_pos", "1,2.5,-3", "--emit_pos", "0,0,1e-3", "--width", "32", "--height", "24", "--exact", "--output_path", "x"])
    assert np.array_equal(np.stack(o.emit_pos), np.float32([[1, 2.5, -3], [0, 0, 1e-3]])) and o.exact and (o.width, o.height, o.output_path) == (32, 24, "x")
    for bad in ("1,2", "1,2,x", "1,2,nan", "1,2,3,4"):
        with pytest.raises(argparse.ArgumentTypeError):
            dv.parse_position(bad)
    assert dv.output_names(1, "png") == ["phong.png"] and dv.output_names(3, "npy") == ["phong_000.npy", "phong_001.npy", "phong_002.npy"]
    depth, normal = dv.map_images(np.float32([[0, 2], [4, 1]]), np.float32(np.full((2, 2, 3), -1)))
    assert depth.shape == (2, 2, 3) and depth.max() == 1 and depth[0, 1, 0] == 0.5 and not normal.any()
    assert not dv.map_images(np.zeros((2, 2), np.float32), np.zeros((2, 2, 3), np.float32))[0].any()        # nothing hit: no division by zero


def test_new_entries_are_declared_everywhere():
    from adapt_amd import _lib
    names = [f[0] for f in _lib.RenderCfg._fields_]
    k = names.index("volumetric")
    assert names[k - 3:k + 2] == ["profile", "direct", "direct_intensity", "volumetric", "ao"]      # before every block added earlier; `volumetric` stays the ao block's neighbour (tests/test_ao_host.py)
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "adapt_mi.h")).read()
    for sym in ("apt_render_direct", "apt_read_direct_maps"):
        assert sym in _lib.SYMBOLS and f"int {sym}(" in header


DIRECT_HEADERS = ("include/adapt_mi.h", "adapt_amd/csrc/bvh_build.hpp", "adapt_amd/csrc/direct.hpp")
ARGS = "(DevScene, Params, DirectQ, LdsPlan)"
INSTANCES = [f"k_direct_{what}<{mode}>{ARGS}" for what in ("hit", "shade") for mode in ("TRACE_BVH", "TRACE_SWEEP", "TRACE_TILE")]
# mangled prefixes: the three template kernels per pass by traversal, and the flat sweep's pair (plain functions: the header alone emits them)
KERNELS = {f"{what}<{name}>": f"_Z{len('k_direct_' + what)}k_direct_{what}ILi{mode}E" for what in ("hit", "shade") for mode, name in enumerate(("bvh", "sweep", "tile"))}
KERNELS.update({"hit_flat": "_Z17k_direct_hit_flat", "shade_flat": "_Z19k_direct_shade_flat"})


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_product_build_kernels_allocate_no_scratch(kernel):
    """compiled for gfx950 with the product build's flags (tests/kernel_probe.py): no scratch, hence no spilled register either"""
    from kernel_probe import compile_probe, resources
    r = resources(compile_probe(INSTANCES, headers=DIRECT_HEADERS), KERNELS[kernel])
    print(f"k_direct_{kernel} [fast]: {r}")
    assert r["scratch"] == 0 and r["spilled"] == 0
