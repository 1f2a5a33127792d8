"""The CPU oracle (oracle/pt_oracle.c) against fixtures recorded from the REFERENCE's own source
(tests/golden/gen: unchanged /root/reference code run under a float32 stand-in for the absent taichi
package, same libm, RNG wired to the shared Philox stream).  Arithmetic is float32 on both sides in the
same operation order, so the bar here is bit equality; the one allowed slack is stated where used."""
import os

import numpy as np
import pytest

from conftest import SCENES, golden
from gpu_cases import bvhref_scene
from adapt_amd.scene_pack import make_config
from oracle import binding as ob

F = golden("functions.npz")


def same(a, b):
    """bit equality, NaN == NaN (the fresnel-blend pdf is NaN for some geometries, upstream too)"""
    return np.array_equal(np.asarray(a, np.float32), np.asarray(b, np.float32), equal_nan=True)


def test_rotation_between_bit_exact():
    for a, b, R in zip(F["rot_a"], F["rot_b"], F["rot_R"]):
        assert np.array_equal(ob.rotation_between(a, b), R)


def test_fresnel_known_answer_and_vectors():
    assert ob.fresnel_equation(1.0, 1.5, 1.0, 1.0) == pytest.approx(0.04, abs=1e-7)     # ((1-1.5)/(1+1.5))^2
    for x, y in zip(F["fresnel_in"], F["fresnel_out"]):
        assert np.float32(ob.fresnel_equation(*map(float, x))) == y


# microfacet_functions.npz: the reference's Trowbridge-Reitz BRDF (type 3), recorded with its `__ENABLE_MICROFACET__` switch on
@pytest.mark.parametrize("fixture", ["functions.npz", "microfacet_functions.npz"])
def test_bxdf_eval_pdf_bit_exact(fixture):
    g = golden(fixture)
    mi, mf = g["mat_i"], g["mat_f"]
    nonzero = 0
    for x, y in zip(g["eval_in"], g["eval_out"]):
        m = int(x[0])
        ev, pdf = ob.bxdf_eval_pdf(mi[m], mf[m], 1.0, x[1:4], x[4:7], x[7:10], x[10:13])
        assert same(ev, y[:3]) and same(pdf, y[3]), (m, x, ev, pdf, y)
        nonzero += bool(np.any(y != 0))
    assert nonzero > 80          # the vectors exercise the non-trivial branches


@pytest.mark.parametrize("fixture", ["functions.npz", "microfacet_functions.npz"])
def test_bxdf_sample_bit_exact(fixture):
    g = golden(fixture)
    mi, mf = g["mat_i"], g["mat_f"]
    lit = 0
    for k, (x, y) in enumerate(zip(g["sample_in"], g["sample_out"])):
        m = int(x[0])
        d, s, pdf, spec, nd = ob.bxdf_sample(mi[m], mf[m], 1.0, x[1:4], x[4:7], x[7:10], None, key=k, seed=777)
        assert same(d, y[:3]) and same(s, y[3:6]) and same(pdf, y[6]), (m, k, d, s, pdf, y)
        assert spec == bool(y[7]) and nd == int(y[8])
        lit += bool(np.any(y[3:6] != 0))
    assert lit > 80


@pytest.mark.parametrize("tag", ["cbox", "balls_mono", "glass_box", "features_a", "features_b", "features_c", "textured", "microfacet"])
def test_scene_functions_bit_exact(tag, parsed, oracle_scene):
    g = golden(f"scene_{SCENES[tag][2]}.npz")
    rc = make_config(parsed(tag)[3], width=int(g["width"]), height=int(g["height"]), max_bounce=int(g["max_bounce"]))
    sc = oracle_scene(tag)
    for x, y in zip(g["pix2ray_in"], g["pix2ray_out"]):
        assert np.array_equal(sc.pix2ray(rc, int(x[0]), int(x[1]), int(x[2]), x[3:5]), y)
    obj, prim, t, uv, ns = sc.intersect(g["ray_o"], g["ray_d"])
    h = g["ray_hit"]
    assert np.array_equal(obj, h[:, 0]) and np.array_equal(prim, h[:, 1]) and np.array_equal(t, h[:, 2])
    assert np.array_equal(uv, h[:, 3:5]) and np.array_equal(ns, h[:, 5:8])
    assert (obj >= 0).sum() > min(60, len(obj) // 2)
    assert np.array_equal(sc.occluded(g["ray_o"], g["ray_d"], g["ray_tmax"]), g["ray_occ"])
    for k, (x, y) in enumerate(zip(g["emit_in"], g["emit_out"])):
        pos, inten, pdf, nd = sc.src_sample_hit(int(x[0]), x[1:4], None, key=k, seed=778)
        le, sap = sc.src_eval(int(x[0]), x[7:10] * x[10], x[4:7], float(x[10]), x[7:10])
        assert same(pos, y[:3]) and same(inten, y[3:6]) and same(pdf, y[6]) and nd == int(y[7])
        assert same(le, y[8:11]) and same(sap, y[11])


@pytest.mark.parametrize("tag", ["cbox", "balls_mono", "glass_box", "features_a", "features_b", "features_c", "textured", "microfacet"])
def test_whole_kernel_matches_reference_run(tag, parsed, oracle_scene):
    """Renderer.render of the reference, spp by spp on the Philox stream, vs orc_render."""
    g = golden(f"scene_{SCENES[tag][2]}.npz")
    rc = make_config(parsed(tag)[3], width=int(g["width"]), height=int(g["height"]), max_bounce=int(g["max_bounce"]))
    assert rc.num_shadow_ray == int(g["num_shadow_ray"])
    sc = oracle_scene(tag)
    img, cnt, st = sc.render(rc, int(g["spp"]), threads=0)
    assert cnt == int(g["spp"]) and st["n_draws"] == int(g["draws"].sum())         # every path consumed the same number of randoms
    # first sample per pixel: colour and draw count
    W, H = rc.width, rc.height
    for i in range(0, W, 3):
        for j in range(0, H, 3):
            col, ev, nd = sc.trace_sample(rc, i, j, 1)
            assert np.array_equal(col, g["first_sample"][i, j]) and nd == g["draws"][0, i, j], (i, j)
    # bit equality, every pixel (the generator's scalars square by multiplication and take `%` as Taichi does: no slack needed)
    assert np.array_equal(img.view(np.uint32), g["accum"].view(np.uint32)) or np.array_equal(np.nan_to_num(img), np.nan_to_num(g["accum"]))
    assert np.array_equal(np.isnan(img), np.isnan(g["accum"]))
    np.testing.assert_array_equal(img / np.float32(cnt), img / np.float32(int(g["spp"])))


def test_texture_query_bit_exact(oracle_scene):
    """Texture.query of the reference (bilinear lookup inside the atlas rectangle, wrap at w-1 / h-1, coordinates outside
    [0, 1] and negative) on every declared map of scenes/test/textured.xml."""
    g = golden("scene_textured.npz")
    tin, tout = g["texq_in"], g["texq_out"]
    assert tin.shape[0] >= 100 and set(np.int32(tin[:, 0])) == {0, 1, 2}
    got = oracle_scene("textured").texture_query(tin[:, 0], tin[:, 1], tin[:, 2:4])
    assert np.array_equal(got.view(np.uint32), tout.view(np.uint32))          # exact, wrap seams included (`a % b` = a - b * floor(a / b) on both sides)


# ---- sweep over every pt-renderable scene file the reference bundles with its assets (tests/golden/refscene_*.npz)
from conftest import REF_SCENE_TAGS, VPT_SCENE_TAGS, scene_from_golden  # noqa: E402


@pytest.mark.parametrize("tag", REF_SCENE_TAGS)
def test_reference_bundled_scene_whole_kernel(tag):
    """The reference's parser output for one of ITS scene files (arrays in the fixture) rendered by the oracle equals the image
    and the per-sample draw counts the reference's own kernel produced on the same Philox stream."""
    from adapt_amd.scene_pack import make_config, pack_scene
    from oracle import binding as ob
    tup, g = scene_from_golden(tag)
    fs = pack_scene(*tup)
    for k in ("prims", "normals", "v_normals", "obj_info", "obj_aabb", "emitter_id", "bxdf_i", "bxdf_f", "src_i", "src_f"):
        assert np.array_equal(np.asarray(getattr(fs, k)).view(np.uint32), np.asarray(g[k]).view(np.uint32)), k     # the adapter is lossless
    rc = make_config(tup[3], seed=int(g["seed"]), use_bvh=False)
    osc = ob.OracleScene(fs, rc.cam_t)
    spp = int(g["spp"])
    acc, cnt, st = osc.render(rc, spp)
    ref = g["accum"]
    same = (acc.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(acc) & np.isnan(ref))
    assert same.all(), (tag, int((~same.all(axis=-1)).sum()))
    assert st["n_draws"] == int(g["draws"].sum())


@pytest.mark.skipif(not os.path.isdir("/root/reference/scenes"), reason="the reference tree exists in the authoring container only")
@pytest.mark.parametrize("tag", REF_SCENE_TAGS)
def test_own_parser_reads_the_reference_scene_files(tag):
    """adapt_amd's front end on the reference's own XML files yields the arrays the reference's parser yields."""
    from adapt_amd.parsers import scene_parsing
    from adapt_amd.scene_pack import pack_scene
    sdir, name = tag.split("_", 1)
    import glob
    cands = [f for f in glob.glob(f"/root/reference/scenes/{sdir}/*.xml") if os.path.basename(f)[:-4].replace("-", "_") == name]
    assert len(cands) == 1, (tag, cands)
    fs = pack_scene(*scene_parsing(os.path.dirname(cands[0]), os.path.basename(cands[0])))
    g = scene_from_golden(tag)[1]
    for k in ("prims", "normals", "v_normals", "obj_info", "obj_aabb", "emitter_id", "bxdf_i", "bxdf_f", "src_i", "src_f"):
        assert np.array_equal(np.asarray(getattr(fs, k)).view(np.uint32), np.asarray(g[k]).view(np.uint32)), (tag, k)


# ---- volumetric path tracer (renderer/vpt.py, homogeneous media): the reference's own vpt scenes through ITS VolumeRenderer.render
@pytest.mark.parametrize("tag", VPT_SCENE_TAGS)
def test_volumetric_whole_kernel_matches_reference_run(tag):
    """World medium (balls: spot light, volbox: area light) and an object medium behind a null surface (cbox): accumulated image
    and per-sample draw counts of VolumeRenderer.render on the shared Philox stream, bit for bit."""
    from adapt_amd.scene_pack import make_config, pack_scene
    tup, g = scene_from_golden(tag, "vptscene")
    fs = pack_scene(*tup)
    assert np.array_equal(fs.med_i, g["med_i"]) and np.array_equal(fs.med_f.view(np.uint32), g["med_f"].view(np.uint32))
    assert fs.has_scattering_media and int(g["volumetric"]) == 1
    rc = make_config(tup[3], seed=int(g["seed"]), use_bvh=False, volumetric=True)
    osc = ob.OracleScene(fs, rc.cam_t)
    acc, cnt, st = osc.render(rc, int(g["spp"]))
    ref = g["accum"]
    same = (acc.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(acc) & np.isnan(ref))
    assert same.all(), (tag, int((~same.all(axis=-1)).sum()))
    assert st["n_draws"] == int(g["draws"].sum()) and st["n_track"] >= st["n_shadow"] > 0
    # and the surface-only renderer on the same scene is a different estimator (media ignored): the flag matters
    acc0 = osc.render(make_config(tup[3], seed=int(g["seed"]), use_bvh=False), int(g["spp"]))[0]
    assert not np.array_equal(acc0, acc)


def test_medium_functions_bit_exact():
    """Medium.sample_mfp / sample_new_rays / eval / transmittance of the reference (ten media: H-G forward, isotropic and backward,
    three multi-H-G weightings, Rayleigh, mie, transparent, zero extinction in two channels) on the shared Philox stream."""
    g = golden("media_functions.npz")
    mi, mf = g["med_i"], g["med_f"]
    assert set(mi.tolist()) == {-1, 0, 1, 2, 3}
    events = 0
    for k, (x, y) in enumerate(zip(g["mfp_in"], g["mfp_out"])):
        m = int(x[0])
        out = ob.medium_probe(mi[m], mf[m], 0, [x[1]], key=k, seed=779)
        assert np.array_equal(out.view(np.uint32), y.view(np.uint32)), (m, k, out, y)
        events += int(y[0])
    assert 40 < events < 200                           # both outcomes of the free-path draw are exercised
    for k, (x, y) in enumerate(zip(g["scat_in"], g["scat_out"])):
        m = int(x[0])
        out = ob.medium_probe(mi[m], mf[m], 1, x[1:4], key=k, seed=780)
        assert np.array_equal(out.view(np.uint32), y.view(np.uint32)), (m, k, out, y)
    for k, (x, y) in enumerate(zip(g["eval_in"], g["eval_out"])):
        m = int(x[0])
        out = ob.medium_probe(mi[m], mf[m], 2, x[1:8])
        assert np.array_equal(out.view(np.uint32), y.view(np.uint32)), (m, k, out, y)


@pytest.mark.parametrize("tag", ["features_a", "features_b", "textured", "microfacet"])
def test_volumetric_loop_on_surface_scenes_matches_reference_run(tag, parsed, oracle_scene):
    """VolumeRenderer.render of the reference on surface-only scenes of this repo (every BRDF / BSDF / emitter type; two-sided BRDFs
    without RR and MIS; image textures): the volumetric loop differs from the surface tracer's even when nothing scatters."""
    g = golden(f"vptrun_{tag}.npz")
    w, h, spp = int(g["width"]), int(g["height"]), int(g["spp"])
    rc = make_config(parsed(tag)[3], width=w, height=h, seed=int(g["seed"]), volumetric=True)
    acc, cnt, st = oracle_scene(tag).render(rc, spp)
    ref = g["accum"]
    same = (acc.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(acc) & np.isnan(ref))
    assert same.all(), (tag, int((~same.all(axis=-1)).sum()))
    assert st["n_draws"] == int(g["draws"].sum())


@pytest.mark.parametrize("name", ["volgrid_a", "volgrid_b"])
def test_grid_volume_matches_reference_run(name):
    """Grid volumes (bxdf/volume.py): this repo's <volume> front end (own .vol reader, mono2rgb colour ramp, density scaling, toWorld)
    yields the record and the density grid the reference exports, bit for bit, and the oracle's delta tracking (free paths) / ratio
    tracking with roulette (light samples) reproduces VolumeRenderer.render of the reference - image and draw counts - with the volume
    in a clear world (A) and rotated inside a scattering world (B)."""
    from conftest import ROOT
    from adapt_amd.parsers.xml_parser import scene_parsing
    from adapt_amd.scene_pack import pack_scene
    g = golden(f"vptrun_{name}.npz")
    cwd = os.getcwd()
    os.chdir(ROOT)                              # the .vol path in the scene file is relative to the repository root
    try:
        tup = scene_parsing(os.path.join(ROOT, "scenes", "test"), name + ".xml")
        fs = pack_scene(*tup)
    finally:
        os.chdir(cwd)
    assert fs.has_volume and np.array_equal(fs.vol_i, g["vol_i"])
    assert np.array_equal(fs.vol_f.view(np.uint32), g["vol_f"].view(np.uint32))
    assert np.array_equal(fs.vol_grid.view(np.uint32), g["vol_grid"].view(np.uint32))
    rc = make_config(tup[3], width=int(g["width"]), height=int(g["height"]), seed=int(g["seed"]), volumetric=True)
    acc, cnt, st = ob.OracleScene(fs, rc.cam_t).render(rc, int(g["spp"]))
    ref = g["accum"]
    same = (acc.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(acc) & np.isnan(ref))
    assert same.all(), int((~same.all(axis=-1)).sum())
    assert st["n_draws"] == int(g["draws"].sum())
    # the volume matters: without it the same scene renders differently
    fs.vol_i = None
    acc0 = ob.OracleScene(fs, rc.cam_t).render(rc, int(g["spp"]))[0]
    assert not np.array_equal(acc0, acc)


# ---- the reference's BVH path (accelerator = bvh), tests/golden/bvhref_*.npz: the reference's OWN traversal code
# (PathTracer.bvh_process -> convert_bvh_info -> ray_intersect_bvh / does_intersect_bvh, tracer/path_tracer.py:143-179,338-422,
# tracer/ti_bvh.py) run on a reference-layout tree handed over by the `bvh_cpp` stand-in of the generator
@pytest.mark.parametrize("tag", ["cbox", "bunnies1", "bunnies3"])
def test_reference_bvh_traversal_bit_exact(tag):
    """Oracle's restatement of the reference's BVH walk == the reference's own walk on the same tree: closest hits (object,
    primitive, t, barycentrics, normals), occlusion flags, and - where recorded - the image and every sample's draw count."""
    tup, fs, g = bvhref_scene(tag)
    rc = make_config(tup[3], width=int(g["width"]), height=int(g["height"]), max_bounce=int(g["max_bounce"]), seed=int(g["seed"]))
    assert rc.use_bvh or tag == "cbox"
    sc = ob.OracleScene(fs, rc.cam_t, build_bvh=True)
    bvh_mm, node_mm, bvh_info, node_info = sc.bvh_arrays()
    assert str(g["tree_source"]) == "oracle" and node_info.shape[0] == int(g["node_num"]) and bvh_info.shape[0] == int(g["bvh_num"])
    if "node_info" in g:                        # small trees travel in the fixture: the tree the reference walked is this tree
        assert np.array_equal(node_info, g["node_info"]) and np.array_equal(bvh_info, g["bvh_info"])
        assert np.array_equal(node_mm, g["node_minmax"]) and np.array_equal(bvh_mm, g["bvh_minmax"])
    O, D, TM, h = g["ray_o"], g["ray_d"], g["ray_tmax"], g["bvh_hit"]
    obj, prim, t, uv, ns = sc.intersect(O, D, use_bvh=True)
    assert np.array_equal(obj, h[:, 0]) and np.array_equal(prim, h[:, 1]) and np.array_equal(t, h[:, 2])
    assert np.array_equal(uv, h[:, 3:5]) and np.array_equal(ns, h[:, 5:8])
    assert np.array_equal(sc.occluded(O, D, TM, use_bvh=True), g["bvh_occ"])
    assert (obj >= 0).sum() > 0.5 * len(O)
    if "accum" in g:
        rc.use_bvh = True
        img, cnt, st = sc.render(rc, int(g["spp"]))
        assert cnt == int(g["spp"]) and st["n_draws"] == int(g["draws"].sum())
        bad = (img.view(np.uint32) != g["accum"].view(np.uint32)) & ~(np.isnan(img) & np.isnan(g["accum"]))
        assert not bad.any(), int(bad.any(axis=2).sum())


@pytest.mark.parametrize("tag", ["cbox", "bunnies1", "bunnies3"])
def test_reference_brute_force_on_the_bvh_rays(tag):
    """The reference's brute-force intersector (tracer_base.py:168-278) on the first rays of the same batch, vs the oracle's
    brute force: bit-exact.  On the Cornell box and the 5 950-triangle scene the reference's two intersectors agree on every
    ray.  On the 95 050-triangle scene the batch starts with rays picked because the ORACLE's two intersectors disagree on
    them - and the reference's own two intersectors disagree on exactly those rays, in exactly the same way: its BVH walk
    (strict slab test on unpadded node boxes, ti_bvh.py:16-22, bvh_helper.h:30-45) loses hits its brute force finds."""
    tup, fs, g = bvhref_scene(tag)
    rc = make_config(tup[3])
    sc = ob.OracleScene(fs, rc.cam_t, build_bvh=True)
    hb, ob_ = g["brute_hit"], g["brute_occ"]
    n = hb.shape[0]
    O, D, TM = g["ray_o"][:n], g["ray_d"][:n], g["ray_tmax"][:n]
    obj, prim, t, uv, ns = sc.intersect(O, D, use_bvh=False)
    assert np.array_equal(obj, hb[:, 0]) and np.array_equal(prim, hb[:, 1]) and np.array_equal(t, hb[:, 2]) and np.array_equal(uv, hb[:, 3:5])
    assert np.array_equal(sc.occluded(O, D, TM, use_bvh=False), ob_)
    differ = (g["bvh_hit"][:n, 1] != hb[:, 1]) | (g["bvh_hit"][:n, 2] != hb[:, 2])
    occ_differ = g["bvh_occ"][:n] != ob_
    if tag != "bunnies3":
        assert not differ.any() and not occ_differ.any()
    else:
        # every lost closest hit is a hit the brute force finds NEARER (or at all); never the other way round
        assert differ.sum() >= 30 and (g["bvh_hit"][:n, 2][differ] > hb[:, 2][differ]).all()
        assert occ_differ.sum() >= 1 and (ob_[occ_differ] == 1).all()
        assert not differ[n // 2:].any()              # the second half of the picked rays are the undisputed controls
