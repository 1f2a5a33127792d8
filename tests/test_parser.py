"""Scene front end (adapt_amd/parsers) against dumps of the REFERENCE parser's output on its own scene files
(tests/golden/parse_*.npz, produced by tests/golden/gen/gen_goldens.py)."""
import os
import xml.etree.ElementTree as xet

import numpy as np
import pytest

from conftest import ROOT, SCENES, golden
from adapt_amd.parsers.general_parser import parse_str, rgb_parse, transform_parse, vec3d_parse
from adapt_amd.parsers.obj_loader import apply_transform, calculate_surface_area, extract_obj_info, read_obj
from adapt_amd.parsers.obj_desc import get_aabb
from adapt_amd.parsers.xml_parser import scene_parsing
from adapt_amd.scene_pack import fov2focal, make_config, np_rotation_between, pack_scene


@pytest.mark.parametrize("tag", ["cbox", "balls_mono", "glass_box"])
def test_parse_matches_reference_dump(tag, parsed, flat):
    g = golden(f"parse_{SCENES[tag][2]}.npz")
    em, arr, objs, cfg = parsed(tag)
    fs = flat(tag)
    for k in ("primitives", "n_g", "n_s", "uvs"):
        assert arr[k].dtype == np.float32 and np.array_equal(arr[k], g[k]), k
    idx = arr["indices"] if arr["indices"] is not None else np.int64([])
    assert np.array_equal(idx, g["indices"])
    assert np.array_equal(fs.obj_aabb, g["aabb"])
    assert np.array_equal(fs.obj_info[:, 1], g["tri_num"]) and np.array_equal(fs.obj_info[:, 2], g["obj_type"])
    assert np.array_equal(fs.obj_info[:, 0], np.concatenate([[0], np.cumsum(g["tri_num"])[:-1]]))
    assert np.array_equal(fs.emitter_id, g["emitter_ref"])
    assert np.array_equal(fs.bxdf_i[:, 0], g["bxdf_type"]) and np.array_equal(fs.bxdf_i[:, 1], g["bxdf_delta"])
    assert np.array_equal(fs.bxdf_i[:, 2], g["bxdf_is_bsdf"])
    assert np.array_equal(fs.bxdf_f[:, 0:3], g["k_d"]) and np.array_equal(fs.bxdf_f[:, 3:6], g["k_s"]) and np.array_equal(fs.bxdf_f[:, 6:9], g["k_g"])
    assert np.array_equal(fs.bxdf_f[:, 12], g["ior"])
    assert np.array_equal(fs.src_f[:, 0:3], g["src_intensity"]) and np.array_equal(fs.src_f[:, 9], g["src_inv_area"])
    assert [e.type for e in em] == list(g["src_type"])
    rc = make_config(cfg)
    assert np.array_equal(rc.cam_r, g["cam_r"]) and np.array_equal(rc.cam_t, g["cam_pos"])
    assert rc.focal == float(g["focal"])
    assert fs.has_vertex_normal == bool(g["has_vertex_normal"]) and fs.world_ior == float(g["world_ior"])
    assert cfg["num_shadow_ray"] == int(g["num_shadow_ray"])
    # area emitters point back at the object they are attached to
    for s in range(fs.n_sources):
        if fs.src_i[s, 0] == 1:
            assert fs.emitter_id[fs.src_i[s, 2]] == s


@pytest.mark.skipif(not os.path.isdir("/root/reference/scenes"), reason="reference tree only exists in the authoring container")
@pytest.mark.parametrize("d,f,tag", [("cbox", "cbox.xml", "cbox"), ("csphere", "balls-mono.xml", "balls_mono"), ("cbox", "complex.xml", "complex")])
def test_reference_scene_files_load_unchanged(d, f, tag):
    """Drop-in: the reference's own XML files parse to the same arrays as its own parser produced."""
    g = golden(f"parse_{tag}.npz")
    em, arr, objs, cfg = scene_parsing(os.path.join("/root/reference/scenes", d), f)
    assert np.array_equal(arr["primitives"], g["primitives"]) and np.array_equal(arr["n_s"], g["n_s"])
    assert cfg["max_bounce"] == int(g["max_bounce"]) and cfg["film"]["width"] == int(g["width"])


def test_known_answers():
    # SURVEY §4.3 analytic pins
    assert abs(fov2focal(39.3077, 512) - 716.79898) < 1e-4
    assert abs(rgb_parse(xet.fromstring('<rgb value="#BCBCBC"/>'))[0] - 0.7372549) < 1e-7
    np.testing.assert_array_equal(rgb_parse(xet.fromstring('<rgb r="10" g="1000"/>')), np.float32([10, 1000, 0]))
    np.testing.assert_array_equal(rgb_parse(xet.fromstring('<rgb value="0.25"/>')), np.float32([0.25] * 3))
    np.testing.assert_array_equal(parse_str("1, 2,3"), np.float32([1, 2, 3]))
    np.testing.assert_array_equal(parse_str("1 2 3"), np.float32([1, 2, 3]))
    with pytest.raises(ValueError):
        parse_str("1.0", no_else_branch=True)
    with pytest.raises(ValueError):
        rgb_parse(xet.fromstring("<rgb/>"))
    np.testing.assert_array_equal(vec3d_parse(xet.fromstring('<point x="1" z="3"/>')), np.float32([1, 0, 3]))
    d, o, s = transform_parse(xet.fromstring('<transform><lookat target="2.78, 2.73, -7.99" origin="2.78, 2.73, -8.00"/></transform>'))
    np.testing.assert_allclose(d, [0, 0, 1], atol=1e-6)
    assert s is None and o.dtype == np.float32
    with pytest.raises(ValueError):
        transform_parse(xet.fromstring('<transform><lookat target="1,1,1" origin="1,1,1"/></transform>'))
    with pytest.raises(ValueError):
        transform_parse(xet.fromstring('<transform><shear/></transform>'))
    # fresnel-blend cached coefficient: sqrt(11 * 1001) / 8pi
    from adapt_amd.materials import BRDF_np
    b = BRDF_np(xet.fromstring('<brdf type="fresnel-blend" id="f"><rgb name="k_g" r="10" g="1000"/></brdf>'))
    assert abs(b.k_g[2] - 4.1752) < 1e-3
    assert BRDF_np(xet.fromstring('<brdf type="specular" id="m"/>')).is_delta
    assert BRDF_np(xet.fromstring('<brdf type="microfacet" id="m"/>')).type_id == 1      # compiled out upstream -> Lambertian
    with pytest.raises(NotImplementedError):
        BRDF_np(xet.fromstring('<brdf type="velvet" id="m"/>'))


def test_rotation_between_matches_scipy_free_cases():
    np.testing.assert_array_equal(np_rotation_between(np.float32([0, 0, 1]), np.float32([0, 0, 1])), np.eye(3, dtype=np.float32))
    np.testing.assert_array_equal(np_rotation_between(np.float32([0, 0, 1]), np.float32([0, 0, -1])), -np.eye(3, dtype=np.float32))
    t = np.float32([0.3, 0.4, 0.8660254])
    t /= np.linalg.norm(t)
    R = np_rotation_between(np.float32([0, 0, 1]), t)
    np.testing.assert_allclose(R @ np.float32([0, 0, 1]), t, atol=1e-6)
    np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-6)


def test_obj_reader(tmp_path):
    p = tmp_path / "quad.obj"
    p.write_text("# quad as one polygon, negative indices, no normals\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nf -4/-4 -3/-3 -2/-2 -1/-1\n")
    meshes, uvs, vns = read_obj(str(p))
    assert meshes.shape == (2, 3, 3) and uvs.shape == (2, 3, 2) and vns is None
    np.testing.assert_array_equal(meshes[1], np.float32([[0, 0, 0], [1, 1, 0], [0, 1, 0]]))     # fan (0, i, i+1)
    m, n, vn, uv = extract_obj_info(str(p))
    np.testing.assert_allclose(n, [[0, 0, 1], [0, 0, 1]])
    assert abs(calculate_surface_area(m) - 1.0) < 1e-6
    (tmp_path / "empty.obj").write_text("v 0 0 0\n")
    with pytest.raises(ValueError):
        read_obj(str(tmp_path / "empty.obj"))
    lum = extract_obj_info(os.path.join(ROOT, "scenes", "meshes", "cornell", "cbox_luminaire.obj"))[0]
    assert abs(calculate_surface_area(lum) - 1.365) < 1e-5                                    # SURVEY §8(c) probe value
    assert abs(calculate_surface_area(np.float32([[[0, 0, 0], [0.5] * 3, [0] * 3]]), 1) - np.pi) < 1e-6


def test_obj_reader_keeps_the_first_material_in_pywavefront_order(tmp_path):
    """The reference reads the vertex stream of the FIRST entry of pywavefront's `obj.materials` (obj_loader.py:35-37): .mtl definition
    order first, then materials first met in `usemtl`, then the default material of faces without one."""
    v = "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nv 0 0 1\n"
    (tmp_path / "two.mtl").write_text("newmtl B\nKd 1 0 0\nnewmtl A\nKd 0 1 0\n")
    (tmp_path / "two.obj").write_text("mtllib two.mtl\n" + v + "usemtl A\nf 1 2 3\nusemtl B\nf 1 3 4\nf 1 4 5\n")
    with pytest.warns(RuntimeWarning):
        meshes, _, _ = read_obj(str(tmp_path / "two.obj"))
    assert meshes.shape[0] == 2                                             # B's two faces (defined first), not A's one (used first)
    np.testing.assert_array_equal(meshes[0], np.float32([[0, 0, 0], [1, 1, 0], [0, 1, 0]]))
    (tmp_path / "nomtl.obj").write_text(v + "usemtl A\nf 1 2 3\nusemtl B\nf 1 3 4\nf 1 4 5\n")
    with pytest.warns(RuntimeWarning):
        assert read_obj(str(tmp_path / "nomtl.obj"))[0].shape[0] == 1     # no .mtl: order of first use
    (tmp_path / "default.obj").write_text(v + "f 1 2 3\nusemtl A\nf 1 3 4\n")
    with pytest.warns(RuntimeWarning):
        assert read_obj(str(tmp_path / "default.obj"))[0].shape[0] == 1   # faces before any usemtl: the default material comes first
    (tmp_path / "unused.mtl").write_text("newmtl X\nnewmtl A\n")
    (tmp_path / "unused.obj").write_text("mtllib unused.mtl\n" + v + "usemtl A\nf 1 2 3\n")
    with pytest.raises(ValueError):                                         # the first material owns no faces: upstream reads an empty stream
        read_obj(str(tmp_path / "unused.obj"))


def test_transform_dtype_flow_and_aabb():
    m = np.float32([[[0, 0, 0], [1, 0, 0], [0, 0, 1]]])
    out, _ = apply_transform(m.copy(), None, None, np.float32([0, -0.001, 0]), None)
    assert out.dtype == np.float32 and out[0, 0, 1] == np.float32(-0.001)
    rot, _ = apply_transform(m.copy(), np.float32([[0, 1, 0]]), np.eye(3), None, None)
    assert rot.dtype == np.float64                    # float64 until the final pack, as upstream
    box = get_aabb(m)
    np.testing.assert_allclose(box, [[0, -0.02, 0], [1, 0.02, 1]], atol=1e-7)       # flat axis padded by 2e-2
    np.testing.assert_array_equal(get_aabb(np.float32([[[1, 2, 3], [0.5] * 3, [0] * 3]]), 1), np.float32([[0.5, 1.5, 2.5], [1.5, 2.5, 3.5]]))


def test_scene_errors(tmp_path):
    (tmp_path / "bad.xml").write_text('<scene version="0.9"><sensor/></scene>')
    with pytest.raises(ValueError):
        scene_parsing(str(tmp_path), "bad.xml")
    (tmp_path / "tex.xml").write_text('<scene version="1.1"><texture id="t" type="checkerboard"/><sensor/></scene>')
    with pytest.raises(NotImplementedError):                       # no lookup for checkerboards upstream either (bxdf/texture.py:96)
        scene_parsing(str(tmp_path), "tex.xml")
    (tmp_path / "tex2.xml").write_text('<scene version="1.1"><texture id="t" type="image"><string name="filename" value="nope.ppm"/></texture><sensor/></scene>')
    with pytest.raises(ValueError):                                # missing image file, same message as upstream
        scene_parsing(str(tmp_path), "tex2.xml")


def test_textured_scene_parse(parsed, flat):
    """scenes/test/textured.xml: texture records, uv coordinates and atlases reach the flat scene; lookups stay inside rectangles."""
    from adapt_amd.parsers.image_io import imread_rgb
    tup, fs = parsed("textured"), flat("textured")
    assert fs.has_textures and fs.uvs.shape == (fs.n_prims, 3, 2) and fs.tex_i.shape == (fs.n_objects, 3, 5)
    assert [None if a is None else a.shape[2] for a in fs.atlas] == [3, 3, 3]
    used = fs.tex_i[:, :, 0] > -255
    assert used.sum() == 6 and used[:, 0].sum() == 4 and used[:, 1].sum() == 1 and used[:, 2].sum() == 1
    for o, m in zip(*np.nonzero(used)):
        _, ox, oy, w, h = fs.tex_i[o, m]
        H, W, _ = fs.atlas[m].shape
        assert 0 <= ox and ox + w <= W and 0 <= oy and oy + h <= H and w >= 2 and h >= 2
    # atlas content = the image file / 255 (bump maps with y and z swapped, bxdf/texture.py:69-71)
    wood = imread_rgb(os.path.join(ROOT, "scenes", "test", "tex", "wood.ppm")).astype(np.float32) / 255.
    o = int(np.nonzero(used[:, 0])[0][0]); _, ox, oy, w, h = fs.tex_i[o, 0]
    assert (w, h) == (48, 32) and np.array_equal(fs.atlas[0][oy:oy + h, ox:ox + w], wood)
    dents = imread_rgb(os.path.join(ROOT, "scenes", "test", "tex", "dents_bump.ppm")).astype(np.float32) / 255.
    o = int(np.nonzero(used[:, 2])[0][0]); _, ox, oy, w, h = fs.tex_i[o, 2]
    assert np.array_equal(fs.atlas[2][oy:oy + h, ox:ox + w], dents[..., [0, 2, 1]])
    assert np.array_equal(fs.tex_f[o, 2], np.float32([1.0, 2.0]))


def test_jpeg_albedo_map_loads_and_matches_the_ppm_of_the_same_image(tmp_path):
    """Every textured scene the reference ships names .jpg files (scenes/cbox/bunny.xml:176-186; texture.py:61 reads them with cv.imread).
    scenes/test/textured.xml with its albedo maps re-encoded as JPEG (quality 100, no chroma subsampling) parses to the same records and
    to atlases within JPEG's loss of the PPM-fed ones."""
    Image = pytest.importorskip("PIL.Image")
    from adapt_amd.parsers import scene_parsing
    from adapt_amd.parsers.image_io import imread_rgb
    from adapt_amd.scene_pack import pack_scene
    src = os.path.join(ROOT, "scenes", "test")
    xml = open(os.path.join(src, "textured.xml")).read()
    assert "scenes/test/tex/wood.ppm" in xml and "scenes/test/tex/tiles.ppm" in xml
    os.makedirs(tmp_path / "tex")
    for name in os.listdir(os.path.join(src, "tex")):
        rgb = imread_rgb(os.path.join(src, "tex", name))
        if name in ("wood.ppm", "tiles.ppm"):
            Image.fromarray(rgb, "RGB").save(tmp_path / "tex" / name.replace(".ppm", ".jpg"), format="JPEG", quality=100, subsampling=0)
        else:
            Image.fromarray(rgb, "RGB").save(tmp_path / "tex" / name.replace(".ppm", ".png"), format="PNG")      # (and the PNG reader on the way)
    xml = xml.replace("wood.ppm", "wood.jpg").replace("tiles.ppm", "tiles.jpg").replace("_bump.ppm", "_bump.png").replace("_normal.ppm", "_normal.png")
    xml = xml.replace("scenes/test/tex/", str(tmp_path / "tex") + "/")
    xml = xml.replace('value="../meshes/', 'value="' + os.path.join(ROOT, "scenes", "meshes") + "/").replace('value="meshes/', 'value="' + os.path.join(src, "meshes") + "/")
    (tmp_path / "textured_jpg.xml").write_text(xml)
    a = pack_scene(*scene_parsing(str(tmp_path), "textured_jpg.xml"))
    b = pack_scene(*scene_parsing(src, "textured.xml"))
    assert np.array_equal(a.tex_i, b.tex_i) and np.array_equal(a.tex_f, b.tex_f) and np.array_equal(a.uvs, b.uvs)
    assert np.array_equal(a.atlas[1], b.atlas[1]) and np.array_equal(a.atlas[2], b.atlas[2])            # PNG: lossless
    d = np.abs(a.atlas[0] - b.atlas[0]) * 255.0
    assert d.max() <= 4.01 and d.mean() <= 0.6, (d.max(), d.mean())                                     # JPEG at quality 100: a level or two (measured: max 3, mean 0.21)
    jpg = imread_rgb(str(tmp_path / "tex" / "wood.jpg"))
    assert jpg.dtype == np.uint8 and jpg.shape == (32, 48, 3)


def test_oversized_textures_are_resized_like_cv_resize(tmp_path):
    """texture.py:65-68: a side above max_size is clamped to it (each side on its own) and the image goes through cv.resize's default
    (bilinear, pixel centres, 11-bit fixed point).  Known answers of the restatement, and the Texture_np path through it."""
    import xml.etree.ElementTree as xet
    from adapt_amd.parsers.image_io import resize_bilinear_u8, write_ppm
    from adapt_amd.textures import Texture_np
    rs = np.random.RandomState(3)
    img = rs.randint(0, 256, size=(6, 8, 3)).astype(np.uint8)
    assert np.array_equal(resize_bilinear_u8(img, 8, 6), img)
    assert np.array_equal(resize_bilinear_u8(np.full((9, 7, 3), 77, np.uint8), 3, 4), np.full((4, 3, 3), 77, np.uint8))
    # 4 -> 2 along x: sample positions 0.5 and 2.5 - the mean of pixels (0, 1) and (2, 3), rounded half up by the +2 >> 2
    row = np.uint8([[[10, 0, 255], [20, 0, 255], [30, 1, 0], [41, 2, 0]]])
    assert resize_bilinear_u8(row, 2, 1).tolist() == [[[15, 0, 255], [36, 2, 0]]]
    # upscaling clamps at the borders: the first and last samples sit outside the pixel centres
    up = resize_bilinear_u8(np.uint8([[[0], [100]]]), 4, 1)[0, :, 0]
    assert up.tolist() == [0, 25, 75, 100]
    write_ppm(str(tmp_path / "big.ppm"), rs.randint(0, 256, size=(5, 40, 3)).astype(np.uint8))
    el = xet.fromstring(f'<texture type="image" id="big" tag="albedo"><string name="filename" value="{tmp_path / "big.ppm"}"/></texture>')
    t = Texture_np(el, max_size=16)
    assert (t.w, t.h) == (16, 5) and t.texture_img.shape == (5, 16, 3) and t.texture_img.dtype == np.float32


def test_textured_scene_matches_reference_parser(flat):
    """The reference's own parser (OpenCV / rectpack replaced by the generator's stand-ins) on scenes/test/textured.xml
    (tests/golden/refparser_textured.npz): same uv coordinates and texture records up to the atlas layout, same texels behind every record."""
    ref = golden("refparser_textured.npz")
    fs = flat("textured")
    assert np.array_equal(ref["uvs"], fs.uvs) and np.array_equal(ref["tex_f"], fs.tex_f)
    assert np.array_equal(ref["tex_i"][:, :, [0, 3, 4]], fs.tex_i[:, :, [0, 3, 4]])       # type, w, h; offsets depend on the packer
    records = list(zip(*np.nonzero(fs.tex_i[:, :, 0] > -255)))
    assert {f"texels_{o}_{m}" for o, m in records} == {k for k in ref.files if k.startswith("texels_")}
    for o, m in records:
        _, ox, oy, w, h = fs.tex_i[o, m]
        assert np.array_equal(fs.atlas[m][oy:oy + h, ox:ox + w], ref[f"texels_{o}_{m}"])


def test_config_overrides_and_crop(parsed):
    cfg = dict(parsed("cbox")[3])
    rc = make_config(cfg, width=256, height=128, max_bounce=4)
    assert (rc.width, rc.height, rc.max_bounce) == (256, 128, 4)
    assert rc.focal == fov2focal(39.3077, 128) and rc.half_w == 128 and rc.half_h == 64 and not rc.do_crop
    cfg["film"] = {"width": 64, "height": 64, "crop_x": 32, "crop_y": 20, "crop_rx": 8, "crop_ry": 4}
    rc = make_config(cfg)
    assert rc.do_crop and (rc.start_x, rc.end_x, rc.start_y, rc.end_y) == (24, 40, 16, 24)
    assert rc.rr_bounce_th == 4 and abs(rc.rr_threshold - 0.1) < 1e-12 and rc.use_bvh is False


@pytest.mark.parametrize("d,f,tag", [("cbox", "cbox.xml", "cbox"), ("csphere", "balls-mono.xml", "balls_mono"), ("cbox", "complex.xml", "glass_box")])
def test_reference_parser_objects_are_accepted(d, f, tag, flat):
    """INTEGRATION.md option A: the objects AdaPT's own scene_parsing returns for its <d>/<f> (its host classes, imported from the
    reference tree under the golden generator's taichi stand-in) pack to the same flat scene as this repo's parser.  The packed
    arrays are tests/golden/refparser_<tag>.npz (tests/golden/gen/gen_goldens.py --only parse)."""
    ref = golden(f"refparser_{tag}.npz")
    mine = flat(tag)
    for name in ("prims", "normals", "v_normals", "obj_info", "obj_aabb", "emitter_id", "bxdf_i", "bxdf_f", "src_i", "src_f"):
        assert np.array_equal(ref[name], getattr(mine, name)), name
    assert float(ref["world_ior"]) == mine.world_ior and bool(ref["has_vertex_normal"]) == mine.has_vertex_normal


# ---- participating media (volumetric tracer inputs)
@pytest.mark.parametrize("name", ["media_a", "media_b", "null_panes"])
def test_media_scene_parse_matches_reference_parser_arrays(name):
    """scenes/test/media_*.xml through this repo's front end = the arrays the reference's parser produced for the same file (stored
    in the vptscene fixture): geometry, materials, emitters and the per-object / world medium tables, bit for bit."""
    from conftest import golden
    from adapt_amd.scene_pack import pack_scene, make_config
    tup = scene_parsing(os.path.join(ROOT, "scenes", "test"), name + ".xml")
    fs, g = pack_scene(*tup), golden(f"vptscene_{name}.npz")
    for k in ("prims", "normals", "v_normals", "obj_info", "obj_aabb", "emitter_id", "bxdf_i", "bxdf_f", "src_i", "src_f", "med_i", "med_f"):
        assert np.array_equal(np.asarray(getattr(fs, k)).view(np.uint32), np.asarray(g[k]).view(np.uint32)), (name, k)
    assert fs.has_scattering_media
    rc = make_config(tup[3], volumetric=True)
    assert rc.volumetric and rc.max_bounce == int(g["max_bounce"]) and rc.num_shadow_ray == int(g["num_shadow_ray"])
    assert np.array_equal(np.float32(rc.cam_t), g["cam_pos"])


def test_medium_records():
    """Medium_np (bxdf/medium.py:24-68): type ids, u_e = u_a + u_s, defaults of a missing <medium>, unknown types refused."""
    import xml.etree.ElementTree as xet
    from adapt_amd.materials import Medium_np
    from adapt_amd.scene_pack import pack_medium
    m = Medium_np(xet.fromstring('<medium type="multi-hg"><rgb name="u_a" value="0.25"/><rgb name="u_s" r="1" g="2" b="3"/>'
                                 '<rgb name="par" r="0.5" g="-0.5" b="0"/><rgb name="pdf" r="0.25" g="0.5" b="0.25"/><float name="ior" value="1.25"/></medium>'))
    kind, f = pack_medium(m)
    assert kind == 1 and f.dtype == np.float32 and f.shape == (16,)
    assert np.array_equal(f, np.float32([1.25, 1, 2, 3, .25, .25, .25, 1.25, 2.25, 3.25, .5, -.5, 0, .25, .5, .25]))
    kind, f = pack_medium(Medium_np(None))
    assert kind == -1 and f[0] == 1.0 and np.array_equal(f[1:13], np.zeros(12, np.float32)) and np.array_equal(f[13:], np.float32([1, 0, 0]))
    assert [Medium_np(xet.fromstring(f'<medium type="{k}"/>')).type_id for k in ("hg", "multi-hg", "rayleigh", "mie", "transparent")] == [0, 1, 2, 3, -1]
    with pytest.raises(NotImplementedError):
        Medium_np(xet.fromstring('<medium type="smoke"/>'))
    assert pack_medium(None)[0] == -1


def test_vol_reader_and_refusals(tmp_path):
    """Own .vol reader (Mitsuba v3 layout, vol2numpy.cpp:35-73) and the configurations that fail upstream are refused with a reason."""
    import struct
    import xml.etree.ElementTree as xet
    from adapt_amd.volumes import GridVolume_np, read_vol
    grid = np.arange(2 * 3 * 4, dtype=np.float32).reshape(2, 3, 4)          # [z][y][x]
    path = tmp_path / "g.vol"
    path.write_bytes(b"VOL\x03" + struct.pack("<5i", 1, 4, 3, 2, 1) + struct.pack("<6f", 0, 0, 0, 1, 1, 1) + grid.tobytes())
    data, shape = read_vol(str(path))
    assert shape == (4, 3, 2, 1) and data.shape == (2, 3, 4, 1) and np.array_equal(data[..., 0], grid)
    (tmp_path / "bad.vol").write_bytes(b"VOX\x03" + bytes(60))
    with pytest.raises(ValueError):
        read_vol(str(tmp_path / "bad.vol"))
    mk = lambda body, kind="mono": xet.fromstring(f'<volume name="v" type="{kind}" phase_type="hg"><string name="density_grid" path="{path}"/>{body}</volume>')
    v = GridVolume_np(mk('<bool name="mono2rgb" value="true"/><rgb name="density_scaling" r="2" g="3" b="4"/>'))
    ints, floats, g3 = v.pack()
    assert ints.tolist() == [2, 4, 3, 2, 0] and floats.shape == (33,) and g3.shape == (2, 3, 4, 3)
    assert np.array_equal(g3[1, :, :, 1], grid[1] * np.float32(3))           # z = 1 lies in the second part of the ramp: green untouched
    with pytest.raises(NotImplementedError):                                  # mono without mono2rgb: upstream fails exporting the majorant
        GridVolume_np(mk(""))
    with pytest.raises(NotImplementedError):
        GridVolume_np(mk("", kind="smoke"))
    with pytest.raises(RuntimeError):
        GridVolume_np(xet.fromstring('<volume name="v" type="mono" phase_type="hg"><string name="density_grid" path="/nonexistent.vol"/></volume>'))


def test_microfacet_switch_mirrors_the_reference(monkeypatch):
    """`__ENABLE_MICROFACET__` (bxdf/brdf.py:8): off, a microfacet BRDF parses to a Lambertian one (brdf.py:60-65); on, type 3 stays
    and `roughness` becomes the Trowbridge-Reitz alphas (brdf.py:96-103,115-120).  The expected records are the ones the reference's
    own BRDF_np produced with the switch on (tests/golden/microfacet_functions.npz: k_d, k_s, k_g, mean, ior per material)."""
    from conftest import golden
    from adapt_amd import materials
    specs = [('#E0C8A0', 'value="0.08"', 'r="1.0" g="1.5" b="0.0"'), ('#A0C8E0', 'value="0.45"', 'r="1.0" g="1.33" b="0.0"'),
             ('#D8D8D8', 'r="0.05" g="0.5" b="0.0"', 'r="1.0" g="2.4" b="0.0"'), ('#FFFFFF', 'value="1.0"', 'r="1.5" g="1.0" b="0.0"'),
             ('#808080', 'value="0.0"', 'r="1.0" g="1.5" b="0.0"')]
    xml = [f'<brdf type="microfacet" id="m"><rgb name="k_d" value="{kd}"/><rgb name="roughness" {r}/><rgb name="ref_ior" {ior}/></brdf>' for kd, r, ior in specs]
    g = golden("microfacet_functions.npz")
    monkeypatch.setattr(materials, "ENABLE_MICROFACET", True)
    for k, x in enumerate(xml):
        ints, flts = materials.BRDF_np(xet.fromstring(x)).pack()
        assert ints.tolist() == g["mat_i"][k].tolist() == [3, 0, 0, 0]
        assert np.array_equal(flts, g["mat_f"][k])
    monkeypatch.setattr(materials, "ENABLE_MICROFACET", False)
    for k, x in enumerate(xml):
        b = materials.BRDF_np(xet.fromstring(x))
        assert (b.type, b.type_id) == ("lambertian", 1)
        assert np.array_equal(b.k_g, g["mat_f"][k][6:9])              # the roughness -> alpha conversion goes by the attribute's name, switch or not
