#!/usr/bin/env python3
"""Generate tests/golden/*.npz from the reference's own source (authoring container only).

    python tests/golden/gen/gen_goldens.py [--only parse|func|media|volfunc|image|features|textured|refscenes|vpt|volgrid|bvh|microfacet|settings]

Every fixture is produced by calling UNMODIFIED reference code (/root/reference) under the
float32 stand-in `taichi` package in shim/ (third-party taichi==1.6.0 is not installable
here).  Fixtures are plain input/output arrays; no reference source text is stored.

`--only microfacet` is the one section that runs the reference with a setting other than its default: the module switch
`__ENABLE_MICROFACET__` of bxdf/brdf.py:8, which upstream tells its users to flip by hand (brdf.py:63), is True for that
section (refenv.py flips it at import, in memory).  It is never part of `all`: the switch is process-wide, so the section
runs in a process of its own (`ADAPT_REF_MICROFACET=1`, set by this script when it re-executes itself).

`--only settings` (tests/settings_cases.py: every sensor setting flipped on five scenes, one whole-kernel run each) takes minutes and
is not part of `all` either.
"""
import argparse
import os
import sys
import time

import numpy as np

import refenv

ti = refenv.setup()
from taichi.math import vec3  # noqa: E402

OUT = os.path.abspath(os.path.join(refenv.HERE, ".."))
RS = np.random.RandomState(20260928)


def reseed(fixture):
    """Every fixture draws its random inputs from its own stream, seeded by its file name: `--only <section>` then rewrites exactly
    the committed vectors, whatever else ran before it in the same process."""
    import zlib
    global RS
    RS = np.random.RandomState(zlib.crc32(fixture.encode()) & 0x7fffffff)


def unit(v):
    v = np.float32(v)
    return v / np.float32(np.linalg.norm(v))


def rand_dir():
    return unit(RS.normal(size=3))


# ------------------------------------------------------------------ parsed scenes
def dump_parse(scene_dir, xml, tag):
    from parsers.xml_parser import scene_parsing
    emitters, arr, objs, cfg = scene_parsing(os.path.join(refenv.REFERENCE, "scenes", scene_dir), xml)
    from la.cam_transform import np_rotation_between, fov2focal
    orient = np.float32(cfg["transform"][0]) / np.linalg.norm(cfg["transform"][0])
    out = {
        "primitives": arr["primitives"], "n_g": arr["n_g"], "n_s": arr["n_s"], "uvs": arr["uvs"],
        "indices": np.int64(arr["indices"]) if arr["indices"] is not None else np.int64([]),
        "aabb": np.float32([o.aabb for o in objs]), "tri_num": np.int32([o.tri_num for o in objs]),
        "obj_type": np.int32([o.type for o in objs]), "emitter_ref": np.int32([o.emitter_ref_id for o in objs]),
        "bxdf_type": np.int32([o.bsdf.type_id for o in objs]), "bxdf_delta": np.int32([int(o.bsdf.is_delta) for o in objs]),
        "bxdf_is_bsdf": np.int32([int(hasattr(o.bsdf, "medium")) for o in objs]),
        "k_d": np.float32([o.bsdf.k_d for o in objs]), "k_s": np.float32([o.bsdf.k_s for o in objs]),
        "k_g": np.float32([o.bsdf.k_g for o in objs]),
        "ior": np.float32([o.bsdf.medium.ior if hasattr(o.bsdf, "medium") else 1.0 for o in objs]),
        "src_type": np.array([e.type for e in emitters]), "src_intensity": np.float32([e.intensity for e in emitters]),
        "src_inv_area": np.float32([e.inv_area for e in emitters]),
        "src_pos": np.float32([getattr(e, "pos", np.zeros(3)) if not hasattr(getattr(e, "pos", None), "a") else np.zeros(3) for e in emitters]),
        "cam_dir": np.float32(cfg["transform"][0]), "cam_pos": np.float32(cfg["transform"][1]),
        "cam_r": np.float32(np_rotation_between(np.float32([0, 0, 1]), orient)),
        "focal": np.float64(fov2focal(cfg["fov"], min(cfg["film"]["width"], cfg["film"]["height"]))),
        "fov": np.float64(cfg["fov"]), "max_bounce": np.int32(cfg["max_bounce"]), "num_shadow_ray": np.int32(cfg["num_shadow_ray"]),
        "width": np.int32(cfg["film"]["width"]), "height": np.int32(cfg["film"]["height"]),
        "has_vertex_normal": np.int32(cfg["has_vertex_normal"]), "world_ior": np.float32(cfg["world"].medium.ior),
    }
    np.savez_compressed(os.path.join(OUT, f"parse_{tag}.npz"), **out)
    print(f"parse_{tag}: {arr['primitives'].shape[0]} prims, {len(objs)} objects, {len(emitters)} emitters")


FLAT_KEYS = ("prims", "normals", "v_normals", "obj_info", "obj_aabb", "emitter_id", "bxdf_i", "bxdf_f", "src_i", "src_f")


def dump_ref_parser_objects(scene_dir, xml, tag):
    """The host objects the reference's scene_parsing returns, packed by adapt_amd.scene_pack.pack_scene (INTEGRATION.md option A)."""
    sys.path.insert(0, refenv.REPO)
    from parsers.xml_parser import scene_parsing
    from adapt_amd.scene_pack import pack_scene
    fs = pack_scene(*scene_parsing(os.path.join(refenv.REFERENCE, "scenes", scene_dir), xml))
    out = {k: getattr(fs, k) for k in FLAT_KEYS}
    out.update(world_ior=np.float32(fs.world_ior), has_vertex_normal=np.int32(fs.has_vertex_normal))
    np.savez_compressed(os.path.join(OUT, f"refparser_{tag}.npz"), **out)
    print(f"refparser_{tag}: {fs.prims.shape[0]} prims, {fs.obj_info.shape[0]} objects")


def dump_ref_parser_textures():
    """The reference's parser on scenes/test/textured.xml, packed: uv coordinates, texture records, and the texels behind every record
    (texels_<object>_<map>; the atlas itself is not stored, its layout depends on the packer)."""
    sys.path.insert(0, refenv.REPO)
    from parsers.xml_parser import scene_parsing
    from adapt_amd.scene_pack import pack_scene
    cwd = os.getcwd()
    os.chdir(refenv.REPO)                               # texture paths in the scene file are relative to the repository root
    try:
        fs = pack_scene(*scene_parsing(os.path.join(refenv.REPO, "scenes", "test"), "textured.xml"))
    finally:
        os.chdir(cwd)
    out = {"uvs": fs.uvs, "tex_i": fs.tex_i, "tex_f": fs.tex_f}
    for o, m in zip(*np.nonzero(fs.tex_i[:, :, 0] > -255)):
        _, x, y, w, h = fs.tex_i[o, m]
        out[f"texels_{o}_{m}"] = fs.atlas[m][y:y + h, x:x + w]
    np.savez_compressed(os.path.join(OUT, "refparser_textured.npz"), **out)
    print(f"refparser_textured: {len(out) - 3} texture records")


# ------------------------------------------------------------- function vectors
def gen_functions():
    from bxdf.brdf import BRDF
    from bxdf.bsdf import BSDF
    from bxdf.medium import Medium
    from tracer.interaction import Interaction
    from la.cam_transform import rotation_between, delocalize_rotate
    from la.geo_optics import fresnel_equation, snell_refraction, inci_reflect_dir, is_total_reflection
    from renderer.constants import INVALID
    from sampler import general_sampling as gs

    reseed("functions.npz")
    out = {}
    # --- rotation_between (incl. parallel / anti-parallel)
    A, B, R = [], [], []
    pairs = [(rand_dir(), rand_dir()) for _ in range(48)]
    pairs += [(np.float32([0, 1, 0]), np.float32([0, 1, 0])), (np.float32([0, 1, 0]), np.float32([0, -1, 0])),
              (np.float32([0, 1, 0]), unit([1e-3, 1, 0])), (np.float32([0, 1, 0]), unit([0.3, -0.2, 0.9]))]
    for a, b in pairs:
        A.append(a); B.append(b); R.append(rotation_between(vec3(a), vec3(b)).to_numpy())
    out["rot_a"], out["rot_b"], out["rot_R"] = np.float32(A), np.float32(B), np.float32(R)

    # --- fresnel / snell
    fr_in, fr_out = [], []
    for _ in range(32):
        n1, n2 = np.float32(RS.uniform(1, 2)), np.float32(RS.uniform(1, 2))
        c1, c2 = np.float32(RS.uniform(0, 1)), np.float32(RS.uniform(0, 1))
        fr_in.append([n1, n2, c1, c2]); fr_out.append(fresnel_equation(n1, n2, c1, c2))
    fr_in.append([1, 1.5, 1, 1]); fr_out.append(fresnel_equation(np.float32(1), np.float32(1.5), np.float32(1), np.float32(1)))
    out["fresnel_in"], out["fresnel_out"] = np.float32(fr_in), np.float32(fr_out)
    sn_in, sn_out = [], []
    for _ in range(32):
        n = rand_dir(); d = rand_dir()
        ni, nr = (np.float32(1.0), np.float32(1.5)) if RS.rand() < 0.5 else (np.float32(1.5), np.float32(1.0))
        dn = np.float32(np.dot(d, n))
        v, c2 = snell_refraction(vec3(d), vec3(n), dn, ni, nr)
        sn_in.append(np.concatenate([d, n, [dn, ni, nr]])); sn_out.append(np.concatenate([v.to_numpy(), [c2]]))
    out["snell_in"], out["snell_out"] = np.float32(sn_in), np.float32(sn_out)

    # --- BRDF / BSDF eval, pdf, sample
    mats = []
    def brdf(t, kd, ks, kg, delta=0):
        kd, ks, kg = np.float32(kd), np.float32(ks), np.float32(kg)
        if t == 5:
            kg = kg.copy(); kg[2] = np.sqrt((kg[0] + 1) * (kg[1] + 1)) / (8. * np.pi)
        mean = np.float32([kd.mean(), ks.mean(), kg.mean()])
        return dict(is_bsdf=0, type=t, delta=delta, kd=kd, ks=ks, kg=kg, mean=mean, ior=np.float32(1))
    h = lambda s: [int(s[i:i + 2], 16) / 255. for i in (0, 2, 4)]
    mats.append(brdf(0, h("D2D2D2"), [0] * 3, [1] * 3))                     # phong (balls-mono diffuse)
    mats.append(brdf(0, h("BCBCBC"), [0.3] * 3, [8, 8, 8]))                  # glossy blinn-phong
    mats.append(brdf(1, h("FFFFFF"), [0] * 3, [1] * 3))                      # lambertian
    mats.append(brdf(2, h("DEDEDE"), [0] * 3, [1] * 3, delta=1))             # mirror
    mats.append(brdf(4, h("BCBCBC"), h("424242"), [10] * 3))                 # mod-phong
    mats.append(brdf(5, h("CACACA"), h("333333"), [10, 1000, 0]))            # fresnel-blend
    sig = np.float32(20.0) * np.float32(np.pi / 180.); s2 = sig * sig
    on_kg = [1 - (s2 / (2 * (s2 + 0.33))), 0.45 * s2 / (s2 + 0.09), 1.5]
    mats.append(brdf(6, h("C8B496"), [0] * 3, on_kg))                        # oren-nayar
    mats.append(brdf(7, h("C8B496"), [0.9] * 3, on_kg))                      # thin-coat
    mats.append(dict(is_bsdf=1, type=0, delta=1, kd=np.float32(h("FAFAFA")), ks=np.zeros(3, np.float32), kg=np.ones(3, np.float32),
                     mean=np.zeros(3, np.float32), ior=np.float32(1.5)))     # det-refraction glass
    mats.append(dict(is_bsdf=1, type=1, delta=0, kd=np.float32(h("E0E0FA")), ks=np.zeros(3, np.float32), kg=np.ones(3, np.float32),
                     mean=np.zeros(3, np.float32), ior=np.float32(1.33)))    # lambertian transmission
    world_medium = Medium(_type=-1, ior=1.0)

    def build(m):
        if m["is_bsdf"]:
            return BSDF(_type=m["type"], is_delta=m["delta"], k_d=vec3(m["kd"]), k_s=vec3(m["ks"]), k_g=vec3(m["kg"]),
                        medium=Medium(_type=-1, ior=m["ior"]))
        return BRDF(_type=m["type"], is_delta=m["delta"], k_d=vec3(m["kd"]), k_s=vec3(m["ks"]), k_g=vec3(m["kg"]), mean=vec3(m["mean"]))

    mat_i, mat_f = [], []
    ev_in, ev_out, sm_in, sm_scr, sm_out = [], [], [], [], []
    for mi, m in enumerate(mats):
        obj = build(m)
        mat_i.append([m["type"], m["delta"], m["is_bsdf"], 0])
        mat_f.append(np.concatenate([m["kd"], m["ks"], m["kg"], m["mean"], [m["ior"]]]))
        for _ in range(24):
            n_s = rand_dir()
            n_g = unit(n_s + np.float32(RS.normal(size=3) * 0.05))
            incid = rand_dir()
            if np.dot(incid, n_s) > 0 and RS.rand() < 0.8:
                incid = -incid                                   # mostly arriving against the normal
            outd = rand_dir()
            if RS.rand() < 0.25:                                 # exercise the delta-direction matching branches
                it0 = Interaction(n_s=vec3(n_s), n_g=vec3(n_g), tex=INVALID)
                if m["is_bsdf"]:
                    # eval/get_pdf match `incid` against the mirror / refraction of `out`: build such a pair
                    dn = np.float32(np.dot(outd, n_s))
                    if RS.rand() < 0.5:
                        incid = (vec3(outd) - 2 * vec3(n_s) * dn).normalized().to_numpy()
                    else:
                        ni, nr = (np.float32(1.0), m["ior"]) if dn < 0 else (m["ior"], np.float32(1.0))
                        rv, c2 = snell_refraction(vec3(outd), vec3(n_s), dn, ni, nr)
                        if c2 > 0:
                            incid = rv.to_numpy()
                else:
                    outd = inci_reflect_dir(vec3(incid), vec3(n_s))[0].to_numpy()
            it = Interaction(n_s=vec3(n_s), n_g=vec3(n_g), tex=INVALID)
            if m["is_bsdf"]:
                e = obj.eval_surf(it, vec3(incid), vec3(outd), world_medium, -1)
                p = obj.get_pdf(it, vec3(outd), vec3(incid), world_medium)
            else:
                e = obj.eval(it, vec3(incid), vec3(outd))
                p = obj.get_pdf(it, vec3(outd), vec3(incid))
            ev_in.append(np.concatenate([[mi], n_s, n_g, incid, outd])); ev_out.append(np.concatenate([e.to_numpy(), [p]]))
            script = np.zeros(8)                      # kept for shape compatibility; the stream is Philox(key = test index, seed 777, sample 1)
            ti.RNG.set_philox(len(sm_in), 777, 1)
            it = Interaction(n_s=vec3(n_s), n_g=vec3(n_g), tex=INVALID)
            if m["is_bsdf"]:
                d, s, pdf, spec = obj.sample_surf_rays(it, vec3(incid), world_medium, -1)
            else:
                d, s, pdf, spec = obj.sample_new_rays(it, vec3(incid))
            sm_in.append(np.concatenate([[mi], n_s, n_g, incid])); sm_scr.append(script)
            sm_out.append(np.concatenate([np.float32(d.to_numpy()), np.float32(s.to_numpy()), [pdf, float(bool(spec)), ti.RNG.draw]]))
    # fixed geometries on which the fresnel-blend pdf is NaN upstream (outgoing direction below the shading normal: a negative base under a
    # fractional power, brdf.py get_pdf): the quirk is part of the contract, so it is part of the vectors whatever the random rows happen to hit
    for row in ([0.66424567, 0.40828657, -0.6261627, 0.73268086, 0.27544102, -0.62234324, 0.94675964, -0.01885428, 0.32138875, 0.38887125, -0.36176717, 0.84729207],
                [0.8451841, -0.5228336, -0.11094508, 0.87144643, -0.48752844, -0.05382608, -0.44677615, -0.81933254, -0.3592842, -0.18898904, 0.16722248, 0.9676362],
                [-0.6718239, 0.71369886, 0.19820789, -0.6796413, 0.715816, 0.16029695, -0.81376815, 0.30567485, 0.49431202, 0.34559214, -0.9259488, 0.15226662]):
        r = np.float32(row); n_s, n_g, incid, outd = r[0:3], r[3:6], r[6:9], r[9:12]
        obj = build(mats[5])
        it = Interaction(n_s=vec3(n_s), n_g=vec3(n_g), tex=INVALID)
        e = obj.eval(it, vec3(incid), vec3(outd)); pq = obj.get_pdf(it, vec3(outd), vec3(incid))
        ev_in.append(np.concatenate([[5], n_s, n_g, incid, outd])); ev_out.append(np.concatenate([e.to_numpy(), [pq]]))
    out["mat_i"], out["mat_f"] = np.int32(mat_i), np.float32(mat_f)
    out["eval_in"], out["eval_out"] = np.float32(ev_in), np.float32(ev_out)
    out["sample_in"], out["sample_script"], out["sample_out"] = np.float32(sm_in), np.float64(sm_scr), np.float32(sm_out)

    # --- free samplers with scripted randoms
    smp = {}
    for name, fn, nrand in (("cosine_hemisphere", lambda: gs.cosine_hemisphere(), 2),
                            ("uniform_sphere", lambda: gs.uniform_sphere(), 2),
                            ("mod_phong_hemisphere", lambda: gs.mod_phong_hemisphere(np.float32(10.0)), 2),
                            ("fresnel_hemisphere", lambda: gs.fresnel_hemisphere(np.float32(10.0), np.float32(1000.0)), 2)):
        scr, res = [], []
        for _ in range(16):
            s = RS.rand(nrand); ti.RNG.set_script(s)
            v, p = fn()
            scr.append(s); res.append(np.concatenate([v.to_numpy(), [p]]))
        out[f"smp_{name}_script"], out[f"smp_{name}_out"] = np.float64(scr), np.float32(res)
    np.savez_compressed(os.path.join(OUT, "functions.npz"), **out)
    print("functions:", {k: v.shape for k, v in out.items()})


def gen_microfacet_functions():
    """BRDF.eval / get_pdf / sample_new_rays of the reference for microfacet BRDFs (type 3), switch on.  Same layout as functions.npz."""
    from bxdf import brdf as brdf_mod
    from bxdf.brdf import BRDF, BRDF_np
    from tracer.interaction import Interaction
    from la.geo_optics import inci_reflect_dir
    from renderer.constants import INVALID
    import xml.etree.ElementTree as xet
    assert brdf_mod.__ENABLE_MICROFACET__ is True
    reseed("microfacet_functions.npz")
    out = {}
    specs = [('#E0C8A0', '0.08', 'r="1.0" g="1.5" b="0.0"'), ('#A0C8E0', '0.45', 'r="1.0" g="1.33" b="0.0"'),
             ('#D8D8D8', None, 'r="1.0" g="2.4" b="0.0"'), ('#FFFFFF', '1.0', 'r="1.5" g="1.0" b="0.0"'), ('#808080', '0.0', 'r="1.0" g="1.5" b="0.0"')]
    mats = []
    for kd, rough, ior in specs:
        rnode = f'<rgb name="roughness" value="{rough}"/>' if rough is not None else '<rgb name="roughness" r="0.05" g="0.5" b="0.0"/>'
        m = BRDF_np(xet.fromstring(f'<brdf type="microfacet" id="m"><rgb name="k_d" value="{kd}"/>{rnode}<rgb name="ref_ior" {ior}/></brdf>'))
        assert m.type_id == 3
        mats.append(m)
    mat_i, mat_f, ev_in, ev_out, sm_in, sm_out = [], [], [], [], [], []
    for mi, m in enumerate(mats):
        obj = m.export()
        mean = np.float32([m.k_d.mean(), m.k_s.mean(), m.k_g.mean()])
        mat_i.append([3, 0, 0, 0]); mat_f.append(np.concatenate([m.k_d, m.k_s, m.k_g, mean, [1.0]]))
        for k in range(40):
            n_s = rand_dir() if k % 5 else np.float32([0, 1, 0])
            n_g = unit(n_s + np.float32(RS.normal(size=3) * 0.05))
            incid = rand_dir()
            if np.dot(incid, n_s) > 0 and RS.rand() < 0.85:
                incid = -incid
            outd = rand_dir()
            if np.dot(outd, n_s) < 0 and RS.rand() < 0.85:
                outd = -outd
            if RS.rand() < 0.3:                                  # near the mirror direction, where a smooth lobe lives
                outd = unit(inci_reflect_dir(vec3(incid), vec3(n_s))[0].to_numpy() + np.float32(RS.normal(size=3) * 0.05))
            if k % 11 == 0:
                incid = unit(-n_s + np.float32(RS.normal(size=3) * 1e-4))       # (almost) normal incidence: the `cos_theta > 1 - eps` sampling branch
            it = Interaction(n_s=vec3(n_s), n_g=vec3(n_g), tex=INVALID)
            e = obj.eval(it, vec3(incid), vec3(outd))
            p = obj.get_pdf(it, vec3(outd), vec3(incid))
            ev_in.append(np.concatenate([[mi], n_s, n_g, incid, outd])); ev_out.append(np.concatenate([e.to_numpy(), [p]]))
            ti.RNG.set_philox(len(sm_in), 777, 1)
            it = Interaction(n_s=vec3(n_s), n_g=vec3(n_g), tex=INVALID)
            d, sp, pdf, spec = obj.sample_new_rays(it, vec3(incid))
            sm_in.append(np.concatenate([[mi], n_s, n_g, incid]))
            sm_out.append(np.concatenate([np.float32(d.to_numpy()), np.float32(sp.to_numpy()), [pdf, float(bool(spec)), ti.RNG.draw]]))
    # fixed geometries on which the fresnel-blend pdf is NaN upstream (outgoing direction below the shading normal: a negative base under a
    # fractional power, brdf.py get_pdf): the quirk is part of the contract, so it is part of the vectors whatever the random rows happen to hit
    for row in ([0.66424567, 0.40828657, -0.6261627, 0.73268086, 0.27544102, -0.62234324, 0.94675964, -0.01885428, 0.32138875, 0.38887125, -0.36176717, 0.84729207],
                [0.8451841, -0.5228336, -0.11094508, 0.87144643, -0.48752844, -0.05382608, -0.44677615, -0.81933254, -0.3592842, -0.18898904, 0.16722248, 0.9676362],
                [-0.6718239, 0.71369886, 0.19820789, -0.6796413, 0.715816, 0.16029695, -0.81376815, 0.30567485, 0.49431202, 0.34559214, -0.9259488, 0.15226662]):
        r = np.float32(row); n_s, n_g, incid, outd = r[0:3], r[3:6], r[6:9], r[9:12]
        obj = build(mats[5])
        it = Interaction(n_s=vec3(n_s), n_g=vec3(n_g), tex=INVALID)
        e = obj.eval(it, vec3(incid), vec3(outd)); pq = obj.get_pdf(it, vec3(outd), vec3(incid))
        ev_in.append(np.concatenate([[5], n_s, n_g, incid, outd])); ev_out.append(np.concatenate([e.to_numpy(), [pq]]))
    out["mat_i"], out["mat_f"] = np.int32(mat_i), np.float32(mat_f)
    out["eval_in"], out["eval_out"] = np.float32(ev_in), np.float32(ev_out)
    out["sample_in"], out["sample_out"] = np.float32(sm_in), np.float32(sm_out)
    np.savez_compressed(os.path.join(OUT, "microfacet_functions.npz"), **out)
    ev, so = out["eval_out"], out["sample_out"]
    print("microfacet_functions:", {k: v.shape for k, v in out.items()}, "nonzero evals", int(np.any(ev[:, :3] != 0, axis=1).sum()),
          "nonzero pdfs", int((ev[:, 3] != 0).sum()), "nonzero sampled", int(np.any(so[:, 3:6] != 0, axis=1).sum()), "NaNs", int(np.isnan(ev).sum() + np.isnan(so).sum()))


# ---------------------------------------------- scene-bound functions + images

def gen_media_functions():
    """Medium.sample_mfp / transmittance / sample_new_rays / eval (bxdf/medium.py:84-125) and the phase functions behind them
    (bxdf/phase.py, sampler/phase_sampling.py) on the shared Philox stream: key = test index, seeds 779 (free path) / 780 (scatter)."""
    from bxdf.medium import Medium
    from bxdf.phase import PhaseFunction
    reseed("media_functions.npz")
    media = [   # type, ior, u_s, u_a, par, pdf
        (0, 1.0, [1.2, 1.0, 0.8], [0.15] * 3, [0.6] * 3, [1, 0, 0]),                    # forward H-G, coloured
        (0, 1.0, [1.5] * 3, [0.2] * 3, [0.0] * 3, [1, 0, 0]),                           # isotropic branch of sample_hg (|g| < 1e-4)
        (0, 1.33, [0.05, 2.5, 0.4], [0.0, 0.1, 1.0], [-0.75] * 3, [1, 0, 0]),           # back-scattering, very different channels
        (1, 1.0, [0.05, 0.06, 0.08], [0.01] * 3, [0.7, -0.3, 0.1], [0.5, 0.3, 0.2]),    # three lobes
        (1, 1.0, [0.9] * 3, [0.1] * 3, [0.8, -0.2, 0.0], [0.7, 0.3, 0.0]),              # two lobes (third weight 0; pdf[1] > 1e-4 still adds lobe 3)
        (1, 1.0, [0.9] * 3, [0.1] * 3, [0.5, 0.2, 0.9], [1.0, 0.0, 0.0]),               # pdf[1] = 0: the third lobe is skipped in eval
        (2, 1.5, [0.6, 0.9, 1.4], [0.05] * 3, [0] * 3, [1, 0, 0]),                      # Rayleigh
        (3, 1.0, [1.0] * 3, [0.1] * 3, [0] * 3, [1, 0, 0]),                             # mie: no phase function upstream
        (-1, 1.5, [0] * 3, [0] * 3, [0] * 3, [1, 0, 0]),                                # transparent
        (0, 1.0, [0.0, 0.0, 2.0], [0.0] * 3, [0.3] * 3, [1, 0, 0]),                     # u_e = 0 in two channels: the 1e-5 floor of random_rgb
    ]
    med_i, med_f, objs = [], [], []
    for t, ior, us, ua, par, pdf in media:
        us, ua, par, pdf = np.float32(us), np.float32(ua), np.float32(par), np.float32(pdf)
        ue = us + ua
        med_i.append(t); med_f.append(np.concatenate([[ior], us, ua, ue, par, pdf]))
        objs.append(Medium(_type=t, ior=ior, u_a=vec3(ua), u_s=vec3(us), u_e=vec3(ue), ph=PhaseFunction(_type=t, par=vec3(par), pdf=vec3(pdf))))
    mfp_in, mfp_out, sc_in, sc_out, ev_in, ev_out = [], [], [], [], [], []
    for mi, m in enumerate(objs):
        for k in range(24):
            depth = np.float32(10.0 ** RS.uniform(-2, 1.3))
            ti.RNG.set_philox(len(mfp_in), 779, 1)
            is_mi, t, beta = m.sample_mfp(depth)
            mfp_in.append([mi, depth]); mfp_out.append(np.concatenate([[float(bool(is_mi)), t], np.float32(beta.to_numpy()), [ti.RNG.draw]]))
            incid, outd = rand_dir(), rand_dir()
            if k % 6 == 0:
                outd = incid.copy()                       # straight on (cos = -1 for eval_p)
            if k % 6 == 1:
                outd = -incid
            ti.RNG.set_philox(len(sc_in), 780, 1)
            d, s, pdf = m.sample_new_rays(vec3(incid))
            sc_in.append(np.concatenate([[mi], incid])); sc_out.append(np.concatenate([np.float32(d.to_numpy()), np.float32(s.to_numpy()), [pdf, ti.RNG.draw]]))
            p = m.eval(vec3(incid), vec3(outd)) if m.is_scattering() else np.float32(1.0)
            tr = m.transmittance(depth)
            ev_in.append(np.concatenate([[mi], incid, outd, [depth]])); ev_out.append(np.concatenate([[p], np.float32(tr.to_numpy())]))
    np.savez_compressed(os.path.join(OUT, "media_functions.npz"), med_i=np.int32(med_i), med_f=np.float32(med_f),
                        mfp_in=np.float32(mfp_in), mfp_out=np.float32(mfp_out), scat_in=np.float32(sc_in), scat_out=np.float32(sc_out),
                        eval_in=np.float32(ev_in), eval_out=np.float32(ev_out))
    print(f"media_functions: {len(objs)} media, {len(mfp_in)} vectors each; medium events {int(np.float32(mfp_out)[:, 0].sum())}")


def gen_volume_functions():
    """GridVolume.intersect_volume / density_lookup_3d / sample_mfp / transmittance (bxdf/volume.py:268-463) on the rows of
    tests/volume_cases.py (the first VOLFUNC_PER rows of every volume x stratum), the reference object built from the packed arrays the
    device and the oracle take.  Philox stream: key = row index within its array, seeds 881 (sample_mfp) / 882 (transmittance)."""
    sys.path.insert(0, os.path.join(refenv.REPO, "tests"))
    import volume_cases as VC
    from taichi.math import mat3
    from bxdf.volume import GridVolume
    from bxdf.phase import PhaseFunction
    vols, groups, dens = VC.same_stream_rows(VC.VOLFUNC_PER, VC.VOLFUNC_DENSITY)
    names = list(vols)
    objs, grids = {}, {}
    for name, (vi, vf, vg) in vols.items():
        grids[name] = ti.Vector.field(3, float, (int(vi[3]), int(vi[2]), int(vi[1])))
        grids[name].from_numpy(vg)
        objs[name] = GridVolume(_type=int(vi[0]), albedo=vec3(vf[0:3]), inv_T=mat3(vf[3:12].reshape(3, 3)), trans=vec3(vf[12:15]),
                                mini=vec3(vf[15:18]), maxi=vec3(vf[18:21]), max_idxs=ti.math.ivec3([int(vi[1]) - 1, int(vi[2]) - 1, int(vi[3]) - 1]),
                                majorant=vec3(vf[21:24]), pdf=vec3(vf[24:27]),
                                ph=PhaseFunction(_type=int(vi[4]), par=vec3(vf[27:30]), pdf=vec3(vf[30:33])))
    ray_vol, ray_in, isect, mfp, trn = [], [], [], [], []
    for name, stratum, rows in groups:
        gv, grid = objs[name], grids[name]
        for x in rows:
            k = len(ray_in)
            o, d, thp, max_t = vec3(x[0:3]), vec3(x[3:6]), vec3(x[6:9]), np.float32(x[9])
            with np.errstate(all="ignore"):
                nf = gv.intersect_volume(o, d, max_t)
                isect.append([float(bool(nf[0] < nf[1] and nf[1] > 0)), nf[0], nf[1]])
                ti.RNG.set_philox(k, VC.SEED_MFP, 1)
                r = gv.sample_mfp(grid, o, d, thp, max_t)
                mfp.append([r[3], r[0], r[1], r[2], ti.RNG.draw])
                ti.RNG.set_philox(k, VC.SEED_TR, 1)
                t = gv.transmittance(grid, o, d, thp, max_t)
                trn.append([t[0], t[1], t[2], ti.RNG.draw])
            ray_vol.append(names.index(name)); ray_in.append(x)
    den_vol, den_in, den_out = [], [], []
    for name, rows in dens:
        for x in rows:
            v = objs[name].density_lookup_3d(grids[name], vec3(x[0:3]), vec3(x[3:6]))
            den_vol.append(names.index(name)); den_in.append(x); den_out.append(v[int(x[6])])
    arrays = dict(ray_vol=np.int32(ray_vol), ray_in=np.float32(ray_in), isect_out=np.float32(isect), mfp_out=np.float32(mfp),
                  tr_out=np.float32(trn), den_vol=np.int32(den_vol), den_in=np.float32(den_in), den_out=np.float32(den_out))
    for j, name in enumerate(names):
        arrays[f"vol{j}_i"], arrays[f"vol{j}_f"], arrays[f"vol{j}_grid"] = vols[name]
    np.savez_compressed(os.path.join(OUT, "volume_functions.npz"), **arrays)
    print(f"volume_functions: {len(names)} volumes, {len(ray_in)} rays ({int(np.float32(isect)[:, 0].sum())} hit, "
          f"{int((np.float32(mfp)[:, 0] > 0).sum())} collisions, most draws {int(np.float32(trn)[:, 3].max())}), {len(den_in)} lookups")


def gen_scene(scene_dir, xml, tag, w, h, spp, overrides, seed=0, n_rays=192):
    ov = dict(overrides); ov.update(width=w, height=h)
    t0 = time.time()
    reseed(f"scene_{tag}.npz")
    rdr, (emitters, arr, objs, cfg) = refenv.make_renderer(scene_dir, xml, ov)
    out = {"width": np.int32(w), "height": np.int32(h), "spp": np.int32(spp), "seed": np.int32(seed),
           "max_bounce": np.int32(rdr.max_bounce), "num_shadow_ray": np.int32(rdr.num_shadow_ray)}

    # --- pix2ray with scripted jitter
    pin, pout = [], []
    for _ in range(24):
        i, j, cnt = int(RS.randint(w)), int(RS.randint(h)), int(RS.randint(1, 40))
        s = RS.rand(2); ti.RNG.set_script(s); rdr.cnt[None] = cnt
        pin.append([i, j, cnt, s[0], s[1]]); pout.append(rdr.pix2ray(i, j).to_numpy())
    rdr.cnt[None] = 0
    out["pix2ray_in"], out["pix2ray_out"] = np.float64(pin), np.float32(pout)

    # --- closest hit / occlusion on a ray batch (camera rays + rays from inside the room)
    O, D, TM = [], [], []
    for k in range(n_rays):
        if k % 3 == 0:
            ti.RNG.set_script(RS.rand(2)); rdr.cnt[None] = 1
            O.append(rdr.cam_t.to_numpy()); D.append(rdr.pix2ray(int(RS.randint(w)), int(RS.randint(h))).to_numpy())
        else:
            O.append(np.float32(RS.uniform([0.2, 0.2, 0.2], [5.3, 5.2, 5.3]))); D.append(rand_dir())
        TM.append(np.float32(RS.uniform(0.5, 6.0)))
    rdr.cnt[None] = 0
    hits, occ = [], []
    for o, d, tm in zip(O, D, TM):
        it = rdr.ray_intersect(vec3(d), vec3(o))
        hits.append(np.concatenate([[it.obj_id, it.prim_id, it.min_depth], it.uv.to_numpy(), it.n_s.to_numpy(), it.n_g.to_numpy()]))
        occ.append(int(bool(rdr.does_intersect(vec3(d), vec3(o), tm))))
    out["ray_o"], out["ray_d"], out["ray_tmax"] = np.float32(O), np.float32(D), np.float32(TM)
    out["ray_hit"], out["ray_occ"] = np.float32(hits), np.int32(occ)

    # --- emitters: sample_hit (scripted), eval_le, solid_angle_pdf
    from tracer.interaction import Interaction
    ein, escr, eout = [], [], []
    for s_idx in range(rdr.src_num):
        for _ in range(16):
            hp = np.float32(RS.uniform([0.2, 0.1, 0.2], [5.3, 5.0, 5.3]))
            scr = np.zeros(4)                          # Philox(key = test index, seed 778, sample 1)
            ti.RNG.set_philox(len(ein), 778, 1)
            pos, inten, pdf, _n = rdr.src_field[s_idx].sample_hit(rdr.precom_vec, rdr.normals, rdr.obj_info, vec3(hp))
            nrm, rd = rand_dir(), rand_dir()
            md = np.float32(RS.uniform(0.5, 5))
            le = rdr.src_field[s_idx].eval_le(vec3(rd * md), vec3(nrm))
            sap = rdr.src_field[s_idx].solid_angle_pdf(Interaction(n_s=vec3(nrm), n_g=vec3(nrm), min_depth=md), vec3(rd))
            ein.append(np.concatenate([[s_idx], hp, nrm, rd, [md]])); escr.append(scr)
            eout.append(np.concatenate([pos.to_numpy(), inten.to_numpy(), [pdf, ti.RNG.draw], le.to_numpy(), [sap]]))
    out["emit_in"], out["emit_script"], out["emit_out"] = np.float32(ein), np.float64(escr), np.float32(eout)

    # --- Texture.query (bilinear atlas lookup) on every declared map, coordinates also outside [0, 1] and negative
    if cfg.get("packed_textures") is not None:
        tq_in, tq_out = [], []
        for m, name in enumerate(("albedo", "normal", "bump")):
            if not getattr(rdr, f"has_{name}_map"):
                continue
            tmap, timg = getattr(rdr, f"{name}_map"), getattr(rdr, f"{name}_img")
            for o in range(rdr.num_objects):
                if tmap[o].type <= -255:
                    continue
                for _ in range(24):
                    u, v = np.float32(RS.uniform(-1.5, 2.5)), np.float32(RS.uniform(-1.5, 2.5))
                    tq_in.append([m, o, u, v]); tq_out.append(tmap[o].query(timg, u, v).to_numpy())
        out["texq_in"], out["texq_out"] = np.float32(tq_in), np.float32(tq_out)

    # --- whole-kernel run on the Philox stream: per-sample colours and draw counts
    colors = np.zeros((spp, w, h, 3), np.float32)
    draws = np.zeros((spp, w, h), np.int32)
    state = {"prev": None}

    def hook(i, j):
        if state["prev"] is not None:
            pi, pj = state["prev"]; draws[state["s"], pi, pj] = ti.RNG.draw
        ti.RNG.set_philox(i * h + j, seed, rdr.cnt[None])
        state["prev"] = (i, j)

    ti.PIXEL_HOOK[0] = hook
    prev = rdr.color.to_numpy().copy()
    for s in range(spp):
        state["s"], state["prev"] = s, None
        rdr.render(0, 0, 0, 0, 0, 0)
        pi, pj = state["prev"]; draws[s, pi, pj] = ti.RNG.draw
        cur = rdr.color.to_numpy()
        colors[s] = cur if s == 0 else (cur - prev)     # exact only for s == 0; per-sample values re-derived below
        prev = cur.copy()
    ti.PIXEL_HOOK[0] = None
    out["accum"], out["pixels"], out["draws"] = rdr.color.to_numpy(), rdr.pixels.to_numpy(), draws
    out["first_sample"] = colors[0]
    np.savez_compressed(os.path.join(OUT, f"scene_{tag}.npz"), **out)
    n = w * h * spp
    print(f"scene_{tag}: {w}x{h}x{spp}spp in {time.time() - t0:.1f}s ({n / (time.time() - t0):.0f} samples/s), "
          f"mean draws {draws.mean():.2f}, mean radiance {out['pixels'].mean():.4f}")


def _whole_kernel(rdr, w, h, spp, seed):
    """`spp` calls of the reference's render kernel on the shared Philox stream (key = pixel, seed, sample number): the accumulated
    image and every sample's draw count"""
    draws = np.zeros((spp, w, h), np.int32)
    state = {"prev": None}

    def hook(i, j):
        if state["prev"] is not None:
            pi, pj = state["prev"]; draws[state["s"], pi, pj] = ti.RNG.draw
        ti.RNG.set_philox(i * h + j, seed, rdr.cnt[None])
        state["prev"] = (i, j)

    ti.PIXEL_HOOK[0] = hook
    for s_ in range(spp):
        state["s"], state["prev"] = s_, None
        rdr.render(0, 0, 0, 0, 0, 0)
        pi, pj = state["prev"]; draws[s_, pi, pj] = ti.RNG.draw
    ti.PIXEL_HOOK[0] = None
    return rdr.color.to_numpy(), draws


def gen_settings():
    """The sensor-settings matrix (tests/settings_cases.py): Renderer.render / VolumeRenderer.render of the reference with each case's
    overrides written into the sensor dict its parser returned.  One file, per case `<name>:accum`, `<name>:draws` and the nine settings
    the reference's renderer was created with (`<name>:<key>`); no random inputs."""
    sys.path.insert(0, os.path.join(refenv.REPO, "tests"))
    import settings_cases as SC
    os.chdir(refenv.REPO)                               # asset paths in this repo's scene files are relative to the repository root
    w, h, spp, seed = SC.FIXTURE_W, SC.FIXTURE_H, SC.FIXTURE_SPP, SC.FIXTURE_SEED
    out = {"names": np.array([c.name for c in SC.CASES]), "width": np.int32(w), "height": np.int32(h), "spp": np.int32(spp), "seed": np.int32(seed)}
    t_all = time.time()
    for case in SC.CASES:
        sdir, fname, ref, vol = SC.SCENES[case.scene]
        scene_dir, xml = ref if ref is not None else (os.path.join(refenv.REPO, "scenes", sdir), fname)
        t0 = time.time()
        rdr, (_, _, _, cfg) = refenv.make_renderer(scene_dir, xml, dict(case.overrides, width=w, height=h), volumetric=vol)
        assert SC.within_queue_limit(int(cfg["num_shadow_ray"]), int(cfg["max_bounce"])), case.name
        accum, draws = _whole_kernel(rdr, w, h, spp, seed)
        out[f"{case.name}:accum"], out[f"{case.name}:draws"] = accum, draws
        eff = {"rr_bounce_th": 4, "rr_threshold": 0.1, "brdf_two_sides": False}
        eff.update({k: cfg[k] for k in SC.SETTING_KEYS if k in cfg})
        for k in SC.SETTING_KEYS:
            out[f"{case.name}:{k}"] = np.float64(eff[k]) if k == "rr_threshold" else np.int32(eff[k])
        print(f"settings {case.name}: {time.time() - t0:.1f}s, mean draws {draws.mean():.2f}, mean radiance {np.nanmean(accum) / spp:.4f}", flush=True)
    np.savez_compressed(os.path.join(OUT, "settings_matrix.npz"), **out)
    print(f"settings_matrix: {len(SC.CASES)} cases at {w}x{h}x{spp}spp in {time.time() - t_all:.0f}s")


# ------------------------------------------------------------------ sweep over the reference's own bundled scenes
def gen_refscene(scene_dir, xml, tag, w, h, spp, seed=0, volumetric=False, overrides=None):
    """Whole-kernel run of one of the reference's bundled scene files (its own parser, its own kernel) plus the parsed
    scene as flat arrays, so that the tests can render exactly that scene without the XML (which stays in /root/reference)."""
    sys.path.insert(0, refenv.REPO)
    from adapt_amd.scene_pack import pack_scene
    t0 = time.time()
    rdr, (emitters, arr, objs, cfg) = refenv.make_renderer(scene_dir, xml, dict({"width": w, "height": h}, **(overrides or {})), volumetric=volumetric)
    fs = pack_scene(emitters, arr, objs, cfg)          # reads the reference's host objects attribute by attribute
    out = {"med_i": fs.med_i, "med_f": fs.med_f, "volumetric": np.int32(volumetric), "prims": fs.prims, "normals": fs.normals, "v_normals": fs.v_normals, "obj_info": fs.obj_info, "obj_aabb": fs.obj_aabb,
           "emitter_id": fs.emitter_id, "bxdf_i": fs.bxdf_i, "bxdf_f": fs.bxdf_f, "src_i": fs.src_i, "src_f": fs.src_f,
           "has_vertex_normal": np.int32(fs.has_vertex_normal), "world_ior": np.float32(fs.world_ior),
           "width": np.int32(w), "height": np.int32(h), "spp": np.int32(spp), "seed": np.int32(seed),
           "fov": np.float64(cfg["fov"]), "max_bounce": np.int32(cfg["max_bounce"]), "num_shadow_ray": np.int32(cfg["num_shadow_ray"]),
           "use_rr": np.int32(cfg["use_rr"]), "use_mis": np.int32(cfg["use_mis"]), "anti_alias": np.int32(cfg["anti_alias"]),
           "stratified_sampling": np.int32(cfg["stratified_sampling"]), "brdf_two_sides": np.int32(cfg.get("brdf_two_sides", False)),
           "accelerator_bvh": np.int32(cfg.get("accelerator", "none") == "bvh"),
           "rr_bounce_th": np.int32(cfg.get("rr_bounce_th", 4)), "rr_threshold": np.float64(cfg.get("rr_threshold", 0.1)),
           "cam_dir": np.float32(cfg["transform"][0]), "cam_pos": np.float32(cfg["transform"][1])}
    draws = np.zeros((spp, w, h), np.int32)
    state = {"prev": None}

    def hook(i, j):
        if state["prev"] is not None:
            pi, pj = state["prev"]; draws[state["s"], pi, pj] = ti.RNG.draw
        ti.RNG.set_philox(i * h + j, seed, rdr.cnt[None])
        state["prev"] = (i, j)

    ti.PIXEL_HOOK[0] = hook
    for s_ in range(spp):
        state["s"], state["prev"] = s_, None
        rdr.render(0, 0, 0, 0, 0, 0)
        pi, pj = state["prev"]; draws[s_, pi, pj] = ti.RNG.draw
    ti.PIXEL_HOOK[0] = None
    out["accum"], out["draws"] = rdr.color.to_numpy(), draws
    np.savez_compressed(os.path.join(OUT, f"{'vptscene' if volumetric else 'refscene'}_{tag}.npz"), **out)
    print(f"{'vptscene' if volumetric else 'refscene'}_{tag}: {fs.n_prims} prims, {fs.n_objects} objects, {fs.n_sources} sources, {w}x{h}x{spp}spp, bounces {int(cfg['max_bounce'])}, "
          f"{time.time() - t0:.1f}s, mean draws {draws.mean():.2f}, mean radiance {np.nanmean(out['accum']) / spp:.4f}")


def gen_vptrun(scene_dir, xml, tag, w, h, spp, seed=0):
    """VolumeRenderer.render of the reference on a scene file of this repo that the tests parse themselves: only the accumulated
    image and the per-sample draw counts are stored."""
    rdr, (emitters, arr, objs, cfg) = refenv.make_renderer(scene_dir, xml, {"width": w, "height": h}, volumetric=True)
    draws = np.zeros((spp, w, h), np.int32)
    state = {"prev": None}

    def hook(i, j):
        if state["prev"] is not None:
            pi, pj = state["prev"]; draws[state["s"], pi, pj] = ti.RNG.draw
        ti.RNG.set_philox(i * h + j, seed, rdr.cnt[None])
        state["prev"] = (i, j)

    ti.PIXEL_HOOK[0] = hook
    t0 = time.time()
    for s_ in range(spp):
        state["s"], state["prev"] = s_, None
        rdr.render(0, 0, 0, 0, 0, 0)
        pi, pj = state["prev"]; draws[s_, pi, pj] = ti.RNG.draw
    ti.PIXEL_HOOK[0] = None
    extra = {}
    if getattr(rdr, "has_volume", False):               # the reference's exported grid-volume record and density grid
        v = rdr.volume
        tn = lambda x: np.float32(x.to_numpy() if hasattr(x, "to_numpy") else x)
        extra["vol_f"] = np.concatenate([tn(v.albedo), tn(v.inv_T).reshape(-1), tn(v.trans), tn(v.mini), tn(v.maxi), tn(v.majorant), tn(v.pdf),
                                         tn(v.ph.par), tn(v.ph.pdf)]).astype(np.float32)
        extra["vol_i"] = np.int32([int(v._type), int(v.max_idxs[0]) + 1, int(v.max_idxs[1]) + 1, int(v.max_idxs[2]) + 1, int(v.ph._type)])
        extra["vol_grid"] = np.float32(rdr.density_grid.to_numpy())
    np.savez_compressed(os.path.join(OUT, f"vptrun_{tag}.npz"), accum=rdr.color.to_numpy(), draws=draws, width=np.int32(w), height=np.int32(h),
                        spp=np.int32(spp), seed=np.int32(seed), max_bounce=np.int32(cfg["max_bounce"]), **extra)
    print(f"vptrun_{tag}: {w}x{h}x{spp}spp, {time.time() - t0:.1f}s, mean draws {draws.mean():.2f}, mean radiance {np.nanmean(rdr.color.to_numpy()) / spp:.4f}")


# ------------------------------------------------------------------ the reference's BVH path (accelerator = bvh)
def _write_obj(path, tris, flat_normals):
    """(n,3,3) float32 triangles -> OBJ with per-face `vn` (like meshes/cornell/bunny.obj); %.9g round-trips float32 exactly"""
    with open(path, "w") as f:
        for t in tris.reshape(-1, 3):
            f.write("v %.9g %.9g %.9g\n" % tuple(float(x) for x in t))
        for n in flat_normals:
            f.write("vn %.9g %.9g %.9g\n" % tuple(float(x) for x in n))
        for k in range(tris.shape[0]):
            f.write("f %d//%d %d//%d %d//%d\n" % (3 * k + 1, k + 1, 3 * k + 2, k + 1, 3 * k + 3, k + 1))


def write_three_bunnies(tmp, levels):
    """adapt_amd.synth.three_bunnies(levels) as a scene directory the REFERENCE parser can load (temporary files, not committed):
    the placed bunnies as OBJ files + an XML with the same materials / lights / sensor.  Returns (dir, xml, synth 4-tuple)."""
    import shutil
    from adapt_amd import synth
    em, arr, objs, cfg = synth.three_bunnies(levels)
    os.makedirs(os.path.join(tmp, "meshes"), exist_ok=True)
    mesh_dir = os.path.join(refenv.REPO, "scenes", "meshes", "cornell")
    for name in ("floor", "ceiling", "back", "greenwall", "redwall"):
        shutil.copy(os.path.join(mesh_dir, f"cbox_{name}.obj"), os.path.join(tmp, "meshes"))
    start = 10
    for k in range(3):
        n = objs[5 + k].tri_num
        tris = arr["primitives"][start:start + n]
        _write_obj(os.path.join(tmp, "meshes", f"bunny{k}.obj"), tris, arr["n_g"][start:start + n])
        start += n
    spots = ((("6.0, 4.0, 4.0", "245.0", (3.779, 5.2, 2.745), (-0.2, -1.5, -0.3), 20.0)), ("6.0, 6.0, 4.0", "200.0", (1.2, 4.8, 3.2), (0.6, -1.5, -0.05), 15.0),
             ("4.0, 4.0, 6.0", "200.0", (4.9, 2.5, 3.8), (-1.6, -0.6, -0.4), 15.0))
    x = ['<?xml version="1.0" encoding="utf-8"?>', '<scene version="1.1">', '<sensor type="perspective">', '<float name="fov" value="39.3077"/>',
         '<integer name="max_bounce" value="8"/>', '<integer name="num_shadow_ray" value="2"/>', '<boolean name="use_rr" value="true"/>',
         '<boolean name="anti_alias" value="true"/>', '<boolean name="stratified_sampling" value="true"/>', '<boolean name="use_mis" value="true"/>',
         '<string name="accelerator" value="bvh"/>',
         '<transform name="toWorld"><lookat target="2.78, 2.73, -7.0" origin="2.78, 2.73, -8.0" up="0, 1, 0"/></transform>',
         '<film type="film"><integer name="width" value="800"/><integer name="height" value="800"/></film>', '</sensor>']
    for ident, kd in (("white", "#BDBDBD"), ("left", "#DD2525"), ("right", "#25DD25"), ("lava", "#FFFFFF")):
        x.append(f'<brdf type="lambertian" id="{ident}"><rgb name="k_d" value="{kd}"/><rgb name="k_g" value="1.0"/><rgb name="k_s" value="0.0"/></brdf>')
    x.append('<bsdf type="det-refraction" id="glass"><rgb name="k_d" value="#FFFFFF"/><medium type="transparent"><float name="ior" value="1.5"/></medium></bsdf>')
    x.append('<brdf type="fresnel-blend" id="fresnel"><rgb name="k_d" value="#CACACA"/><rgb name="k_s" value="#333333"/><rgb name="k_g" r="10" g="1000"/></brdf>')
    for k, (e, sc, pos, d, ha) in enumerate(spots):
        x.append(f'<emitter type="spot" id="source{k + 1}"><rgb name="emission" value="{e}"/><rgb name="scaler" value="{sc}"/>'
                 f'<point name="pos" x="{pos[0]}" y="{pos[1]}" z="{pos[2]}"/><point name="dir" x="{d[0]}" y="{d[1]}" z="{d[2]}"/><float name="half-angle" value="{ha}"/></emitter>')
    for name, mat in (("floor", "white"), ("ceiling", "white"), ("back", "white"), ("greenwall", "right"), ("redwall", "left")):
        x.append(f'<shape type="obj"><string name="filename" value="meshes/cbox_{name}.obj"/><ref type="material" id="{mat}"/></shape>')
    for k, mat in enumerate(("lava", "glass", "fresnel")):
        x.append(f'<shape type="obj"><string name="filename" value="meshes/bunny{k}.obj"/><ref type="material" id="{mat}"/></shape>')
    x += ['<world name="w"><medium type="transparent"><float name="ior" value="1.0"/></medium></world>', '</scene>']
    with open(os.path.join(tmp, "three_bunnies.xml"), "w") as f:
        f.write("\n".join(x))
    return tmp, "three_bunnies.xml", (em, arr, objs, cfg)


def _ray_batch(rs, rdr, n, w, h, lo=(0.3, 0.2, 0.3), hi=(5.2, 5.2, 5.2)):
    O, D, TM = [], [], []
    for k in range(n):
        if k % 3 == 0:
            ti.RNG.set_script(rs.rand(2)); rdr.cnt[None] = 1
            O.append(rdr.cam_t.to_numpy()); D.append(rdr.pix2ray(int(rs.randint(w)), int(rs.randint(h))).to_numpy())
        else:
            d = np.float32(rs.normal(size=3)); d /= np.float32(np.linalg.norm(d))
            O.append(np.float32(rs.uniform(lo, hi))); D.append(np.float32(d))
        TM.append(np.float32(rs.uniform(0.3, 6.0)))
    rdr.cnt[None] = 0
    return np.float32(O), np.float32(D), np.float32(TM)


def _trace_batch(rdr, O, D, TM, closest, anyhit):
    hits, occ = [], []
    for o, d, tm in zip(O, D, TM):
        it = closest(vec3(d), vec3(o))
        hits.append(np.concatenate([[it.obj_id, it.prim_id, it.min_depth], it.uv.to_numpy(), it.n_s.to_numpy(), it.n_g.to_numpy()]))
        occ.append(int(bool(anyhit(vec3(d), vec3(o), tm))))
    return np.float32(hits), np.int32(occ)


def gen_bvhref(tag, scene_dir, xml, w, h, spp, n_rays, seed=0, synth_check=None, extra_rays=None, brute_rays=0, store_scene=True, overrides=None):
    """The reference's BVH path pinned with the reference's own traversal code: `PathTracer.bvh_process` imports `bvh_cpp` (the
    stand-in in shim/: tree from the builder restated in the oracle, reference layout), `convert_bvh_info` fills the LinearNode /
    LinearBVH fields, and `ray_intersect_bvh` / `does_intersect_bvh` (path_tracer.py:338-422, ti_bvh.py) answer a ray batch and render
    the image.  Stored: the rays, the hits, the occlusion flags, the image + draw counts, the tree's node count (the four arrays
    themselves for small scenes), and for `brute_rays` of the rays also the answer of the reference's brute-force intersector
    (tracer_base.py:168-278) - which is what decides whether the reference's two intersectors agree on a scene."""
    sys.path.insert(0, refenv.REPO)
    import hashlib
    import bvh_cpp
    from adapt_amd.scene_pack import pack_scene
    from tracer.tracer_base import TracerBase
    rs = np.random.RandomState({"cbox": 411, "bunnies1": 412, "bunnies3": 413}.get(tag, 499))      # own stream: `--only bvh` reproduces the committed files
    t0 = time.time()
    ov = dict({"width": w, "height": h, "accelerator": "bvh"}, **(overrides or {}))
    rdr, (emitters, arr, objs, cfg) = refenv.make_renderer(scene_dir, xml, ov)
    assert getattr(rdr, "node_num", 0) > 0 and rdr.ray_intersect.__func__ is type(rdr).ray_intersect_bvh, "the BVH path is not active"
    fs = pack_scene(emitters, arr, objs, cfg)
    if synth_check is not None:                       # the temporary scene directory reproduces the synthetic scene array for array
        from adapt_amd.scene_pack import pack_scene as ps
        fs2 = ps(*synth_check)
        for name in ("prims", "normals", "v_normals", "obj_info", "obj_aabb", "emitter_id", "bxdf_i", "bxdf_f", "src_i", "src_f"):
            assert np.array_equal(getattr(fs, name), getattr(fs2, name)), f"reference parser vs synth: {name} differs"
    bvh_mm, node_mm, bvh_info, node_info = [np.asarray(a) for a in bvh_cpp.LAST["arrays"]]
    out = {"tree_source": np.array(bvh_cpp.LAST["source"]), "node_num": np.int32(rdr.node_num), "bvh_num": np.int32(rdr.bvh_num),
           "prims_sha256": np.array(hashlib.sha256(np.ascontiguousarray(fs.prims).tobytes()).hexdigest()),
           "width": np.int32(w), "height": np.int32(h), "spp": np.int32(spp), "seed": np.int32(seed),
           "max_bounce": np.int32(cfg["max_bounce"]), "num_shadow_ray": np.int32(cfg["num_shadow_ray"])}
    if rdr.node_num <= 20000:
        out.update(bvh_minmax=bvh_mm.reshape(-1, 2, 3), node_minmax=node_mm.reshape(-1, 2, 3), bvh_info=bvh_info.reshape(-1, 2), node_info=node_info.reshape(-1, 3))
    if store_scene:
        out.update({"prims": fs.prims, "normals": fs.normals, "v_normals": fs.v_normals, "obj_info": fs.obj_info, "obj_aabb": fs.obj_aabb,
                    "emitter_id": fs.emitter_id, "bxdf_i": fs.bxdf_i, "bxdf_f": fs.bxdf_f, "src_i": fs.src_i, "src_f": fs.src_f,
                    "has_vertex_normal": np.int32(fs.has_vertex_normal), "world_ior": np.float32(fs.world_ior), "fov": np.float64(cfg["fov"]),
                    "use_rr": np.int32(cfg["use_rr"]), "use_mis": np.int32(cfg["use_mis"]), "anti_alias": np.int32(cfg["anti_alias"]),
                    "stratified_sampling": np.int32(cfg["stratified_sampling"]), "brdf_two_sides": np.int32(cfg.get("brdf_two_sides", False)),
                    "accelerator_bvh": np.int32(1), "rr_bounce_th": np.int32(cfg.get("rr_bounce_th", 4)), "rr_threshold": np.float64(cfg.get("rr_threshold", 0.1)),
                    "cam_dir": np.float32(cfg["transform"][0]), "cam_pos": np.float32(cfg["transform"][1])})
    O, D, TM = _ray_batch(rs, rdr, n_rays, w, h)
    if extra_rays is not None:
        eo, ed, etm = extra_rays(fs, cfg)
        O, D, TM = np.concatenate([eo, O]), np.concatenate([ed, D]), np.concatenate([etm, TM])
    out["ray_o"], out["ray_d"], out["ray_tmax"] = O, D, TM
    out["bvh_hit"], out["bvh_occ"] = _trace_batch(rdr, O, D, TM, rdr.ray_intersect, rdr.does_intersect)
    print(f"bvhref_{tag}: {rdr.node_num} nodes / {rdr.bvh_num} prims, {len(O)} rays traced through the BVH in {time.time() - t0:.1f}s", flush=True)
    if brute_rays:
        nb = min(brute_rays if brute_rays > 0 else getattr(disputed_rays_95k, 'count', 0), len(O))
        out["brute_hit"], out["brute_occ"] = _trace_batch(rdr, O[:nb], D[:nb], TM[:nb], lambda d, o: TracerBase.ray_intersect(rdr, d, o),
                                                          lambda d, o, tm: TracerBase.does_intersect(rdr, d, o, tm))
        nd = int((out["brute_hit"][:, 1] != out["bvh_hit"][:nb, 1]).sum()); no = int((out["brute_occ"] != out["bvh_occ"][:nb]).sum())
        print(f"bvhref_{tag}: brute force on the first {nb} rays in {time.time() - t0:.1f}s: {nd} closest hits and {no} occlusion flags differ from the BVH path", flush=True)
    if spp > 0:
        draws = np.zeros((spp, w, h), np.int32)
        state = {"prev": None}

        def hook(i, j):
            if state["prev"] is not None:
                pi, pj = state["prev"]; draws[state["s"], pi, pj] = ti.RNG.draw
            ti.RNG.set_philox(i * h + j, seed, rdr.cnt[None])
            state["prev"] = (i, j)

        ti.PIXEL_HOOK[0] = hook
        for s_ in range(spp):
            state["s"], state["prev"] = s_, None
            rdr.render(0, 0, 0, 0, 0, 0)
            pi, pj = state["prev"]; draws[s_, pi, pj] = ti.RNG.draw
        ti.PIXEL_HOOK[0] = None
        out["accum"], out["draws"] = rdr.color.to_numpy(), draws
    np.savez_compressed(os.path.join(OUT, f"bvhref_{tag}.npz"), **out)
    print(f"bvhref_{tag}: done in {time.time() - t0:.1f}s" + (f", mean draws {out['draws'].mean():.2f}, mean radiance {np.nanmean(out['accum']) / spp:.4f}" if spp > 0 else ""), flush=True)


def disputed_rays_95k(fs, cfg):
    """Rays of the 95 050-triangle scene on which the oracle's two intersectors (brute force vs reference-layout BVH) disagree, found
    among 300 000 random rays, plus as many rays on which they agree: the reference's own two intersectors then answer exactly these."""
    from adapt_amd.scene_pack import make_config
    from oracle import binding as ob
    rs = np.random.RandomState(414)
    rc = make_config(cfg)
    sc = ob.OracleScene(fs, rc.cam_t, build_bvh=True)
    n = 300000
    o = rs.uniform([0.3, 0.2, 0.3], [5.2, 5.2, 5.2], size=(n, 3)).astype(np.float32)
    d = rs.normal(size=(n, 3)).astype(np.float32); d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    tm = rs.uniform(0.3, 6.0, n).astype(np.float32)
    _, p0, t0, _, _ = sc.intersect(o, d, use_bvh=False)
    _, p1, t1, _, _ = sc.intersect(o, d, use_bvh=True)
    bad = np.nonzero((p0 != p1) | (t0 != t1))[0]
    occ_bad = np.nonzero(sc.occluded(o, d, tm, use_bvh=False) != sc.occluded(o, d, tm, use_bvh=True))[0]
    pick = np.unique(np.concatenate([bad[:40], occ_bad[:8]]))
    good = np.setdiff1d(np.arange(n), np.concatenate([bad, occ_bad]))[:len(pick)]
    idx = np.concatenate([pick, good])
    print(f"95k scene: oracle brute force vs oracle reference-layout BVH on {n} rays: {len(bad)} closest hits differ, {len(occ_bad)} occlusion flags differ; "
          f"{len(pick)} disputed + {len(good)} undisputed rays go to the reference", flush=True)
    disputed_rays_95k.count = len(idx)
    return o[idx], d[idx], tm[idx]


REF_SCENES = [("cbox", "cbox-point.xml"), ("cbox", "cbox-vn.xml"), ("cbox", "smaller.xml"), ("cbox", "single-orb.xml"), ("cbox", "ite-orb.xml"),
              ("cbox", "skeleton.xml"), ("cbox", "vader.xml"), ("cbox", "venus.xml"), ("cbox", "bvh-benchmark.xml"),
              ("csphere", "balls-glossy.xml"), ("csphere", "balls-multi.xml"), ("csphere", "big.xml"), ("csphere", "mix-balls.xml"),
              ("csphere", "single-ball.xml"), ("csphere", "whiskey.xml"), ("trans", "cbox-collimated.xml"), ("trans", "cbox-point.xml"), ("trans", "balls-mono.xml")]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="all")
    ap.add_argument("--out", default="", help="write the fixtures into this directory instead of tests/golden/ (check_freshness.py)")
    a = ap.parse_args()
    if a.out:
        OUT = os.path.abspath(a.out)
    if a.only == "microfacet":
        if os.environ.get("ADAPT_REF_MICROFACET") != "1":                  # the switch is read when bxdf.brdf is imported: own process
            os.execve(sys.executable, [sys.executable] + sys.argv, dict(os.environ, ADAPT_REF_MICROFACET="1"))
        gen_microfacet_functions()
        gen_scene(os.path.join(refenv.REPO, "scenes", "test"), "microfacet.xml", "microfacet", 40, 30, 4, {}, n_rays=48)
        gen_vptrun(os.path.join(refenv.REPO, "scenes", "test"), "microfacet.xml", "microfacet", 40, 30, 2)       # the same BRDFs in the volumetric loop
        sys.exit(0)
    if a.only == "settings":
        gen_settings()
        sys.exit(0)
    if a.only in ("all", "parse"):
        dump_parse("cbox", "cbox.xml", "cbox")
        dump_parse("csphere", "balls-mono.xml", "balls_mono")
        dump_parse("cbox", "complex.xml", "complex")
        dump_ref_parser_objects("cbox", "cbox.xml", "cbox")
        dump_ref_parser_objects("csphere", "balls-mono.xml", "balls_mono")
        dump_ref_parser_objects("cbox", "complex.xml", "glass_box")
        dump_ref_parser_textures()
    if a.only in ("all", "func"):
        gen_functions()
    if a.only in ("all", "image"):
        gen_scene("cbox", "cbox.xml", "cbox", 32, 32, 6, {"max_bounce": 8})
        gen_scene("csphere", "balls-mono.xml", "balls_mono", 24, 24, 3, {})
        gen_scene("cbox", "complex.xml", "complex", 20, 20, 3, {})
    if a.only in ("all", "refscenes"):
        # every pt-renderable scene file the reference bundles whose assets are in its tree
        for sdir, xml in REF_SCENES:
            tag = (sdir + "_" + xml[:-4]).replace("-", "_")
            try:
                gen_refscene(sdir, xml, tag, 32, 24, 2)
            except Exception as e:                      # missing mesh / texture / volume assets: not loadable here
                print(f"refscene_{tag}: SKIPPED ({type(e).__name__}: {str(e)[:120]})")
    if a.only in ("all", "bvh"):
        import tempfile
        gen_bvhref("cbox", "cbox", "cbox.xml", 32, 32, 4, 256, brute_rays=256, overrides={"max_bounce": 8})
        with tempfile.TemporaryDirectory() as tmp:
            sdir, xml, synth4 = write_three_bunnies(tmp, 1)
            gen_bvhref("bunnies1", sdir, xml, 24, 24, 2, 384, synth_check=synth4, brute_rays=48, store_scene=False)
        with tempfile.TemporaryDirectory() as tmp:
            sdir, xml, synth4 = write_three_bunnies(tmp, 3)
            gen_bvhref("bunnies3", sdir, xml, 800, 800, 0, 600, synth_check=synth4, extra_rays=disputed_rays_95k, brute_rays=-1, store_scene=False)
    if a.only in ("all", "func", "media"):
        gen_media_functions()
    if a.only in ("all", "func", "volfunc"):
        gen_volume_functions()
    if a.only in ("all", "vpt"):
        # the reference's volumetric scenes (homogeneous media) through its own VolumeRenderer.render
        for sdir, xml, ov in (("vpt", "cbox.xml", {}), ("vpt", "balls.xml", {"max_bounce": 12}), ("vpt", "volbox.xml", {})):
            gen_refscene(sdir, xml, (sdir + "_" + xml[:-4]).replace("-", "_"), 32, 24, 2, volumetric=True, overrides=ov)
        # media coverage scenes authored in this repo (multi-H-G world, Rayleigh, media inside glass / frosted balls, several lights)
        test_dir = os.path.join(refenv.REPO, "scenes", "test")
        gen_refscene(test_dir, "media_a.xml", "media_a", 40, 30, 3, volumetric=True)
        gen_refscene(test_dir, "media_b.xml", "media_b", 40, 30, 3, volumetric=True)
        gen_refscene(test_dir, "null_panes.xml", "null_panes", 40, 30, 3, volumetric=True)      # four null-surface panes: track_ray to its seven-segment limit
        # surface-only scenes through the volumetric loop (the reference's default renderer type): every BRDF / BSDF / emitter type,
        # and image textures (vpt.py looks up the albedo map only)
        os.chdir(refenv.REPO)                           # texture paths in textured.xml are relative to the repository root
        for name in ("features_a", "features_b", "textured"):
            gen_vptrun(test_dir, name + ".xml", name, 40, 30, 2)
    if a.only in ("all", "vpt", "volgrid"):
        os.chdir(refenv.REPO)                           # the .vol paths in the scene files are relative to the repository root
        test_dir = os.path.join(refenv.REPO, "scenes", "test")
        for name in ("volgrid_a", "volgrid_b"):
            gen_vptrun(test_dir, name + ".xml", name, 40, 30, 3)
    if a.only in ("all", "image", "features"):
        # feature-coverage scenes authored in this repo (scenes/test/*.xml), run through the reference's own parser + kernel
        test_dir = os.path.join(refenv.REPO, "scenes", "test")
        gen_scene(test_dir, "features_a.xml", "features_a", 40, 30, 3, {}, n_rays=96)
        gen_scene(test_dir, "features_b.xml", "features_b", 40, 30, 3, {}, n_rays=96)
        gen_scene(test_dir, "features_c.xml", "features_c", 40, 30, 3, {}, n_rays=96)
    if a.only in ("all", "image", "features", "textured"):
        os.chdir(refenv.REPO)                           # texture paths in the scene file are relative to the repository root
        gen_scene(os.path.join(refenv.REPO, "scenes", "test"), "textured.xml", "textured", 40, 30, 3, {}, n_rays=96)
