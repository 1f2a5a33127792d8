#!/usr/bin/env python3
"""Fixtures of the direct-light viewer: the reference's unmodified renderer/direct_render.py, imported through refenv
under the `taichi` stand-in, run on scenes this repository ships (given by absolute path).

    python tests/golden/gen/gen_direct.py [--only CASE]

Per case tests/golden/direct_<case>.npz: `pixels` after render(emit_pos) for every light position, depth_map, norm_map, the positions, the
intensity and the settings used.  BlinnPhongTracer draws no random number: no pixel hook, no stream.  Taichi bakes the Python floats a
kernel captures as f32 constants: the tracer's float attributes are rounded (refenv.f32_constants) before the first render.

Light positions, per case (the test's notes say why each is there):
  own      the scene's first point emitter's position (a scene without one: OWN_WITHOUT_POINT, and its first emitter's intensity)
  wall     1e-3 off the surface a chosen pixel's ray hits, along the normal towards the camera: 1 / (1e-5 + d^2) near its 1e5 cap.  The
           pixel is taken from the visible face with the FEWEST pixels: a light 1e-3 above a face makes the shadow ray of every pixel of that
           face further than 0.2 away re-cross the face's own plane beyond the 1e-4 gate or not, by the sign of the hit point's rounding
           error - the reference's own coin toss, which the tests keep below 0.25 % of the film (tests/test_direct_host.py)
  outside  far above the scene's box: every hit pixel that is not on the outside is occluded
  behind   behind the camera, on its axis
  graze    0.1 above the plane of the visible face with the MOST pixels, 0.7 along a tangent from their centroid: grazing light on a large
           face.  (IN the plane every one of the face's pixels is such a coin toss: 16 of 432 pixels on features_a; 0.05 above, still 4 of 768 on cbox.  dot(h, n_s) <= 0 comes
           from `outside` and `behind`, whose light is behind many surfaces.)
Authoring container only; data out only."""
import argparse
import copy
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refenv                                                   # noqa: E402

ti = refenv.setup()
OUT = os.path.abspath(os.path.join(HERE, ".."))
SCENES = os.path.join(refenv.REPO, "scenes")

CROP = {"crop_x": 14, "crop_y": 11, "crop_rx": 9, "crop_ry": 6}
ALL = ("own", "wall", "outside", "behind", "graze")
# case -> (scene directory below scenes/, file, width, height, sensor overrides, film overrides, k_g overrides {object index: rgb},
#          the positions kept: all five on cbox; fewer elsewhere, because the whole set of fixtures is held below 90 KB and a frame is 5 KB)
CASES = {
    "cbox": ("cbox", "c2_cbox.xml", 32, 24, {"anti_alias": False}, {}, {}, ALL),
    "cbox_50x30": ("cbox", "c2_cbox.xml", 50, 30, {"anti_alias": False}, {}, {}, ("own",)),
    "balls_mono": ("csphere", "c3_balls_mono.xml", 24, 24, {}, {}, {}, ("own", "wall", "graze")),
    "textured": ("test", "textured.xml", 24, 18, {}, {}, {}, ("own", "wall", "graze")),
    "features_a": ("test", "features_a.xml", 24, 18, {}, {}, {}, ("own", "wall", "behind", "graze")),
    # a zero channel of k_g: pow(0, 0) = 1 where dot(h, n_s) <= 0.  No shipped material has one, so two objects' k_g are set after parsing
    "features_a_kg0": ("test", "features_a.xml", 24, 18, {}, {}, {7: (0.0, 2.0, 0.5), 3: (0.0, 0.0, 0.0)}, ("outside", "graze")),       # (objects that see dot <= 0 under these two lights)
    "cbox_crop": ("cbox", "c2_cbox.xml", 32, 24, {"anti_alias": False}, CROP, {}, ("own",)),                          # must equal cbox: the loop has no crop test
    "cbox_aa": ("cbox", "c2_cbox.xml", 32, 24, {"anti_alias": True, "stratified_sampling": True}, {}, {}, ("own",)),   # must equal cbox: TracerBase fixes anti_alias = False
}
OWN_WITHOUT_POINT = np.float32([3.5, 4.5, 0.0])                # a scene whose emitters are all area lights (csphere): a point below its ceiling, near the open front


def first_point(emitters):
    for e in emitters:
        if getattr(e, "type", None) == "point":
            return e
    return emitters[0]


def light_positions(rdr, own):
    """the five positions, from the tracer's own first frame (depth and normal map) and its pix2ray"""
    w, h = rdr.w, rdr.h
    depth, normal = rdr.depth_map.to_numpy(), rdr.norm_map.to_numpy()
    cam_t = np.float32(rdr.cam_t.to_numpy() if hasattr(rdr.cam_t, "to_numpy") else np.asarray(getattr(rdr.cam_t, "a", rdr.cam_t)))

    def hit_of(i, j):
        ray = np.float32(getattr(rdr.pix2ray(i, j), "a", None))
        n = normal[i, j] / np.linalg.norm(normal[i, j])
        if np.dot(n, ray) > 0:
            n = -n
        return cam_t + ray * depth[i, j], n.astype(np.float32)

    # the visible faces: hit pixels grouped by plane (unit normal to 2 decimals, offset to 1); every pixel of a sphere is a face of its own
    faces = {}
    for i in range(w):
        for j in range(h):
            if depth[i, j] > 0:
                p, n = hit_of(i, j)
                faces.setdefault((tuple(np.round(n, 2).tolist()), round(float(np.dot(n, p)), 1)), []).append((i, j, p, n))
    off_centre = lambda q: (q[0] - w / 2) ** 2 + (q[1] - h / 2) ** 2
    small = min(faces.values(), key=lambda g: (len(g), min(off_centre(q) for q in g)))
    large = max(faces.values(), key=len)
    _, _, pa, na = min(small, key=off_centre)
    pb, nb = np.mean([q[2] for q in large], 0).astype(np.float32), large[0][3]
    tangent = np.cross(nb, np.float32([0.3, 0.5, 0.8])); tangent /= np.linalg.norm(tangent)
    axis = np.float32(np.asarray(getattr(rdr.cam_r, "a", rdr.cam_r)).reshape(3, 3)[:, 2])
    lo = np.float32(rdr.aabbs.to_numpy()[:, 0].min(0)); hi = np.float32(rdr.aabbs.to_numpy()[:, 1].max(0))
    outside = np.float32([(lo[0] + hi[0]) / 2, hi[1] + 4.0, (lo[2] + hi[2]) / 2])
    names = list(ALL)
    pos = np.float32([own, pa + na * np.float32(1e-3), outside, cam_t - axis * np.float32(2.0), pb + tangent * np.float32(0.7) + nb * np.float32(0.1)])
    return names, pos


def gen_case(name):
    scene_dir, xml, w, h, sensor, film, kg, keep = CASES[name]
    from parsers.xml_parser import scene_parsing
    from renderer.direct_render import BlinnPhongTracer
    from taichi.math import vec3
    t0 = time.time()
    emitters, array_info, objs, cfg = scene_parsing(os.path.join(SCENES, scene_dir), xml)
    cfg["film"]["width"], cfg["film"]["height"] = w, h
    cfg["film"].update(film)
    cfg.update(sensor)
    for k, rgb in kg.items():
        objs[k].bsdf = copy.copy(objs[k].bsdf)                  # (objects of one material share the parser's BSDF instance: this object's alone)
        objs[k].bsdf.k_g = np.float32(rgb)
    emitter = first_point(emitters)
    rdr = BlinnPhongTracer(emitter, array_info, objs, cfg)
    refenv.f32_constants(rdr)
    own = np.float32(emitter.pos) if getattr(emitter, "type", None) == "point" else OWN_WITHOUT_POINT
    rdr.render(vec3(own))
    names, pos = light_positions(rdr, own)
    pos = np.float32([p for n, p in zip(names, pos) if n in keep]); names = [n for n in names if n in keep]
    frames = np.zeros((len(pos), w, h, 3), np.float32)
    for f, p in enumerate(pos):
        rdr.render(vec3(p))
        frames[f] = rdr.pixels.to_numpy()
    depth, normal = rdr.depth_map.to_numpy().astype(np.float32), rdr.norm_map.to_numpy().astype(np.float32)
    # (few entries: an entry of the archive costs 150 bytes of headers, and the set's size is bounded)
    # settings: width, height, has_vertex_normal, the sensor's anti_alias and stratified_sampling, crop_x, crop_y, crop_rx, crop_ry, cnt after the last render
    settings = np.int32([w, h, bool(cfg["has_vertex_normal"]), bool(cfg.get("anti_alias", False)), bool(cfg.get("stratified_sampling", False)),
                         *[film.get(k, 0) for k in ("crop_x", "crop_y", "crop_rx", "crop_ry")], rdr.cnt[None]])
    out = {"settings": settings, "positions": pos, "position_names": np.array(names), "intensity": np.float32(emitter.intensity),
           "pixels": frames, "depth_map": depth, "norm_map": normal,
           "kg": np.float32([[k, *kg[k]] for k in sorted(kg)]).reshape(-1, 4)}      # rows (object index, k_g rgb) set after parsing
    np.savez_compressed(os.path.join(OUT, f"direct_{name}.npz"), **out)
    length = np.linalg.norm(normal, axis=-1)[depth > 0]
    print(f"direct_{name}: {w}x{h}, {len(pos)} positions in {time.time() - t0:.1f}s; hit share {np.mean(depth > 0):.3f}, |n_s| in [{length.min():.4f}, {length.max():.4f}], "
          f"frame max {[float(f.max()) for f in frames]}, non-finite {int((~np.isfinite(frames)).sum())}, vertex normals {bool(cfg['has_vertex_normal'])}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    os.chdir(refenv.REPO)                                       # texture paths in scenes/test/textured.xml are relative to the repository root
    for case in CASES:
        if a.only in (None, case):
            gen_case(case)
