#!/usr/bin/env python3
"""Fixtures of the ambient-occlusion renderer: the reference's unmodified renderer/ssao.py, imported through refenv
under the `taichi` stand-in, run on the shared Philox stream.

    python tests/golden/gen/gen_ao.py [--only CASE]

Per case tests/golden/ao_<case>.npz: the depth map the constructor makes, the accumulation after every call of render, `pixels` after the
last one, every call's per-pixel draw counts, the depth pass's per-pixel draw counts and the settings used.  The pixel hook is installed
BEFORE the renderer is constructed: it keys the stream (i * h + j, seed, cnt), and cnt is 0 while the constructor makes the depth map.
Taichi bakes the Python floats a kernel captures as f32 constants; get_depth_map runs inside the constructor, so the renderer's float
attributes are rounded (refenv.f32_constants) by a wrapper around it, not after construction.  Authoring container only; data out only."""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refenv                                                   # noqa: E402

ti = refenv.setup()
OUT = os.path.abspath(os.path.join(HERE, ".."))
TEST_DIR = os.path.join(refenv.REPO, "scenes", "test")

DEFAULTS = {"smp_hemisphere": 32, "depth_samples": 64, "sample_extent": 0.1}      # ssao.py:36-38 (the reference's cbox.xml sets keys of its own: written out here)
# case -> (scene directory, file, width, height, spp, sensor overrides, film overrides)
CASES = {
    "cbox": ("cbox", "cbox.xml", 32, 24, 3, dict(DEFAULTS), {}),
    "cbox_defaults": ("cbox", "cbox.xml", 16, 12, 2, dict(DEFAULTS), {}),
    "balls_mono": ("csphere", "balls-mono.xml", 24, 24, 2, {"smp_hemisphere": 8, "depth_samples": 8}, {}),
    "features_a": (TEST_DIR, "features_a.xml", 24, 18, 2, {"smp_hemisphere": 8, "depth_samples": 8}, {}),
    "textured": (TEST_DIR, "textured.xml", 24, 18, 2, {"smp_hemisphere": 8, "depth_samples": 8}, {}),
    "cbox_crop": ("cbox", "cbox.xml", 32, 24, 2, {"smp_hemisphere": 8, "depth_samples": 8}, {"crop_x": 14, "crop_y": 11, "crop_rx": 9, "crop_ry": 6}),
    "cbox_smp1": ("cbox", "cbox.xml", 16, 12, 2, {"smp_hemisphere": 1, "depth_samples": 4}, {}),
    "cbox_smp33": ("cbox", "cbox.xml", 16, 12, 2, {"smp_hemisphere": 33, "depth_samples": 4}, {}),
    "cbox_depth1": ("cbox", "cbox.xml", 16, 12, 2, {"smp_hemisphere": 8, "depth_samples": 1}, {}),
    "cbox_extent2": ("cbox", "cbox.xml", 16, 12, 2, {"smp_hemisphere": 8, "depth_samples": 4, "sample_extent": 2.0}, {}),
    "cbox_no_aa": ("cbox", "cbox.xml", 16, 12, 2, {"smp_hemisphere": 8, "depth_samples": 4, "anti_alias": False}, {}),
    "cbox_no_strat": ("cbox", "cbox.xml", 16, 12, 2, {"smp_hemisphere": 8, "depth_samples": 4, "stratified_sampling": False}, {}),
}


class _WriteThrough:
    """`color` as ssao.py uses it.  `self.color[i, j][2] += d` writes one component of a field element in place; the stand-in's fields hand
    out copies (its value semantics serve the path tracers, which assign whole elements), so the update would be lost.  This view of the
    same Field hands out element views whose components read and write the field's own array; everything else is the field's."""

    class _Elem:
        def __init__(self, data, key): self._d, self._k = data, key
        def __getitem__(self, c): return ti.f32(self._d[self._k + (int(c),)])
        def __setitem__(self, c, v): self._d[self._k + (int(c),)] = np.float32(v)

    def __init__(self, field): self._f = field
    def __getitem__(self, idx): return self._Elem(self._f.data, tuple(int(q) for q in idx))
    def __setitem__(self, idx, val): self._f[idx] = val
    def __getattr__(self, name): return getattr(self._f, name)
    def __iter__(self): return iter(self._f)


def gen_case(name, seed=0):
    scene_dir, xml, w, h, spp, sensor, film = CASES[name]
    from parsers.xml_parser import scene_parsing
    import renderer.ssao as ssao_module
    from renderer.ssao import SSAORenderer
    t0 = time.time()
    base = scene_dir if os.path.isabs(scene_dir) else os.path.join(refenv.REFERENCE, "scenes", scene_dir)
    emitters, array_info, objs, cfg = scene_parsing(base, xml)
    cfg["film"]["width"], cfg["film"]["height"] = w, h
    cfg["film"].update(film)
    cfg.update(sensor)

    state = {"rdr": None, "prev": None, "draws": None}

    def hook(i, j):
        if state["rdr"] is None:                                # (a 2-D loop of the base constructors, before the depth map)
            return
        if state["prev"] is not None:
            pi, pj = state["prev"]; state["draws"][pi, pj] = ti.RNG.draw
        rdr = state["rdr"]
        ssao_module.ZERO_V3.a[...] = 0                          # `color_vec = ZERO_V3` copies in Taichi; here it binds the module's constant, which color_vec.fill() then overwrites
        ti.RNG.set_philox(i * h + j, seed, rdr.cnt[None])
        state["prev"] = (i, j)

    def flush():
        pi, pj = state["prev"]; state["draws"][pi, pj] = ti.RNG.draw
        state["prev"] = None

    original = SSAORenderer.get_depth_map

    def depth_map_with_f32_constants(self):
        refenv.f32_constants(self)
        self.color = _WriteThrough(self.color)
        state["rdr"] = self
        return original(self)

    depth_draws = np.zeros((w, h), np.int32)
    state["draws"] = depth_draws
    ti.PIXEL_HOOK[0] = hook
    SSAORenderer.get_depth_map = depth_map_with_f32_constants
    try:
        rdr = SSAORenderer(emitters, array_info, objs, cfg)
    finally:
        SSAORenderer.get_depth_map = original
    flush()
    refenv.f32_constants(rdr)
    out = {"width": np.int32(w), "height": np.int32(h), "spp": np.int32(spp), "seed": np.int32(seed),
           "smp_hemisphere": np.int32(rdr.smp_hemisphere), "depth_samples": np.int32(rdr.depth_samples), "sample_extent": np.float32(rdr.sample_extent),
           "anti_alias": np.int32(bool(rdr.anti_alias)), "stratified": np.int32(bool(rdr.stratified_sample)),
           "do_crop": np.int32(bool(rdr.do_crop)), "window": np.int32([rdr.start_x, rdr.end_x, rdr.start_y, rdr.end_y]),
           "inv_cam_r": rdr.inv_cam_r.to_numpy().astype(np.float32), "cam_normal": rdr.cam_normal.to_numpy().astype(np.float32),
           "depth": rdr.color.to_numpy()[..., 2].copy(), "depth_draws": depth_draws}
    accum = np.zeros((spp, w, h, 3), np.float32)
    draws = np.zeros((spp, w, h), np.int32)
    for s in range(spp):
        state["draws"] = draws[s]
        rdr.render(0, 0, 0, 0, 0, 0)
        flush()
        accum[s] = rdr.color.to_numpy()
    ti.PIXEL_HOOK[0] = None
    out["accum"], out["draws"], out["pixels"] = accum, draws, rdr.pixels.to_numpy().astype(np.float32)
    np.savez_compressed(os.path.join(OUT, f"ao_{name}.npz"), **out)
    print(f"ao_{name}: {w}x{h}x{spp}spp, smp_hemisphere {int(out['smp_hemisphere'])}, depth_samples {int(out['depth_samples'])} in {time.time() - t0:.1f}s; "
          f"hit share {np.mean(out['depth'] > 0):.3f}, mean AO {out['pixels'].mean():.4f}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    os.chdir(refenv.REPO)                                       # texture paths in scenes/test/textured.xml are relative to the repository root
    for case in CASES:
        if a.only in (None, case):
            gen_case(case)
