#!/usr/bin/env python3
"""What the denoiser buys at low sample counts: relMSE of raw and denoised frames against a long render.

    python tools/denoise_quality.py [--size 512] [--ref-spp 4096] [--scenes cbox,glass_box,c3_balls_mono,textured] [--spp 4,16,64] [--grid] [--out FILE.jsonl]

Per scene: a render of --ref-spp samples with another seed is the reference (the one tools/adaptive_quality.py uses); a second renderer is
taken to 4, 16 and 64 spp and at each stop its raw `pixels` and `denoised()` are held against the reference (relMSE as tests/conftest.py
image_metrics defines it).  Without --grid one line per scene and stop, with the shipped defaults (adapt_amd.renderer.DENOISE_DEFAULTS);
with --grid also one line per setting of a small grid around them, which is how the defaults were chosen."""
import argparse
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = {"cbox": ("cbox", "c2_cbox.xml"), "glass_box": ("cbox", "glass_box.xml"), "c3_balls_mono": ("csphere", "c3_balls_mono.xml"),
          "textured": ("test", "textured.xml")}
GRID = {"sigma_c": [0.0, 0.3, 1.0, 3.0, 10.0], "iterations": [3, 4, 5], "sigma_z": [0.1, 1.0], "sigma_n": [32.0, 128.0], "sigma_a": [0.1, 0.3],
        "firefly_threshold": [0.0, 0.4]}


def rel_mse(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    a = np.where(np.isfinite(a), a, 0.0)
    return float(np.mean((a - b) ** 2 / (b ** 2 + 1e-2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--spp", default="4,16,64")
    ap.add_argument("--grid", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from adapt_amd.parsers import scene_parsing
    from adapt_amd.renderer import DENOISE_DEFAULTS, Renderer
    settings = [{}]
    if a.grid:
        keys = list(GRID)
        settings += [dict(zip(keys, v)) for v in itertools.product(*(GRID[k] for k in keys))]
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)
    for name in a.scenes.split(","):
        folder, fname = SCENES[name]
        os.chdir(ROOT)                               # texture paths are relative to the repository root
        sc = scene_parsing(os.path.join(ROOT, "scenes", folder), fname)
        kw = dict(width=a.size, height=a.size)
        ref_r = Renderer(*sc, seed=1, **kw)
        ref_r.render(n_spp=a.ref_spp)
        ref = ref_r.pixels.to_numpy(); ref_r.close()
        ref = np.where(np.isfinite(ref), ref, 0.0)
        r = Renderer(*sc, **kw)
        done = 0
        for spp in [int(s) for s in a.spp.split(",")]:
            r.render(n_spp=spp - done); done = spp
            raw = rel_mse(r.pixels.to_numpy(), ref)
            for cfg in settings:
                e = rel_mse(r.denoised(**cfg), ref)
                emit({"scene": name, "size": a.size, "spp": spp, "ref_spp": a.ref_spp, "settings": {**DENOISE_DEFAULTS, **cfg}, "shipped": not cfg,
                      "relMSE_raw": raw, "relMSE_denoised": e, "ratio": e / raw})
        r.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("".join(json.dumps(d) + "\n" for d in lines))


if __name__ == "__main__":
    main()
