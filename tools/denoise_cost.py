#!/usr/bin/env python3
"""What the feature-buffer pass and the denoiser cost, beside the render they accompany.

    python tools/denoise_cost.py [--sizes 512,2048] [--spp 32] [--rounds 5] [--scene cbox] [--out FILE.jsonl]

Per film size, on one renderer, `rounds` rounds of: 32 spp of the ordinary render | the AOV pass for the same 32 samples | one denoised()
call with the shipped defaults - alternating, each timed by the host clock around work that ends in a device synchronise (the denoiser's
figure includes its copy of the frame back to the host); medians and the spread (min .. max) are printed.  A second renderer with
APT_CAMERA_FUSE=0 and profile=True gives the HIP-event time of the render's own camera-ray kernel (generate, which in the product build
also traces the camera ray) for the same 32 samples: the work the AOV pass restates.  Under `rocprofv3 --kernel-trace --stats` the same
run yields the per-kernel times (k_aov_trace*, k_aov_sum, k_dn_*)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCENES = {"cbox": ("cbox", "c2_cbox.xml"), "c3_balls_mono": ("csphere", "c3_balls_mono.xml"), "textured": ("test", "textured.xml")}


def clock(fn, sync):
    sync()
    t = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t) * 1e3


def spread(v):
    return {"median_ms": round(float(np.median(v)), 3), "min_ms": round(float(np.min(v)), 3), "max_ms": round(float(np.max(v)), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,2048")
    ap.add_argument("--spp", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scene", default="cbox")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from adapt_amd.parsers import scene_parsing
    from adapt_amd.renderer import Renderer
    os.chdir(ROOT)
    sc = scene_parsing(os.path.join(ROOT, "scenes", SCENES[a.scene][0]), SCENES[a.scene][1])
    lines = []
    for size in [int(s) for s in a.sizes.split(",")]:
        r = Renderer(*sc, width=size, height=size, aov_spp=a.spp)
        r.render(n_spp=a.spp); r.aov(); r.denoised()            # warm-up: first launches, buffers allocated
        t_render, t_aov, t_dn = [], [], []
        for _ in range(a.rounds):
            r.clear()
            t_render.append(clock(lambda: r.render(n_spp=a.spp), r.synchronize))
            t_aov.append(clock(r._update_aov, r.synchronize))
            t_dn.append(clock(r.denoised, r.synchronize))
        info = r.info()
        r.close()
        os.environ["APT_CAMERA_FUSE"] = "0"
        p = Renderer(*sc, width=size, height=size, profile=True)
        del os.environ["APT_CAMERA_FUSE"]
        p.render(n_spp=a.spp); p.synchronize(); p.clear()
        p.render(n_spp=a.spp); p.synchronize()
        st = p.stats()
        p.close()
        d = {"scene": a.scene, "size": size, "spp": a.spp, "rounds": a.rounds, "traversal": info["traversal"], "arithmetic": info["arithmetic"],
             "render": spread(t_render), "aov_pass": spread(t_aov), "denoised_call": spread(t_dn),
             "render_kernel_ms_unfused": {k: round(v, 3) for k, v in st["kernel_ms"].items()}, "render_launches_unfused": st["launches"]}
        lines.append(d)
        print(json.dumps(d), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("".join(json.dumps(d) + "\n" for d in lines))


if __name__ == "__main__":
    main()
