#!/usr/bin/env python3
"""Time to quality of adaptive sampling against uniform sampling, and the cost of a round at low active fractions.

    python tools/adaptive_quality.py [--size 512] [--ref-spp 4096] [--scenes glass_box,c3,cbox_fog] [--out FILE.jsonl]

Per scene: a uniform render of --ref-spp samples with another seed is the reference; uniform renders of 16 .. 1024 spp and adaptive renders
(min_spp 64, step 32, at most 1024 spp) at several thresholds are held against it (relMSE as tests/conftest.py image_metrics defines it).
Times are the HIP-event time of the render calls (stats()["render_ms"]).  For every adaptive point the uniform time that reaches the same
relMSE is read off the uniform curve (log-log interpolation) and the ratio printed.  Then one round (step samples) is timed with
~100 %, 10 % and 1 % of the pixels active (a random mask set through the checkpoint entry point, threshold tiny: nothing retires)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = {"glass_box": ("cbox", "glass_box.xml", False), "c3": ("csphere", "c3_balls_mono.xml", False), "cbox_fog": ("vpt", "cbox_fog.xml", True)}
UNIFORM_SPP = [16, 32, 64, 128, 256, 512, 1024]
THRESHOLDS = [0.2, 0.1, 0.05, 0.03, 0.02, 0.01]
MIN_SPP, STEP, MAX_SPP = 64, 32, 1024


def rel_mse(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.mean((a - b) ** 2 / (b ** 2 + 1e-2)))


def timed(rdr, n):
    before = rdr.stats()["render_ms"]
    rdr.render(n_spp=n)
    rdr.synchronize()
    return rdr.stats()["render_ms"] - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--scenes", default="glass_box,c3,cbox_fog")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from adapt_amd.parsers import scene_parsing
    from adapt_amd.renderer import Renderer, VolumeRenderer
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)
    for name in a.scenes.split(","):
        folder, fname, vol = SCENES[name]
        os.chdir(ROOT)
        sc = scene_parsing(os.path.join(ROOT, "scenes", folder), fname)
        cls = VolumeRenderer if vol else Renderer
        kw = dict(width=a.size, height=a.size)
        ref_r = cls(*sc, seed=1, **kw)
        timed(ref_r, a.ref_spp)
        ref = ref_r.pixels.to_numpy(); ref_r.close()
        uni = []
        r = cls(*sc, **kw)
        timed(r, 8)                                  # warm-up (first launches), then from a cleared film
        r.clear()
        t, done = 0.0, 0
        for spp in UNIFORM_SPP:
            t += timed(r, spp - done); done = spp
            uni.append((spp, t, rel_mse(r.pixels.to_numpy(), ref)))
            emit({"scene": name, "mode": "uniform", "spp": spp, "ms": round(t, 3), "relMSE": uni[-1][2]})
        r.close()
        ut, ue = np.log([u[1] for u in uni]), np.log([u[2] for u in uni])
        for thr in THRESHOLDS:
            r = cls(*sc, adaptive={"threshold": thr, "min_spp": MIN_SPP, "step": STEP}, **kw)
            t = timed(r, MAX_SPP)
            e = rel_mse(r.pixels.to_numpy(), ref)
            n = r.sample_counts()
            order = np.argsort(ue)                   # uniform time that reaches relMSE e (relMSE falls with time)
            t_uni = float(np.exp(np.interp(np.log(e), ue[order], ut[order]))) if ue.min() <= np.log(e) <= ue.max() else float("nan")
            emit({"scene": name, "mode": "adaptive", "threshold": thr, "ms": round(t, 3), "relMSE": e, "mean_spp": float(n.mean()),
                  "retired": float(1.0 - r.active_fraction()), "uniform_ms_same_relMSE": round(t_uni, 3), "speedup": round(t_uni / t, 3) if t_uni == t_uni else None})
            r.close()
        # the cost of one round with a given share of the pixels active
        r = cls(*sc, adaptive={"threshold": 1e-30, "min_spp": MIN_SPP, "step": STEP}, **kw)
        timed(r, MIN_SPP)
        rs = np.random.RandomState(0)
        for frac in (1.0, 0.1, 0.01):
            n, _ = r.tile_sample_counts(with_mask=True)
            act = rs.uniform(size=n.shape) < frac if frac < 1.0 else np.ones(n.shape, bool)
            ck = r.get_check_point()
            ck["active"] = act
            r.load_check_point(ck)
            ms = [timed(r, STEP) for _ in range(3)]
            emit({"scene": name, "mode": "round", "active": float(act.mean()), "step": STEP, "ms_per_round": round(float(np.median(ms)), 3)})
        r.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("".join(json.dumps(d) + "\n" for d in lines))


if __name__ == "__main__":
    main()
