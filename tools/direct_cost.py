#!/usr/bin/env python3
"""What the direct-light viewer costs at 512 x 512 on the product build, for DESIGN.md §4.11 and profiles/NOTES.md:

    python tools/direct_cost.py [--scene cbox|bunnies] [--frames 64]

cbox is the Cornell box (flat sweep), bunnies is synth.three_bunnies() - the three subdivided bunnies in a box, the 95 k-triangle stand-in
for the reference's bunny scene (BVH walk).  Four things are timed apart, each five times on the host clock after two warm-up rounds; every
call of the viewer returns after its stream has drained, so the bracket needs no synchronize of its own:
  create    making the viewer: scene upload, queues and the hit pass (the hit pass is not timed apart: a path tracer made the same way
            builds camera strips and light masks the viewer does not, so the difference of the two says nothing)
  render    one render(emit_pos): upload of the position, the shade launch, the wait
  sweep     render_sweep of `frames` positions: one launch (or a few), the frames copied back into a NEW host array - and the same into
            an array handed in (out=), whose pages have been touched before
  singles   `frames` calls of render, nothing read back - and the same with `pixels` read after each, which is what a caller who wants the
            frames has to do
The light moves along a line below the ceiling.  Prints one JSON line: the times, their medians and ranges, the kernel time of one render
and of the sweep (launch-bracketing events, a second viewer with profile=True) and the traversal that ran.  One process per scene; compare
scenes by starting the processes in turn, several rounds."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, rounds=5, warm=2):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(rounds):
        t0 = time.perf_counter(); fn(); ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def point_light(scene):
    """the scene's first point emitter, or one made for it (the bunny scene is lit by spot lights)"""
    for e in scene[0]:
        if e.type == "point":
            return e
    import xml.etree.ElementTree as xet
    from adapt_amd.emitters import PointSource
    return PointSource(xet.fromstring('<emitter type="point" id="viewer"><rgb name="emission" value="12.0"/><point name="center" x="2.78" y="4.5" z="3.0"/></emitter>'))


def main(scene, frames):
    from adapt_amd import scene_parsing
    from adapt_amd.renderer import BlinnPhongTracer
    from adapt_amd.synth import three_bunnies
    parsed = three_bunnies() if scene == "bunnies" else scene_parsing(os.path.join(ROOT, "scenes", "cbox"), "c2_cbox.xml")
    em, arr, objs, prop = parsed
    prop = dict(prop); prop["film"] = dict(prop["film"], width=512, height=512)
    light = point_light(parsed)
    positions = np.float32([[0.8 + 4.0 * k / max(1, frames - 1), 4.5, 2.0 + 1.5 * k / max(1, frames - 1)] for k in range(frames)])

    def create_viewer():
        v = BlinnPhongTracer(light, arr, objs, prop); v.synchronize(); v.close()
    create_ms = timed(create_viewer)

    v = BlinnPhongTracer(light, arr, objs, prop)
    info = v.info()
    render_ms = timed(lambda: v.render(positions[0]))
    sweep_ms = timed(lambda: v.render_sweep(positions))
    held = np.empty((frames, 512, 512, 3), np.float32)
    sweep_reuse_ms = timed(lambda: v.render_sweep(positions, out=held))

    def singles():
        for e in positions:
            v.render(e)

    def singles_read():
        for e in positions:
            v.render(e); v.pixels.to_numpy()
    singles_ms, singles_read_ms = timed(singles), timed(singles_read)
    v.close()

    prof = BlinnPhongTracer(light, arr, objs, prop, profile=True)
    prof.render(positions[0]); one = sum(prof.stats()["kernel_ms"].values())
    prof.render_sweep(positions); both = sum(prof.stats()["kernel_ms"].values())
    kernel = {"one_render_ms": one, "sweep_ms": both - one}
    prof.close()
    med = statistics.median
    rng = lambda ms: [min(ms), max(ms)]
    out = {"scene": scene, "frames": frames, "film": [512, 512], "traversal": info["traversal"], "primitives": int(arr["primitives"].shape[0]),
           "create_ms": create_ms, "create_median_ms": med(create_ms), "create_range_ms": rng(create_ms),
           "render_ms": render_ms, "render_median_ms": med(render_ms), "render_range_ms": rng(render_ms),
           "sweep_ms": sweep_ms, "sweep_median_ms": med(sweep_ms), "sweep_range_ms": rng(sweep_ms), "sweep_per_frame_ms": med(sweep_ms) / frames,
           "sweep_reuse_ms": sweep_reuse_ms, "sweep_reuse_median_ms": med(sweep_reuse_ms), "sweep_reuse_range_ms": rng(sweep_reuse_ms), "sweep_reuse_per_frame_ms": med(sweep_reuse_ms) / frames,
           "singles_ms": singles_ms, "singles_median_ms": med(singles_ms), "singles_range_ms": rng(singles_ms), "singles_per_frame_ms": med(singles_ms) / frames,
           "singles_read_ms": singles_read_ms, "singles_read_median_ms": med(singles_read_ms), "singles_read_per_frame_ms": med(singles_read_ms) / frames,
           "kernel": kernel}
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(usage=__doc__)
    ap.add_argument("--scene", default="cbox", choices=["cbox", "bunnies"])
    ap.add_argument("--frames", type=int, default=64)
    a = ap.parse_args()
    main(a.scene, a.frames)
