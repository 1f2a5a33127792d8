#!/usr/bin/env python3
"""What the ambient-occlusion renderer costs at 512 x 512 x 64 spp on the product build, for DESIGN.md §4.10 and profiles/NOTES.md:

    python tools/ao_cost.py [--scene cbox|bunnies] [--spp 64]

cbox is the Cornell box (flat sweep), bunnies is synth.three_bunnies() - the three subdivided bunnies in a box, the stand-in for the
reference's bunny scene (BVH walk).  Three things are timed apart, each five times on the host clock after two warm-up rounds, with a
synchronize inside the bracket:
  depth   creating the renderer: scene upload, queues and the depth pass (depth_samples camera rays per pixel) - and, for comparison, the
          same creation with depth_samples = 0, which has everything but the depth pass
  render  render(spp) of the AO renderer
  floor   apt_render_aov of a path tracer over the same sample numbers: the same camera rays and closest hits without the hemisphere loop
Prints one JSON line: the times, their medians and spreads, Msamples/s of the render and of the floor, the kernels' share of the render
(launch-bracketing events, a second renderer with profile=True) and the pipeline that ran.  One process per scene; compare scenes or
settings by starting the processes in turn, several rounds."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, rounds=5, warm=2):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(rounds):
        t0 = time.perf_counter(); fn(); ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def main(scene, spp):
    from adapt_amd import scene_parsing
    from adapt_amd.renderer import AORenderer, Renderer
    from adapt_amd.synth import three_bunnies
    parsed = three_bunnies() if scene == "bunnies" else scene_parsing(os.path.join(ROOT, "scenes", "cbox"), "c2_cbox.xml")
    film = {"width": 512, "height": 512}
    n = film["width"] * film["height"] * spp

    def create(cls, **kw):
        r = cls(*parsed, **film, **kw); r.synchronize(); r.close()
    create_ao, create_no_depth = timed(lambda: create(AORenderer)), timed(lambda: create(AORenderer, depth_samples=0))

    ao = AORenderer(*parsed, **film)

    def render():
        ao.clear(); ao.render(n_spp=spp); ao.synchronize()
    render_ms = timed(render)
    info = ao.info()
    ao.close()

    pt = Renderer(*parsed, **film, aov_spp=spp)
    pt._cnt = spp                                   # (the pass restates the rays of samples 1..spp; nothing needs to be rendered for that)

    def floor():
        pt._clear_aov(); pt.tile_aov()
    floor_ms = timed(floor)
    pt.close()

    prof = AORenderer(*parsed, **film, profile=True)
    prof.render(n_spp=spp); prof.synchronize()
    st = prof.stats()
    prof.close()
    med = statistics.median
    out = {"scene": scene, "spp": spp, "film": [film["width"], film["height"]], "traversal": info["traversal"], "spp_per_batch": info["spp_per_batch"], "ao": info["ao"],
           "create_ao_ms": create_ao, "create_no_depth_ms": create_no_depth, "depth_pass_ms": med(create_ao) - med(create_no_depth),
           "render_ms": render_ms, "render_median_ms": med(render_ms), "render_spread_ms": max(render_ms) - min(render_ms), "render_msamples_s": n / med(render_ms) / 1e3,
           "floor_ms": floor_ms, "floor_median_ms": med(floor_ms), "floor_msamples_s": n / med(floor_ms) / 1e3,
           "kernel_ms": st["kernel_ms"], "device_ms": st["render_ms"], "kernel_share": sum(st["kernel_ms"].values()) / max(st["render_ms"], 1e-9)}
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(usage=__doc__)
    ap.add_argument("--scene", default="cbox", choices=["cbox", "bunnies"])
    ap.add_argument("--spp", type=int, default=64)
    a = ap.parse_args()
    main(a.scene, a.spp)
