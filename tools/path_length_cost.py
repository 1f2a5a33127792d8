#!/usr/bin/env python3
"""One timed render of the Cornell box at 512 x 512 x 256 spp, for the cost figures of DESIGN.md §4.8:

    python tools/path_length_cost.py lengths | transient | steady        (steady: run with APT_FUSED=0 for the staged pipeline)

Prints one JSON line: three host-clock times of render(256) + synchronize after two warm-up renders of the same shape, the device
time of the three, and the pipeline that ran.  Compare modes by starting one process per mode in turn, several rounds, and taking the
median of the per-process medians (profiles/r07_path_length_cost.jsonl)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(mode):
    from adapt_amd import scene_parsing
    from adapt_amd.renderer import Renderer
    name = "transient_cbox.xml" if mode == "transient" else "c2_cbox.xml"      # the same scene; the former's sensor has the 400 bins
    parsed = scene_parsing(os.path.join(ROOT, "scenes", "cbox"), name)
    kw = {"lengths": {"path_lengths": True}, "transient": {"transient": True}, "steady": {}}[mode]
    r = Renderer(*parsed, width=512, height=512, **kw)
    for _ in range(2):
        r.render(n_spp=256); r.synchronize()
    ms = []
    for _ in range(3):
        r.clear(); r.synchronize()
        t0 = time.perf_counter(); r.render(n_spp=256); r.synchronize(); ms.append((time.perf_counter() - t0) * 1e3)
    info = r.info()
    out = {"mode": mode, "ms": ms, "device_ms": r.stats()["render_ms"], "spp_per_batch": info["spp_per_batch"], "shade": info["shade_variant"],
           "traversal": info["traversal"], "max_bounce": r.max_bounce, "S": r.num_shadow_ray, "n_bins": r.n_bins}
    if mode == "lengths":
        out["plane_bytes"] = int(r.tile_path_lengths().nbytes)
    print(json.dumps(out))
    r.close()


if __name__ == "__main__":
    if len(sys.argv) != 2 or sys.argv[1] not in ("lengths", "transient", "steady"):
        sys.exit(__doc__)
    main(sys.argv[1])
