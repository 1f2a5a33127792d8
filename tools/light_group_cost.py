#!/usr/bin/env python3
"""One timed render of scenes/test/features_b.xml (five emitters) at 512 x 512 x 256 spp, for the cost figures of DESIGN.md §4.9:

    python tools/light_group_cost.py lights | lengths | steady

Prints one JSON line: five host-clock times of render(256) + synchronize after two warm-up renders of the same shape, their median and
spread, the device time, and the pipeline that ran; `lights` adds five times of one relit() call.  The three modes launch the same kernels
but for the binning one; compare them by starting one process per mode in turn (profiles/r07_light_group_cost.jsonl)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(mode):
    import numpy as np
    from adapt_amd import scene_parsing
    from adapt_amd.renderer import Renderer
    parsed = scene_parsing(os.path.join(ROOT, "scenes", "test"), "features_b.xml")
    kw = {"lights": {"light_groups": True}, "lengths": {"path_lengths": True}, "steady": {}}[mode]
    r = Renderer(*parsed, width=512, height=512, **kw)
    for _ in range(2):
        r.render(n_spp=256); r.synchronize()
    ms = []
    for _ in range(5):
        r.clear(); r.synchronize()
        t0 = time.perf_counter(); r.render(n_spp=256); r.synchronize(); ms.append((time.perf_counter() - t0) * 1e3)
    info = r.info()
    out = {"mode": mode, "ms": ms, "median_ms": statistics.median(ms), "spread_ms": max(ms) - min(ms), "device_ms": r.stats()["render_ms"],
           "spp_per_batch": info["spp_per_batch"], "shade": info["shade_variant"], "traversal": info["traversal"], "max_bounce": r.max_bounce,
           "S": r.num_shadow_ray, "emitters": r.src_num}
    if mode == "lights":
        out["plane_bytes"] = int(r.tile_light_groups().nbytes)
        gains = np.linspace(0.5, 1.5, 3 * r.src_num, dtype=np.float32).reshape(-1, 3)
        rel = []
        for _ in range(5):
            t0 = time.perf_counter(); r.relit(gains); rel.append((time.perf_counter() - t0) * 1e3)
        out["relit_ms"] = rel
        out["n_stray_light"] = r.stats()["n_stray_light"]
    print(json.dumps(out))
    r.close()


if __name__ == "__main__":
    if len(sys.argv) != 2 or sys.argv[1] not in ("lights", "lengths", "steady"):
        sys.exit(__doc__)
    main(sys.argv[1])
