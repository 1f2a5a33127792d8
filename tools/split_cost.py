#!/usr/bin/env python3
"""One timed render at 512 x 512 x 256 spp in one split mode, for the cost figures of DESIGN.md §4.5, §4.8 and §4.9:

    python tools/split_cost.py steady | transient | lengths | lights [--scene cbox|features_b]

cbox is the Cornell box (the default; `transient` renders scenes/cbox/transient_cbox.xml, the same scene with the 400 bins in its sensor,
and takes no other scene), features_b is scenes/test/features_b.xml with its five emitters (the default of `lights`).  Prints one JSON line:
five host-clock times of render(256) + synchronize after two warm-up renders of the same shape, their median and spread, the device time,
and the pipeline that ran; `lights` adds five times of one relit() call.  The modes launch the same kernels but for the binning one
(steady: run with APT_FUSED=0 for the staged pipeline); compare them by starting one process per mode in turn, several rounds
(profiles/r07_path_length_cost.jsonl, profiles/r07_light_group_cost.jsonl)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = {"steady": {}, "transient": {"transient": True}, "lengths": {"path_lengths": True}, "lights": {"light_groups": True}}


def main(mode, scene):
    import numpy as np
    from adapt_amd import scene_parsing
    from adapt_amd.renderer import Renderer
    if scene == "features_b":
        parsed = scene_parsing(os.path.join(ROOT, "scenes", "test"), "features_b.xml")
    else:
        parsed = scene_parsing(os.path.join(ROOT, "scenes", "cbox"), "transient_cbox.xml" if mode == "transient" else "c2_cbox.xml")
    r = Renderer(*parsed, width=512, height=512, **MODES[mode])
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
    if mode != "steady":
        tile = {"transient": r.tile_transient, "lengths": r.tile_path_lengths, "lights": r.tile_light_groups}[mode]
        out["plane_bytes"] = int(tile().nbytes)
    if mode == "lights":
        gains = np.linspace(0.5, 1.5, 3 * r.src_num, dtype=np.float32).reshape(-1, 3)
        rel = []
        for _ in range(5):
            t0 = time.perf_counter(); r.relit(gains); rel.append((time.perf_counter() - t0) * 1e3)
        out["relit_ms"] = rel
        out["n_stray_light"] = r.stats()["n_stray_light"]
    print(json.dumps(out))
    r.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(usage=__doc__)
    ap.add_argument("mode", choices=list(MODES))
    ap.add_argument("--scene", choices=["cbox", "features_b"], default=None)
    a = ap.parse_args()
    if a.mode == "transient" and a.scene == "features_b":
        ap.error("transient: only cbox has a scene file with time bins in its sensor")
    main(a.mode, a.scene or ("features_b" if a.mode == "lights" else "cbox"))
