"""The draw window of the traced kernels without area lights (csrc/rng.hpp DrawWindow) on the device: a library built with
-DAPT_DRAW_WINDOW=0 - the generator every other kernel keeps: both Philox blocks up front, a general draw at every site - and the
default build render the same accumulation, compared as uint32, and the same counters.  The test builds the variant library itself
(a variant that does not build is a failure) and renders with each library in a child process (ADAPT_MI_LIB is read when adapt_amd is
imported): every bundled scene that takes the lean traced kernels, C1, a film whose pixel count is no multiple of 64, one bounce, no
anti-aliasing (no jitter pass in front of the camera vertex), every ray through the reference-order code, the two-launch camera
vertex, roulette draws from bounce 0 on (at every offset of a block) and at every vertex, and two point lights (the emitter index is
used, and drawn from the window)."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import json, os, sys
import numpy as np
root, out = sys.argv[1], sys.argv[2]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import conftest
import gpu_ab
from adapt_amd import materials
from adapt_amd.parsers import scene_parsing

def parse(tag):
    d, f, _ = conftest.SCENES[tag]
    os.chdir(root); materials.ENABLE_MICROFACET = tag in conftest.MICROFACET_TAGS
    try: return scene_parsing(d, f)
    finally: materials.ENABLE_MICROFACET = False

results, accums = {}, {}
def case(key, tup, w, h, spp, max_bounce=None, cfg=None, env=None, lights=1):
    emitters, arrays, objects, prop = tup
    if cfg: prop = dict(prop, **cfg)
    with gpu_ab.open_renderer((list(emitters) * lights, arrays, objects, prop), w, h, env=env, max_bounce=max_bounce) as r:
        name = r.info()["shade_variant"]                # only the lean traced variant is rendered
        run = gpu_ab.run_of(r, spp) if "lambertian/point" in name and gpu_ab.TRACED in name else None
    results[key] = {"variant": name, "fused": run and bool(run.fused), "counters": run and {k: int(run.stats[k]) for k in gpu_ab.COUNTERS}}
    if run: accums[key] = run.accum.view(np.uint32)

for tag in conftest.ALL_TAGS: case("scene_" + tag, parse(tag), 64, 64, 8)
cbox = parse("cbox")
case("c1", cbox, 256, 256, 16, max_bounce=4)
case("odd_50x30", cbox, 50, 30, 24)
case("one_bounce", cbox, 64, 64, 16, max_bounce=1)
case("no_anti_alias", cbox, 64, 64, 16, cfg={"anti_alias": False})
case("defer_all", cbox, 64, 48, 12, env={"APT_FLAT_DEFER_ALL": "1"})
case("camera_fuse_0", cbox, 64, 64, 16, env={"APT_CAMERA_FUSE": "0"})
case("rr_from_bounce_0", cbox, 64, 64, 32, cfg={"rr_bounce_th": 0})
case("rr_from_bounce_0_no_anti_alias", cbox, 64, 64, 32, cfg={"rr_bounce_th": 0, "anti_alias": False})
case("rr_at_every_vertex", cbox, 64, 64, 32, cfg={"rr_bounce_th": 0, "rr_threshold": 2.0})
case("rr_at_every_vertex_no_anti_alias", cbox, 64, 64, 32, cfg={"rr_bounce_th": 0, "rr_threshold": 2.0, "anti_alias": False})
case("two_lights", cbox, 64, 64, 16, lights=2)
np.savez(out + ".npz", **accums)
json.dump(results, open(out + ".json", "w"))
"""


def _build_variant(dst, flag):
    from adapt_amd import build as b
    cmd = [b.hipcc(), *b.FLAGS, *b.VARIANT_FLAGS["fast"], flag, *[os.path.join(b.CSRC, s) for s in b.SOURCES], "-o", dst]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=1800)
    assert out.returncode == 0 and os.path.exists(dst), f"the {flag} library does not build:\n{out.stderr[-3000:]}"


def _child(script, out, lib):
    env = dict(os.environ)
    env.pop("ADAPT_MI_LIB", None)
    if lib: env["ADAPT_MI_LIB"] = lib
    run = subprocess.run([sys.executable, script, ROOT, out], capture_output=True, text=True, timeout=1500, env=env)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    return json.load(open(out + ".json")), np.load(out + ".npz")


def test_draw_window_leaves_every_lean_traced_render_bit_identical(tmp_path):
    assert shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"), "hipcc is needed to build the APT_DRAW_WINDOW=0 library"
    lib0 = str(tmp_path / "libadapt_mi_window0.so")
    _build_variant(lib0, "-DAPT_DRAW_WINDOW=0")
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    res1, acc1 = _child(str(script), str(tmp_path / "window1"), None)
    res0, acc0 = _child(str(script), str(tmp_path / "window0"), lib0)
    assert sorted(res0) == sorted(res1)
    compared = []
    for key in sorted(res1):
        a, b = res1[key], res0[key]
        assert a["variant"] == b["variant"], key
        if a["counters"] is None:                       # the scene does not take the lean traced kernels
            assert key.startswith("scene_"), (key, a["variant"])
            continue
        assert a["fused"] == b["fused"], key
        print(key, a["variant"], a["counters"])
        assert a["counters"] == b["counters"], (key, a["counters"], b["counters"])
        assert a["counters"]["n_draws"] > 0 and a["counters"]["n_shade"] > 0, key
        x, y = acc1[key], acc0[key]
        assert x.dtype == np.uint32 and x.shape == y.shape and np.array_equal(x, y), (key, int(np.count_nonzero(x != y)))
        compared.append(key)
    for key in ("scene_cbox", "c1", "odd_50x30", "one_bounce", "no_anti_alias", "defer_all", "camera_fuse_0", "rr_from_bounce_0",
                "rr_from_bounce_0_no_anti_alias", "rr_at_every_vertex", "rr_at_every_vertex_no_anti_alias", "two_lights"):
        assert key in compared, (key, compared)
    assert res1["camera_fuse_0"]["fused"] is False and res1["c1"]["fused"] is True
    # the roulette cases draw more than the plain render's jitter + three per vertex would
    assert res1["rr_at_every_vertex"]["counters"]["n_draws"] != res1["rr_from_bounce_0"]["counters"]["n_draws"]
