"""Occupancy guard for the camera-fed twin of C1 / C2's shade kernel (csrc/shade_stage.hpp k_shade_traced_lean_cam): the
compile probe of tests/test_kernel_registers.py for the instantiation that makes its camera rays itself.  It ships at the budget of the
queue-fed kernel - seven waves per SIMD: at most 72 VGPRs, nothing spilled, no scratch - and the queue-fed kernel, compiled next to it, must
keep the figures it had before the twin existed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# (explicit instantiation, mangled-name prefix, VGPR budget, why)
KERNELS = [
    ("k_shade_traced_lean_cam<0x002, 0x01>(DevScene, Params, Queues, Counters*, const unsigned long long*)", "_Z23k_shade_traced_lean_camILi2ELi1EE", 72,
     "C1 / C2: camera vertex shaded where the camera ray is traced, seven waves per SIMD"),
    ("k_shade_traced_lean<0x002, 0x01>(DevScene, Params, Queues, Counters*, int, int)", "_Z19k_shade_traced_leanILi2ELi1EE", 72,
     "C1 / C2: rays traced in place, seven waves per SIMD (unchanged by the twin)"),
]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_camera_fed_shade_kernel_keeps_seven_waves(tmp_path):
    src = tmp_path / "probe.hip"
    src.write_text("#include <hip/hip_runtime.h>\n#include <algorithm>\n#include <cmath>\n#include <cstdio>\n#include <cstdlib>\n#include <cstring>\n"
                   f'#include "{ROOT}/include/adapt_mi.h"\n#include "{ROOT}/adapt_amd/csrc/bvh_build.hpp"\n#include "{ROOT}/adapt_amd/csrc/shade_stage.hpp"\n'
                   + "".join(f"template __global__ void {inst};\n" for inst, *_ in KERNELS))
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-fast-math", "-mllvm", "-amdgpu-atomic-optimizer-strategy=None", "-fno-slp-vectorize", "-ffp-contract=off",
           "-DAPT_FAST=1", "-DAPT_EXACT_MATH=0", "-DAPT_FAST_DIV=1", "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", str(src), "-o", str(tmp_path / "probe.o")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    usage = {}
    for blk in out.stderr.split("Function Name: ")[1:]:
        name = blk.split("\n")[0].split(" [")[0].strip()
        v = re.search(r"VGPRs: (\d+)", blk); s = re.search(r"VGPRs Spill: (\d+)", blk); sc = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk); oc = re.search(r"Occupancy \[waves/SIMD\]: (\d+)", blk)
        usage[name] = (int(v.group(1)), int(s.group(1)) if s else 0, int(sc.group(1)) if sc else 0, int(oc.group(1)) if oc else 0)
    for inst, prefix, budget, why in KERNELS:
        hit = [(n, u) for n, u in usage.items() if n.startswith(prefix)]
        assert len(hit) == 1, (prefix, sorted(usage))
        vgprs, spilled, scratch, waves = hit[0][1]
        print(f"{inst}: {vgprs} VGPRs, {spilled} spilled, {scratch} B of scratch, {waves} waves per SIMD")
        assert vgprs <= budget and spilled == 0 and scratch == 0 and waves >= 7, f"{inst}: {vgprs} VGPRs, {spilled} spilled, {scratch} B of scratch, {waves} waves; budget {budget} ({why})"
