"""Occupancy guard for C1 / C2's queue-fed shade kernel with its record staged in LDS a row ahead (csrc/shade_stage.hpp
k_shade_traced_lean_staged): the compile probe of tests/test_kernel_registers.py for that instantiation.  It keeps the budget of
the kernel with the direct loads - seven waves per SIMD: at most 72 VGPRs, nothing spilled, no scratch - and its LDS (4 KiB per wave for the
staged record) must leave seven workgroups resident in a compute unit's 160 KiB."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

INST = "k_shade_traced_lean_staged<0x002, 0x01>(DevScene, Params, Queues, Counters*, int, int)"
PREFIX = "_Z26k_shade_traced_lean_stagedILi2ELi1EE"
VGPR_BUDGET, WAVES, CU_LDS_BYTES = 72, 7, 160 * 1024


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_staged_record_shade_kernel_keeps_seven_waves(tmp_path):
    src = tmp_path / "probe.hip"
    src.write_text("#include <hip/hip_runtime.h>\n#include <algorithm>\n#include <cmath>\n#include <cstdio>\n#include <cstdlib>\n#include <cstring>\n"
                   f'#include "{ROOT}/include/adapt_mi.h"\n#include "{ROOT}/adapt_amd/csrc/bvh_build.hpp"\n#include "{ROOT}/adapt_amd/csrc/shade_stage.hpp"\n'
                   f"template __global__ void {INST};\n")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-fast-math", "-mllvm", "-amdgpu-atomic-optimizer-strategy=None", "-fno-slp-vectorize", "-ffp-contract=off",
           "-DAPT_FAST=1", "-DAPT_EXACT_MATH=0", "-DAPT_FAST_DIV=1", "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", str(src), "-o", str(tmp_path / "probe.o")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    blocks = [blk for blk in out.stderr.split("Function Name: ")[1:] if blk.split("\n")[0].strip().startswith(PREFIX)]
    assert len(blocks) == 1, out.stderr[-2000:]

    def figure(pattern):
        m = re.search(pattern, blocks[0])
        assert m, (pattern, blocks[0])
        return int(m.group(1))

    vgprs, spilled, scratch = figure(r"VGPRs: (\d+)"), figure(r"VGPRs Spill: (\d+)"), figure(r"ScratchSize \[bytes/lane\]: (\d+)")
    waves, lds = figure(r"Occupancy \[waves/SIMD\]: (\d+)"), figure(r"LDS Size \[bytes/block\]: (\d+)")
    print(f"{INST}: {vgprs} VGPRs, {spilled} spilled, {scratch} B of scratch, {waves} waves per SIMD, {lds} B of LDS per workgroup")
    assert vgprs <= VGPR_BUDGET and spilled == 0 and scratch == 0, f"{vgprs} VGPRs, {spilled} spilled, {scratch} B of scratch; budget {VGPR_BUDGET}, no spill, no scratch"
    assert lds * WAVES <= CU_LDS_BYTES, f"{lds} B of LDS per workgroup: {WAVES} workgroups need {lds * WAVES} of {CU_LDS_BYTES} B"
