"""Static guard for the live-row form of C1 / C2's two shade kernels (csrc/shade_stage.hpp shade_traced LIVE: k_shade_traced_lean_staged_live,
k_shade_traced_lean_cam_live): the compile probe of tests/test_kernel_registers_record_stage.py - its command line plus -S -
for the two instantiations.  Each keeps the parent kernel's budget (seven waves per SIMD: at most 72 VGPRs, nothing spilled, no scratch, the
parent's LDS), and its row loop - the largest span of the kernel's assembly that a backward branch closes - issues fewer vector instructions
than the parent's: the form exists to take the dead lanes' default writes (v_mov_b32 of 0 / 1.0 / -1, phi copies) out of that loop.

Counts, VALU / v_mov_b32 per row loop, by loop_counts() below:
    queue-fed   parent 1 591 / 204 (k_shade_traced_lean_staged)   live rows 1 502 / 121
    camera-fed  parent 2 332 / 263 (k_shade_traced_lean_cam)      live rows 2 262 / 206
The bounds are the live rows' counts plus a margin of 10 (compiler point releases move a few instructions); the queue-fed loop must also
stay at least 50 VALU below the parent's 1 591."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

VGPR_BUDGET, MARGIN = 72, 10
PARENT_STAGED_VALU = 1591
# instantiation, mangled prefix, LDS bytes per workgroup (the parent kernel's), VALU and v_mov_b32 of the row loop as built
KERNELS = {
    "staged": ("k_shade_traced_lean_staged_live<0x002, 0x01>(DevScene, Params, Queues, Counters*, int, int)", "_Z31k_shade_traced_lean_staged_liveILi2ELi1EE", 19472, 1502, 121),
    "cam": ("k_shade_traced_lean_cam_live<0x002, 0x01>(DevScene, Params, Queues, Counters*, const unsigned long long*)", "_Z28k_shade_traced_lean_cam_liveILi2ELi1EE", 16, 2262, 206),
}


def loop_counts(asm, prefix):
    """VALU instructions and v_mov_b32 among them in the largest back-edge span of the function whose symbol starts with `prefix`:
    the instructions from a label to the farthest branch behind it that jumps back to it -> (instructions, valu, v_mov)"""
    lines = asm.split("\n")
    start = next(i for i, ln in enumerate(lines) if re.match(re.escape(prefix) + r"\w*:", ln))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
    ins, labels = [], {}
    for ln in lines[start + 1:end + 1]:
        text = ln.split(";")[0].strip()
        m = re.match(r"^([.\w$]+):$", text)
        if m: labels[m.group(1)] = len(ins)
        elif text and not text.startswith("."): ins.append(text)
    first, last = 0, -1
    for i, text in enumerate(ins):
        m = re.match(r"s_c?branch\w*\s+(\S+)$", text)
        if m and labels.get(m.group(1), i + 1) <= i and i - labels[m.group(1)] > last - first: first, last = labels[m.group(1)], i
    ops = [text.split()[0] for text in ins[first:last + 1]]
    return len(ops), sum(o.startswith("v_") for o in ops), sum(o.startswith("v_mov_b32") for o in ops)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """both instantiations compiled once -> (the compiler's resource remarks, the assembly)"""
    if not os.path.exists(HIPCC): pytest.skip("hipcc not found")
    tmp = tmp_path_factory.mktemp("live_rows")
    src = tmp / "probe.hip"
    src.write_text("#include <hip/hip_runtime.h>\n#include <algorithm>\n#include <cmath>\n#include <cstdio>\n#include <cstdlib>\n#include <cstring>\n"
                   f'#include "{ROOT}/include/adapt_mi.h"\n#include "{ROOT}/adapt_amd/csrc/bvh_build.hpp"\n#include "{ROOT}/adapt_amd/csrc/shade_stage.hpp"\n'
                   + "".join(f"template __global__ void {inst};\n" for inst, *_ in KERNELS.values()))
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-fast-math", "-mllvm", "-amdgpu-atomic-optimizer-strategy=None", "-fno-slp-vectorize", "-ffp-contract=off",
           "-DAPT_FAST=1", "-DAPT_EXACT_MATH=0", "-DAPT_FAST_DIV=1", "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-S", str(src), "-o", str(tmp / "probe.s")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stderr, (tmp / "probe.s").read_text()


@pytest.mark.parametrize("which", sorted(KERNELS))
def test_live_row_kernel_keeps_the_parents_budget(probe, which):
    inst, prefix, lds_parent, _, _ = KERNELS[which]
    blocks = [blk for blk in probe[0].split("Function Name: ")[1:] if blk.split("\n")[0].strip().startswith(prefix)]
    assert len(blocks) == 1, probe[0][-2000:]

    def figure(pattern):
        m = re.search(pattern, blocks[0])
        assert m, (pattern, blocks[0])
        return int(m.group(1))

    vgprs, spilled, scratch = figure(r"VGPRs: (\d+)"), figure(r"VGPRs Spill: (\d+)"), figure(r"ScratchSize \[bytes/lane\]: (\d+)")
    lds = figure(r"LDS Size \[bytes/block\]: (\d+)")
    print(f"{inst}: {vgprs} VGPRs, {spilled} spilled, {scratch} B of scratch, {lds} B of LDS per workgroup")
    assert vgprs <= VGPR_BUDGET and spilled == 0 and scratch == 0, f"{vgprs} VGPRs, {spilled} spilled, {scratch} B of scratch; budget {VGPR_BUDGET}, no spill, no scratch"
    assert lds == lds_parent, f"{lds} B of LDS per workgroup, the parent kernel has {lds_parent}"


@pytest.mark.parametrize("which", sorted(KERNELS))
def test_live_row_loop_issues_fewer_vector_instructions(probe, which):
    inst, prefix, _, valu_built, vmov_built = KERNELS[which]
    n, valu, vmov = loop_counts(probe[1], prefix)
    print(f"{inst}: row loop of {n} instructions, {valu} VALU, {vmov} v_mov_b32")
    assert n > 1000, f"no row loop found: the largest back-edge span holds {n} instructions"
    assert valu <= valu_built + MARGIN and vmov <= vmov_built + MARGIN, f"{valu} VALU / {vmov} v_mov_b32; built at {valu_built} / {vmov_built}, margin {MARGIN}"
    if which == "staged": assert valu <= PARENT_STAGED_VALU - 50, f"{valu} VALU: less than 50 below the parent's {PARENT_STAGED_VALU}"
