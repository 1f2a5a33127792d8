"""The compile probe of the kernel guards (test_kernel_registers*.py, test_kernel_live_rows.py): explicit instantiations of the stage headers'
kernels compiled for gfx950 with the product build's own flags (adapt_amd/build.py: FLAGS without the link / PIC / visibility / warning flags,
plus VARIANT_FLAGS["fast"]) and -Rpass-analysis=kernel-resource-usage; hipcc cross-compiles without a GPU.  One probe per set of
instantiations and session: files that ask for the same kernels share the compile."""
import os
import re
import subprocess
import tempfile

import pytest

from adapt_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHADE_HEADERS = ("include/adapt_mi.h", "adapt_amd/csrc/bvh_build.hpp", "adapt_amd/csrc/shade_stage.hpp")
NOT_CODEGEN = ("-fPIC", "-shared", "-fvisibility=hidden", "-Wall", "-Wno-unused-function")      # of build.FLAGS: what a device-only compile has no use for
PROBE_ONLY = ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-S"]
_probes = {}


def command(hipcc, src, out):
    """the probe's command line"""
    return [hipcc, *[f for f in build.FLAGS if f not in NOT_CODEGEN], *build.VARIANT_FLAGS["fast"], *PROBE_ONLY, str(src), "-o", str(out)]


def compile_probe(instantiations, headers=SHADE_HEADERS, asm=False):
    """`template __global__ void <instantiation>;` for each entry, behind `headers` (paths from the repository's root) -> the compiler's
    resource remarks, or (remarks, assembly) when asm is asked for"""
    key = (tuple(instantiations), tuple(headers))
    if key not in _probes:
        try: hipcc = build.hipcc()
        except RuntimeError: pytest.skip("hipcc not found")
        with tempfile.TemporaryDirectory(prefix="kernel_probe") as tmp:
            src, out = os.path.join(tmp, "probe.hip"), os.path.join(tmp, "probe.s")
            with open(src, "w") as f:
                f.write("#include <hip/hip_runtime.h>\n#include <algorithm>\n#include <cmath>\n#include <cstdio>\n#include <cstdlib>\n#include <cstring>\n"
                        + "".join(f'#include "{ROOT}/{h}"\n' for h in headers) + "".join(f"template __global__ void {inst};\n" for inst in instantiations))
            run = subprocess.run(command(hipcc, src, out), capture_output=True, text=True, timeout=600)
            assert run.returncode == 0, run.stderr[-2000:]
            with open(out) as f: _probes[key] = (run.stderr, f.read())
    return _probes[key] if asm else _probes[key][0]


def resources(remarks, prefix):
    """the remarks' record of the one kernel whose mangled name starts with `prefix` -> {vgprs, spilled, scratch, lds, sgprs_spilled, waves}"""
    blocks = [blk for blk in remarks.split("Function Name: ")[1:] if blk.split("\n")[0].strip().startswith(prefix)]
    assert len(blocks) == 1, (prefix, remarks[-2000:])

    def figure(pattern):
        m = re.search(pattern, blocks[0])
        assert m, (pattern, blocks[0])
        return int(m.group(1))

    return {"vgprs": figure(r" VGPRs: (\d+)"), "spilled": figure(r" VGPRs Spill: (\d+)"), "scratch": figure(r"ScratchSize \[bytes/lane\]: (\d+)"),
            "lds": figure(r"LDS Size \[bytes/block\]: (\d+)"), "sgprs_spilled": figure(r"SGPRs Spill: (\d+)"), "waves": figure(r"Occupancy \[waves/SIMD\]: (\d+)")}


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
