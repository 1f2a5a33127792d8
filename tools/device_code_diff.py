#!/usr/bin/env python3
"""Device code of two builds of the library, side by side - what a host-only change must leave untouched:

    python tools/device_code_diff.py OLD/libadapt_mi.so NEW/libadapt_mi.so [more OLD NEW pairs]

Per pair: the exported symbols (nm -D --defined-only, less the per-translation-unit __hip_cuid_ ids), every kernel's recorded registers, scratch and LDS (tools/kernel_meta.py) and the
disassembly of every function symbol of the gfx950 code objects (instruction text and encoding, without addresses).  Prints one line
per check and the names that differ; exit status 1 if anything does.
"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_meta import LLVM, MAGIC, kernel_meta  # noqa: E402


def exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    # (without __hip_cuid_<hash>: the toolchain's id of a translation unit, a hash over its path and text)
    return sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip() and not ln.split()[-1].startswith("__hip_cuid_"))


def functions(lib):
    """{symbol: [instruction lines]} over every gfx950 code object in `lib`"""
    fns = {}
    with tempfile.TemporaryDirectory() as td:
        fb = os.path.join(td, "fatbin")
        subprocess.run([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fb}", lib], capture_output=True, check=True)
        blob = open(fb, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
        for k, at in enumerate(starts):
            part, co = os.path.join(td, f"bundle{k}"), os.path.join(td, f"k{k}.co")
            open(part, "wb").write(blob[at:starts[k + 1] if k + 1 < len(starts) else len(blob)])
            r = subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={part}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], capture_output=True)
            if r.returncode != 0 or not os.path.exists(co):
                continue
            name = None
            for ln in subprocess.run([f"{LLVM}/llvm-objdump", "-d", co], capture_output=True, text=True, check=True).stdout.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln)
                if m:
                    name = m.group(1)
                    fns[name] = []
                elif name and ln.strip():
                    fns[name].append(re.sub(r"//\s*[0-9A-Fa-f]+:", "//", ln.strip()))       # (the encoding stays, the address goes)
    return fns


def compare(what, a, b):
    names = sorted(set(a) | set(b))
    bad = [n for n in names if a.get(n) != b.get(n)]
    print(f"  {what}: {len(names)} compared, {len(bad)} differ")
    for n in bad:
        print(f"    DIFFERS: {n}" + ("" if n in a and n in b else f" (only in {'old' if n in a else 'new'})"))
    return len(bad)


def main(argv):
    if len(argv) < 2 or len(argv) % 2:
        print(__doc__)
        return 2
    bad = 0
    for old, new in zip(argv[0::2], argv[1::2]):
        print(f"{os.path.basename(old)}: old against new")
        ea, eb = exported(old), exported(new)
        print(f"  exported symbols: {len(ea)} old, {len(eb)} new, {'same' if ea == eb else 'DIFFERENT: ' + ' '.join(sorted(set(ea) ^ set(eb)))}")
        bad += ea != eb
        bad += compare("kernels (names; vgpr, agpr, sgpr, scratch, lds)", kernel_meta(old), kernel_meta(new))
        fa, fb = functions(old), functions(new)
        n_ins = sum(len(v) for v in fb.values())
        bad += compare(f"device functions (disassembly, {n_ins} instructions in new)", fa, fb)
    print("identical" if not bad else f"{bad} difference(s)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
