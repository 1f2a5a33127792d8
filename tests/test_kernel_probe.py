"""tests/kernel_probe.py probes the build that ships: its command line, reduced to the flags that decide the code generated, is the product
build's (adapt_amd/build.py FLAGS + VARIANT_FLAGS["fast"]) - so a kernel guard cannot silently judge a different build."""
import kernel_probe
from adapt_amd import build


def codegen_flags(flags):
    """a compile's flags without those that only say what to write where, how to link it, or what to warn about"""
    dropped = ("-fPIC", "-shared", "-c", "-S", "--cuda-device-only")
    return [f for f in flags if f not in dropped and not f.startswith(("-W", "-fvisibility", "-Rpass"))]


def test_the_probe_compiles_with_the_product_builds_flags():
    cmd = kernel_probe.command("hipcc", "probe.hip", "probe.s")
    assert cmd[0] == "hipcc" and cmd[-3:] == ["probe.hip", "-o", "probe.s"]
    assert "-Rpass-analysis=kernel-resource-usage" in cmd and "--cuda-device-only" in cmd
    assert codegen_flags(cmd[1:-3]) == codegen_flags(build.FLAGS + build.VARIANT_FLAGS["fast"])
    assert "-DAPT_FAST=1" in cmd and "--offload-arch=gfx950" in cmd      # (the reduction keeps what it is about)
