"""Static guard for the live-row form of C1 / C2's two shade kernels (csrc/shade_stage.hpp shade_traced LIVE: k_shade_traced_lean_staged_live,
k_shade_traced_lean_cam_live): the compile probe (tests/kernel_probe.py), with its assembly,
for the two instantiations.  Each keeps the parent kernel's budget (seven waves per SIMD: at most 72 VGPRs, nothing spilled, no scratch, the
parent's LDS), and its row loop - the largest span of the kernel's assembly that a backward branch closes - issues fewer vector instructions
than the parent's: the form exists to take the dead lanes' default writes (v_mov_b32 of 0 / 1.0 / -1, phi copies) out of that loop.

Counts, VALU / v_mov_b32 per row loop, by kernel_probe.loop_counts():
    queue-fed   parent 1 591 / 204 (k_shade_traced_lean_staged)   live rows 1 502 / 121
    camera-fed  parent 2 332 / 263 (k_shade_traced_lean_cam)      live rows 2 262 / 206
The bounds are the live rows' counts plus a margin of 10 (compiler point releases move a few instructions); the queue-fed loop must also
stay at least 50 VALU below the parent's 1 591."""
import pytest

from kernel_probe import compile_probe, loop_counts, resources

VGPR_BUDGET, MARGIN = 72, 10
PARENT_STAGED_VALU = 1591
# instantiation, mangled prefix, LDS bytes per workgroup (the parent kernel's), VALU and v_mov_b32 of the row loop as built
KERNELS = {
    "staged": ("k_shade_traced_lean_staged_live<0x002, 0x01>(DevScene, Params, Queues, Counters*, int, int)", "_Z31k_shade_traced_lean_staged_liveILi2ELi1EE", 19472, 1502, 121),
    "cam": ("k_shade_traced_lean_cam_live<0x002, 0x01>(DevScene, Params, Queues, Counters*, const unsigned long long*)", "_Z28k_shade_traced_lean_cam_liveILi2ELi1EE", 16, 2262, 206),
}


@pytest.fixture(scope="module")
def probe():
    """both instantiations compiled once -> (the compiler's resource remarks, the assembly)"""
    return compile_probe([inst for inst, *_ in KERNELS.values()], asm=True)


@pytest.mark.parametrize("which", sorted(KERNELS))
def test_live_row_kernel_keeps_the_parents_budget(probe, which):
    inst, prefix, lds_parent, _, _ = KERNELS[which]
    u = resources(probe[0], prefix)
    vgprs, spilled, scratch, lds = u["vgprs"], u["spilled"], u["scratch"], u["lds"]
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
