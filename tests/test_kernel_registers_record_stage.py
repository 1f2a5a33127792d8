"""Occupancy guard for C1 / C2's queue-fed shade kernel with its record staged in LDS a row ahead (csrc/shade_stage.hpp
k_shade_traced_lean_staged): the compile probe (tests/kernel_probe.py) for that instantiation.  It keeps the budget of
the kernel with the direct loads - seven waves per SIMD: at most 72 VGPRs, nothing spilled, no scratch - and its LDS (4 KiB per wave for the
staged record) must leave seven workgroups resident in a compute unit's 160 KiB."""
from kernel_probe import compile_probe, resources

INST = "k_shade_traced_lean_staged<0x002, 0x01>(DevScene, Params, Queues, Counters*, int, int)"
PREFIX = "_Z26k_shade_traced_lean_stagedILi2ELi1EE"
VGPR_BUDGET, WAVES, CU_LDS_BYTES = 72, 7, 160 * 1024


def test_staged_record_shade_kernel_keeps_seven_waves():
    u = resources(compile_probe([INST]), PREFIX)
    vgprs, spilled, scratch, waves, lds = u["vgprs"], u["spilled"], u["scratch"], u["waves"], u["lds"]
    print(f"{INST}: {vgprs} VGPRs, {spilled} spilled, {scratch} B of scratch, {waves} waves per SIMD, {lds} B of LDS per workgroup")
    assert vgprs <= VGPR_BUDGET and spilled == 0 and scratch == 0, f"{vgprs} VGPRs, {spilled} spilled, {scratch} B of scratch; budget {VGPR_BUDGET}, no spill, no scratch"
    assert lds * WAVES <= CU_LDS_BYTES, f"{lds} B of LDS per workgroup: {WAVES} workgroups need {lds * WAVES} of {CU_LDS_BYTES} B"
