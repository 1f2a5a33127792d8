"""Occupancy guard for the hot kernels.  A kernel's register allocation decides how many waves a SIMD holds (512 VGPRs per lane: <= 128 ->
four waves, <= 96 -> five, <= 72 -> seven), and it is the maximum over every path the compiler sees, including ones a config never takes: an innocent
change elsewhere in the stage headers can cost C2's shade kernel its fourth wave (-10 %: it happened, profiles/NOTES.md).  This test compiles the
hot instantiations for gfx950 with -Rpass-analysis=kernel-resource-usage (tests/kernel_probe.py; ~10 s) and holds each to
the budget it ships with."""
from kernel_probe import SHADE_HEADERS, compile_probe, resources

# (explicit instantiation, mangled-name prefix, VGPR budget, why)
KERNELS = [
    ("k_shade_traced_lean<0x002, 0x01>(DevScene, Params, Queues, Counters*, int, int)", "_Z19k_shade_traced_leanILi2ELi1EE", 72, "C1 / C2: rays traced in place, seven waves per SIMD"),
    ("k_shade_group<0x05, 5, 0x002, 0x504, 0x200, 0x801, 0, 0>(DevScene, Params, Queues, Counters*, GroupIn, int, int)", "_Z13k_shade_groupILi5ELi5ELi2ELi1284ELi512ELi2049ELi0ELi0EE", 96, "C4: the lean group of class kernels, five waves per SIMD, spot lights"),
    ("k_extend_dyn<1>(DevScene, Params, Queues, Counters*, int, const uint32_t*, LdsPlan)", "_Z12k_extend_dynILi1EE", 72, "C4 / C5: closest-hit walk, seven waves per SIMD"),
    ("k_shade_group<0x03, 5, 0x002, 0x504, 0x200, 0x801, 0, 0>(DevScene, Params, Queues, Counters*, GroupIn, int, int)", "_Z13k_shade_groupILi3ELi5ELi2ELi1284ELi512ELi2049ELi0ELi0EE", 96, "C3 / C5: the lean group of class kernels, five waves per SIMD (one 8-byte scratch slot)"),
    ("k_shade_group<0x03, 4, 0x001, 0x040, 0x080, 0x008, 0x010, 0x020>(DevScene, Params, Queues, Counters*, GroupIn, int, int)", "_Z13k_shade_groupILi3ELi4ELi1ELi64ELi128ELi8ELi16ELi32EE", 128, "C3 / C5: every other class kernel in one four-wave group"),
    ("k_vshade_ev_group<0x03, 0, 4, 0x002, 0x040, 0x504, 0x200>(DevScene, Params, Queues, Counters*, VGroupIn, int)", "_Z17k_vshade_ev_groupILi3ELi0ELi4ELi2ELi64ELi1284ELi512EE", 128, "V1 / V2: the four-wave group of surface events of the volumetric tracer"),
    ("k_extend_flat<1, 1>(DevScene, Params, Queues, Counters*, int, const uint32_t*, LdsPlan)", "_Z13k_extend_flatILi1ELi1EE", 96, "C3: hot flat sweep, five waves per SIMD"),
]


def test_hot_kernels_keep_their_register_budget():
    remarks = compile_probe([inst for inst, *_ in KERNELS], SHADE_HEADERS + ("adapt_amd/csrc/volumetric.hpp",))
    for inst, prefix, budget, why in KERNELS:
        u = resources(remarks, prefix)
        vgprs, spilled, scratch = u["vgprs"], u["spilled"], u["scratch"]
        # a scratch budget of 16 bytes per lane: the lean group with area lights parks ONE 8-byte constant there under its five-wave
        # bound; anything beyond that is a spill in a hot loop
        assert vgprs <= budget and spilled <= 1 and scratch <= 16, f"{inst}: {vgprs} VGPRs, {spilled} spilled, {scratch} B of scratch; budget {budget} ({why})"
