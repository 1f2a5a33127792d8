"""Static guard for the 56-byte path record of the lean traced shade kernels (csrc/stages.hpp TrRecord, csrc/shade_stage.hpp shade_traced
C56): one compile probe (tests/kernel_probe.py) builds each of the five 56-byte kernels beside its 64-byte twin, with the
product build's flags.

Resources: each 56-byte kernel keeps the lean kernels' budget - seven waves per SIMD: at most 72 VGPRs, no VGPR spilled, no scratch (the
twins themselves keep 41 to 87 scalar registers in lanes of a spill VGPR: not held here) - and its LDS per workgroup is not above its
twin's; the two staged forms, whose wave area shrinks from 4 KiB to 3.5 KiB, are strictly below (19 472 -> 17 424 B).

Row loop: the 56-byte kernel's row loop (kernel_probe.loop_counts: the largest span a backward branch closes) issues no more vector
instructions than its twin's in the same compile.  The bound is the twin, whatever the compiler release makes of both.

As built, VALU of the row loop, twin -> 56-byte kernel:
    staged_live  1 512 -> 1 509     staged  1 590 -> 1 579     lean  1 576 -> 1 561
    cam_live     2 263 -> 2 258     cam     2 331 -> 2 329
A queue-fed row loses the reader's d * t + o (six instructions: the build does not contract) and gains it as the writer; a camera-fed
row only gains it.  What pays for it there: a staged ray's plane A is stored whole in its rare branch, so the row makes the packed word
without the "nothing hit" test and the point into the registers of the vertex's own; a camera ray's record has no plane D; the staged
camera ray's words that the 56-byte form does not store are not made.  The counts move by a handful with the scalar registers the
compiler keeps in lanes: `cam` takes the writer's other slot form for that reason (shade_stage.hpp append_record, TURN)."""
import pytest

from kernel_probe import compile_probe, loop_counts, resources

VGPR_BUDGET, WAVES = 72, 7
QUEUE_ARGS, CAM_ARGS = "(DevScene, Params, Queues, Counters*, int, int)", "(DevScene, Params, Queues, Counters*, const unsigned long long*)"
# 64-byte twin, 56-byte kernel, argument list, the wave stages its record in LDS
PAIRS = {
    "lean": ("k_shade_traced_lean", "k_shade_traced_lean56", QUEUE_ARGS, False),
    "staged": ("k_shade_traced_lean_staged", "k_shade_traced_lean56_staged", QUEUE_ARGS, True),
    "staged_live": ("k_shade_traced_lean_staged_live", "k_shade_traced_lean56_staged_live", QUEUE_ARGS, True),
    "cam": ("k_shade_traced_lean_cam", "k_shade_traced_lean56_cam", CAM_ARGS, False),
    "cam_live": ("k_shade_traced_lean_cam_live", "k_shade_traced_lean56_cam_live", CAM_ARGS, False),
}


def _inst(name, args): return f"{name}<0x002, 0x01>{args}"
def _prefix(name): return f"_Z{len(name)}{name}ILi2ELi1EE"


@pytest.fixture(scope="module")
def probe():
    """the ten instantiations compiled once -> (the compiler's resource remarks, the assembly)"""
    return compile_probe([_inst(n, args) for twin, compact, args, _ in PAIRS.values() for n in (twin, compact)], asm=True)


@pytest.mark.parametrize("which", sorted(PAIRS))
def test_compact_record_kernel_keeps_the_seven_wave_budget(probe, which):
    twin, compact, _, staged = PAIRS[which]
    u, t = resources(probe[0], _prefix(compact)), resources(probe[0], _prefix(twin))
    print(f"{compact}: {u}\n{twin}: {t}")
    assert u["vgprs"] <= VGPR_BUDGET and u["spilled"] == 0 and u["scratch"] == 0 and u["waves"] == WAVES, u
    if staged: assert u["lds"] < t["lds"], f"{u['lds']} B of LDS per workgroup, the 64-byte twin has {t['lds']}"
    else: assert u["lds"] <= t["lds"], f"{u['lds']} B of LDS per workgroup, the 64-byte twin has {t['lds']}"


@pytest.mark.parametrize("which", sorted(PAIRS))
def test_compact_record_row_loop_issues_no_more_vector_instructions(probe, which):
    twin, compact, _, _ = PAIRS[which]
    n, valu, vmov = loop_counts(probe[1], _prefix(compact))
    n_t, valu_t, vmov_t = loop_counts(probe[1], _prefix(twin))
    print(f"{compact}: row loop of {n} instructions, {valu} VALU, {vmov} v_mov_b32; {twin}: {n_t}, {valu_t}, {vmov_t}")
    assert n > 1000 and n_t > 1000, f"no row loop found: the largest back-edge spans hold {n} and {n_t} instructions"
    assert valu <= valu_t, f"{valu} VALU in the 56-byte row loop, {valu_t} in the 64-byte twin's"
