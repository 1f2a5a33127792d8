"""Occupancy guard for the camera-fed twin of C1 / C2's shade kernel (csrc/shade_stage.hpp k_shade_traced_lean_cam): the
compile probe (tests/kernel_probe.py) for the instantiation that makes its camera rays itself.  It ships at the budget of the
queue-fed kernel - seven waves per SIMD: at most 72 VGPRs, nothing spilled, no scratch - and the queue-fed kernel, compiled next to it, must
keep the figures it had before the twin existed."""
from kernel_probe import compile_probe, resources

# (explicit instantiation, mangled-name prefix, VGPR budget, why)
KERNELS = [
    ("k_shade_traced_lean_cam<0x002, 0x01>(DevScene, Params, Queues, Counters*, const unsigned long long*)", "_Z23k_shade_traced_lean_camILi2ELi1EE", 72,
     "C1 / C2: camera vertex shaded where the camera ray is traced, seven waves per SIMD"),
    ("k_shade_traced_lean<0x002, 0x01>(DevScene, Params, Queues, Counters*, int, int)", "_Z19k_shade_traced_leanILi2ELi1EE", 72,
     "C1 / C2: rays traced in place, seven waves per SIMD (unchanged by the twin)"),
]


def test_camera_fed_shade_kernel_keeps_seven_waves():
    remarks = compile_probe([inst for inst, *_ in KERNELS])
    for inst, prefix, budget, why in KERNELS:
        u = resources(remarks, prefix)
        vgprs, spilled, scratch, waves = u["vgprs"], u["spilled"], u["scratch"], u["waves"]
        print(f"{inst}: {vgprs} VGPRs, {spilled} spilled, {scratch} B of scratch, {waves} waves per SIMD")
        assert vgprs <= budget and spilled == 0 and scratch == 0 and waves >= 7, f"{inst}: {vgprs} VGPRs, {spilled} spilled, {scratch} B of scratch, {waves} waves; budget {budget} ({why})"
