"""The tolerance rule's constants shared by the product build's function tests (tests/test_gpu_product_functions.py states the rule,
tests/test_gpu_texture_chain.py applies it to the maps of a vertex).  Not collected by pytest (no `test_` prefix); nothing here needs a
device."""
import numpy as np

import f64_models as M

# family: K = the budget count along the model's longest chain of substituted operations (floor 1 where there is none)
FAMILIES = {
    "blinn_phong":   2,    # one pow (OCML powf); normalize() and the rest are IEEE in both builds
    "mod_phong":     2,    # one pow in eval, one (separate) in pdf
    "lambertian":    1,    # no substituted operation
    "oren_nayar":    3,    # raw_of_local: v_rsq (localize's fnormalize) + v_sqrt (sin_t) + v_rcp (cos_p = x / sin_t)
    "thin_coat":     3,    # its Oren-Nayar core: as above
    "microfacet":    3,    # to_raw of the half vector: v_rsq + v_sqrt + v_rcp
    "fresnel_blend": 2,    # one pow
    "mirror":        1,
    "glass":         1,    # delta: the same code in both builds
    "lambert_trans": 1,
    "media":         2,    # phase function: nothing substituted; transmittance: OCML expf in both builds (glibc's in the oracle)
    "media_free_path": 4,  # -logf(1 - u) / u_e, then expf of the path: two OCML calls along the chain
    # solid-angle pdf: one sdiv = v_rcp (1 ulp) AND a multiplication whose rounding the IEEE quotient does not have; the budget of
    # "1 per v_rcp" leaves that rounding out (measured 1.07 against a budget of 1), so it is counted here: 1 + 1
    "emitter_pdf":   2,
    # emitter_sample_hit per emitter type (tests/test_gpu_emitter_samples.py), counted along the longest chain to an output:
    "emitter_sample_point":      1,   # srcp = v_rcp (1); the oracle takes the same reciprocal, then the same min and product
    "emitter_sample_mesh":       3,   # fnormalize(diff) = v_rsq (1), sdiv(|diff|^2, dl) = v_rcp (1), fdiv3(intensity, pdf) = v_rcp (1)
    "emitter_sample_sphere":     8,   # sin_t = v_sqrt (1), sincos (OCML, 2), the frame's fnormalize = v_rsq (1), sdiv(p, r^2) = v_rcp (1), then the mesh light's 3
    "emitter_sample_spot":       2,   # fnorm = v_sqrt (1), fdiv3(intensity, depth^2) = v_rcp (1); the cone test's v_rcp feeds a decision only
    "emitter_sample_collimated": 1,   # the ssqrt feeds the rim decision only: no output substitutes anything
    # shade_stage.hpp surface_maps (tests/test_gpu_texture_chain.py): a frame is R = c I + k n n^T + [axis]x with n = fnormalize(axis), and
    # fnormalize is axis * v_rsq in the product build.  The one v_rsq (1 ulp = up to 2 u relative) scales n, n enters every entry twice
    # (k n_i n_j: 4 u), and k = 1 - c reaches 2 where the target is next to -Y, where c + k n_i^2 = -1 + 2 is a result of the size of the
    # output: 2 x 2 x 2 = 8 u S per frame in the worst case (a float32 restatement with the reciprocal square root moved by one ulp gives
    # exactly 8.0 on such a row, one the oracle gets exactly; 4 where the target is at right angles to Y), on top of the roundings every
    # build makes, which the floor of 1 stands for: 9 per frame.  One frame for a normal map or a bump map, two for a bump map on a
    # normal-mapped vertex; the lookups substitute nothing.
    "maps_one_frame":  9,
    "maps_two_frames": 18,
}
AGG = 2.0


def _ratio(x, r, S):
    x, r = np.asarray(x, np.float64), np.asarray(r, np.float64)
    both_nan = np.isnan(x) & np.isnan(r)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.abs(x - r) / (M.U * S)
    return np.where(both_nan | (x == r), 0.0, np.where(np.isnan(q), np.inf, q))
