"""The pane-stack scenes of tests/null_stack_cases.py on the CPU: the float64 model of the transmittance walk on known answers, the
oracle's track_ray held to it past the second crossing and up to the seven-segment limit, and the scenes' own properties that the
GPU tests (tests/test_gpu_null_stack.py) lean on."""
import numpy as np
import pytest

import null_stack_cases as ns
from conftest import record_metric


def test_boxes_are_wound_outwards_and_the_panes_stay_out_of_the_frustum():
    tris = ns.box((1, 2, 3), (2, 4, 7))
    assert tris.shape == (12, 3, 3) and tris.dtype == np.float32
    assert np.array_equal(tris.reshape(-1, 3).min(axis=0), [1, 2, 3]) and np.array_equal(tris.reshape(-1, 3).max(axis=0), [2, 4, 7])
    ref = ns.side_reference()
    pts = ref["points"]
    # every sample meets the quad, left of the first pane; between camera and quad the frustum is narrower still
    assert np.abs(pts[..., 0]).max() < ns.SIDE_QUAD_HALF < ns.SIDE_X0 and np.all(pts[..., 2] == ns.SIDE_QUAD_Z)
    for k in ns.SIDE_KS:
        _, _, objs, _ = ns.side_stack(k)
        assert len(objs) == 1 + k + 1                                   # quad, panes, the backstop behind the light


def test_walk_model_on_known_answers():
    """a sample along +x from the origin (cos = 1): lengths are the pane thicknesses themselves"""
    light, u_e = (40.0, 0.0, 0.0), np.float64([0.1, 0.3, 0.6])
    p = (0.0, 0.0, 0.0)
    for k in range(0, 7):
        seg, T, tau = ns.walk_model(p, k, None, light, u_e)
        assert seg == min(2 * k + 1, 7)
        assert np.allclose(tau, u_e * ns.SIDE_DX * min(k, 3), rtol=0, atol=1e-15) and np.allclose(T, np.exp(-tau), rtol=1e-15)
    for j, want in ((1, 3), (2, 5), (3, 7)):
        seg, T, _ = ns.walk_model(p, 5, j, light, u_e)
        assert seg == want and not T.any()
    for j in (4, 5):
        seg, T, tau = ns.walk_model(p, 5, j, light, u_e)
        assert seg == 7 and np.allclose(tau, u_e * ns.SIDE_DX * 3, rtol=0, atol=1e-15)
    # a light in front of the second pane: the walk ends there, after three segments
    seg, T, tau = ns.walk_model(p, 4, None, (ns.side_pane_x(2)[0] - 0.1, 0.0, 0.0), u_e)
    assert seg == 3 and np.allclose(tau, u_e * ns.SIDE_DX)
    # oblique: every length grows by 1 / cos
    seg, T, tau = ns.walk_model((0.0, 0.0, 0.0), 2, None, (30.0, 0.0, 40.0), u_e)
    assert seg == 5 and np.allclose(tau, u_e * 2 * ns.SIDE_DX / 0.6, rtol=1e-14)


def test_oracle_walk_follows_the_float64_model_to_the_seventh_segment():
    """pixel(k) / pixel(0) of the oracle's 1 spp renders against the model's transmittance at every lit pixel and channel, within
    K_RATIO 2^-24 (1 + optical depth) (null_stack_cases.K_RATIO derives the constant); segments per sample as the model counts them."""
    ref = ns.side_reference()
    img0, st0 = ref["oracle"][(0, None)]
    assert st0["n_shadow"] == ns.SIDE_W * ns.SIDE_H and st0["n_track"] == st0["n_shadow"]
    worst = 0.0
    for k in ns.SIDE_KS:
        img, st = ref["oracle"][(k, None)]
        err, lit = ns.ratio_error(img, img0, k)
        record_metric(f"null stack side k={k} oracle", {"max_err_in_2^-24(1+tau)": err, "lit_pixels": lit, "segments_per_sample": st["n_track"] / st["n_shadow"]})
        assert lit == ns.SIDE_W * ns.SIDE_H                             # the quad fills the view and the light reaches all of it
        assert err <= ns.K_RATIO, (k, err)
        assert st["n_track"] / st["n_shadow"] >= ns.min_segments(k)
        assert st["n_track"] == int(ref["model"][k][2].sum())           # segment for segment
        worst = max(worst, err)
    assert worst == ns.oracle_max_error() > 0                           # the figure the device's bound is a multiple of
    # the fourth pane is never seen
    for k in (4, 6):
        assert np.array_equal(ref["oracle"][(k, None)][0].view(np.uint32), ref["oracle"][(3, None)][0].view(np.uint32))
    assert not np.array_equal(ref["oracle"][(2, None)][0], ref["oracle"][(3, None)][0])


def test_oracle_sheet_blocks_within_seven_segments_only():
    ref = ns.side_reference()
    ns.check_sheets({j: ref["oracle"][(5, j)][0] for j in ns.SIDE_SHEETS}, ref["oracle"][(0, None)][0])
    for j, seg in ((1, 3), (2, 5), (3, 7), (4, 7), (5, 7)):
        st = ref["oracle"][(5, j)][1]
        assert st["n_track"] == seg * st["n_shadow"] and st["n_lit"] == (0 if j <= 3 else st["n_shadow"])
    assert np.array_equal(ref["oracle"][(5, 4)][0].view(np.uint32), ref["oracle"][(3, None)][0].view(np.uint32))


@pytest.mark.parametrize("case", ns.FRONT_CASES)
def test_front_stacks_reach_what_they_are_for(case):
    """the oracle's own statistics of the front stacks: light samples walk well past three segments, camera paths extend through many
    pass-through iterations, the scenes fit the flat sweep's records"""
    tup, rc, img, st = ns.front_reference(case)
    assert tup[1]["primitives"].shape[0] <= 96 and rc.max_bounce == 4 and rc.use_rr and rc.rr_bounce_th == 1
    seg = st["n_track"] / st["n_shadow"]
    ext = st["n_extend"] / st["n_samples"]
    want_seg, want_ext = {"k1": (2.5, 3.0), "k3": (5.0, 5.0), "k6": (5.0, 7.0), "scatter": (4.5, 5.0), "world": (3.5, 4.0), "nested": (3.0, 3.5)}[case]
    assert seg >= want_seg and ext >= want_ext, (case, seg, ext)
    assert np.isfinite(img).all() and img.mean() > 0


def test_null_panes_fixture_walks_to_the_limit():
    """scenes/test/null_panes.xml (tests/golden/vptscene_null_panes.npz): at least a tenth of its light samples walk five or more
    segments.  With at most seven segments per sample and m the mean, the share f of samples with five or more obeys m <= 7 f + 4 (1 - f)."""
    from conftest import scene_from_golden
    from adapt_amd.scene_pack import make_config, pack_scene
    from oracle import binding as ob
    tup, g = scene_from_golden("null_panes", "vptscene")
    rc = make_config(tup[3], seed=int(g["seed"]), use_bvh=False, volumetric=True)
    st = ob.OracleScene(pack_scene(*tup), rc.cam_t).render(rc, int(g["spp"]))[2]
    mean = st["n_track"] / st["n_shadow"]
    assert (mean - 4.0) / 3.0 >= 0.1, mean
