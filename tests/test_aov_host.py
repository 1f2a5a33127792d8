"""Feature buffers, the part that needs no device: the oracle-side facts the GPU tests (tests/test_gpu_aov.py) lean on."""
import numpy as np
import pytest

import aov_cases as ac


@pytest.mark.parametrize("film", ac.FILMS, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("name", sorted({v[0] for v in ac.CASES.values()}))
def test_centre_rays_have_few_near_ties(name, film, parsed):
    """The product build may pick the other of two candidates that lie within 1e-5 of each other; the GPU test allows that on at most
    0.1 % of the rays.  The scenes it uses have fewer such rays than that to begin with."""
    scene = ac.scene_of(name, parsed, anti_alias=False)
    osc, rc, fs = ac.oracle_of(scene, *film)
    d = ac.centre_rays(osc, rc)
    o = np.tile(np.float32(rc.cam_t), (len(d), 1))
    ties = ac.near_ties(fs, o, d)
    assert ties.sum() <= ac.TIE_CAP * len(d), (int(ties.sum()), len(d))
    # the float64 candidates agree with the oracle's own intersector on what is hit at all
    hit = ac.oracle_aov(osc, fs, rc, d)[0]
    cand = np.isfinite(ac.candidate_distances(fs, o[::7], d[::7]).min(axis=1))
    assert np.mean(cand == hit[::7]) >= 0.999


@pytest.mark.parametrize("name", ["cbox", "balls_mono"])
def test_trace_sample_logs_the_camera_hit_as_event_0(name, parsed):
    """With anti-aliasing on, the GPU test takes a pixel-sample's first hit from OracleScene.trace_sample: its event 0 must be the
    camera ray's hit - the primitive and distance the oracle's intersector gives for pix2ray's direction under the sample's own jitter -
    and a sample whose camera ray hits nothing must log no event at all."""
    w, h, spp = 64, 48, 8
    scene = ac.scene_of(name, parsed, anti_alias=True)
    osc, rc, fs = ac.oracle_of(scene, w, h)
    assert rc.anti_alias and rc.max_bounce >= 1
    rows = []
    for i in range(0, w, 3):
        for j in range(0, h, 3):
            for s in range(1, spp + 1):
                _, ev, _ = osc.trace_sample(rc, i, j, s, max_events=2)
                d = osc.pix2ray(rc, i, j, s, ac.jitter(rc, i, j, s))
                rows.append((d, len(ev), ev[0, 1] if len(ev) else -1, ev[0, 2] if len(ev) else 0))
    d = np.float32([r[0] for r in rows])
    _, prim, t, _, _ = osc.intersect(np.tile(np.float32(rc.cam_t), (len(d), 1)), d)
    n_ev, ev_prim, ev_t = np.int32([r[1] for r in rows]), np.int32([r[2] for r in rows]), np.float32([r[3] for r in rows])
    assert np.array_equal(n_ev > 0, prim >= 0)
    hit = prim >= 0
    assert hit.sum() > 0.5 * len(d)
    assert np.array_equal(ev_prim[hit], prim[hit]) and np.array_equal(ev_t[hit], t[hit])
