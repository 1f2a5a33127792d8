"""The float64 model of emitter_sample_hit (tests/f64_models.py) against the CPU oracle on the same Philox stream, on every stratum of
tests/emitter_cases.py, and the properties of the model that need no oracle.  No device: this is what the GPU test
(tests/test_gpu_emitter_samples.py) multiplies - the oracle's own |o - r| / (u S) - and the proof that its strata exist and behave:
draws and NaN pattern equal, every knife-edge cap met by the model alone, the rows placed on an edge inside the two-branch rule."""
import numpy as np
import pytest

import emitter_cases as E
import f64_models as M
from conftest import record_metric


@pytest.fixture(scope="module", params=E.SCENE_TAGS)
def case(request, parsed):
    return E.case(request.param, parsed)


def test_oracle_matches_the_model_on_every_stratum(case):
    c = case
    o, r = c.o, c.r
    assert np.array_equal(o[:, 7], r[:, 7])                                          # draws: 3 for a mesh light, 2 for a sphere light
    assert np.array_equal(r[:, 7], [M.EMITTER_DRAWS[k] for k in c.kind])
    assert np.array_equal(np.isnan(o), np.isnan(r)), np.where(np.isnan(o) != np.isnan(r))[0][:8]
    q = E.ratios(o[:, :7], r[:, :7], c.S[:, :7]).max(axis=1)
    over = []
    for st in np.unique(c.stratum[~c.edge]):
        s = c.stratum == st
        k = s & c.keep
        kind = c.kind[s][0]
        m = {"scene": c.tag, "stratum": st, "rows": int(s.sum()), "left_out": int((s & ~c.keep).sum()), "max_ratio": float(q[k].max()),
             "p50": float(np.percentile(q[k], 50)), "bound": E.ORACLE_ROUNDINGS[kind]}
        record_metric("emitter_sample_oracle", m)
        print(m)
        if not m["max_ratio"] <= m["bound"]:
            over.append(m)
    assert not over, over
    # outside every knife edge the decisions are the model's: dark where it is dark, pdf 1 where the light faces away, pdf 0 for a beam
    k = c.keep
    assert np.array_equal(np.all(o[k, 3:6] == 0, axis=1), np.all(r[k, 3:6] == 0, axis=1))
    assert np.array_equal(o[k, 6] == 1.0, r[k, 6] == 1.0) and np.all(o[c.kind == "collimated", 6] == 0.0)
    fixed = np.isin(c.kind, ["point", "spot"])
    assert np.array_equal(np.float32(o[fixed, 0:3]), np.float32(r[fixed, 0:3]))


def test_knife_edge_cap_holds_on_the_model_alone(case):
    c = case
    for st in np.unique(c.stratum[~c.edge]):
        s = c.stratum == st
        out = int((s & ~c.keep).sum())
        assert out < 0.01 * s.sum(), (st, out, int(s.sum()))
    assert not c.keep[c.edge].any() and (c.edge.any() or set(c.kind) == {"point"})        # (a point light has no edge of its own)


def test_on_edge_rows_follow_one_adjacent_branch(case):
    """the oracle on the rows placed on an edge: its outputs are the model's on one of the branches next to the edge, and it has a
    NaN only where that branch of the model has one (a sphere light sampled from its own centre)"""
    c = case
    bad = E.two_branch_failures(c, c.o, None, E.ORACLE_ROUNDINGS)
    for st in np.unique(c.stratum[c.edge]):
        s = c.stratum == st
        free = np.all(E.within(c.o[s, :7], None, c.r[s, :7], c.S[s, :7], E.ORACLE_ROUNDINGS[c.kind[s][0]]), axis=1)
        record_metric("emitter_sample_oracle_edge", {"scene": c.tag, "stratum": st, "rows": int(s.sum()), "other_branch": int((~free).sum())})
    assert not bad, bad[:8]


def test_model_properties(case):
    """(a) the point of a mesh light lies in the triangle picked, (b) the point of a sphere light on the sphere, (c) the pdf of a lit
    sample is the solid-angle pdf MIS uses at that point: on the model to float64 precision (the packed inverse area is a float32 of
    its own: 2 u), and on the oracle inside its rounding count; every sampled position inside the boxes the culls are built on"""
    c = case
    tiny = 1e-9 * np.maximum(np.abs(np.nan_to_num(c.r[:, :7], posinf=0.0)), 1.0)
    assert not E.property_failures(c, c.r, tiny)
    K = np.array([E.ORACLE_ROUNDINGS[k] for k in c.kind])[:, None]
    assert not E.property_failures(c, c.o, E.allowance(None, c.r[:, :7], c.S[:, :7], K))
    assert not E.containment_failures(c, c.r) and not E.containment_failures(c, c.o)


# (d) the estimator integrates to the solid angle the emitter subtends: intensity / Le = 1 / pdf on the lit samples, 0 on the others
SOLID = [("synthetic", 3), ("features_a", 0)]         # the sphere of radius 0.3; a quad of two equal triangles


@pytest.mark.parametrize("tag,k", SOLID)
def test_model_estimates_the_solid_angle(tag, k, parsed):
    """16 384 samples from each of three hit points: the mean of intensity / Le within 5 standard errors of the closed form (a sphere)
    or of Van Oosterom - Strackee summed over the triangles (the equal-area quad).  The 7-triangle light is not held to this: upstream
    picks a triangle uniformly whatever its area (abtract_source.py:119, "ASSUME that triangles are similar in terms of area"), so its
    estimator does not integrate to the solid angle, and the model restates upstream."""
    c = E.case(tag, parsed)
    g = c.geoms[k]
    if g[0] == "mesh":
        area = np.linalg.norm(np.cross(np.float64(g[1]), np.float64(g[2])), axis=1)
        assert len(area) == 2 and abs(area[0] - area[1]) <= 1e-6 * area[0]
    for p, omega in E.solid_angle_points(c, k):
        w = E.solid_angle_model(c, k, p)
        z = (w.mean() - omega) / (w.std(ddof=1) / np.sqrt(len(w)))
        record_metric("emitter_sample_solid_angle_model", {"scene": tag, "src": k, "omega": omega, "mean": float(w.mean()), "z": float(z)})
        print(tag, k, omega, w.mean(), z)
        assert abs(z) <= 5.0, (tag, k, p, omega, w.mean(), z)
