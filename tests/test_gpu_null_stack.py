"""Null-surface walks past the second crossing, on the device: the pane stacks of tests/null_stack_cases.py under both builds and every
transmittance walk each can take (null_stack_cases.WALKS), against the float64 model of the walk (side stack), against the oracle on
the same stream (front stack), and the invariances of the null-surface tail (tests/test_null_stack.py holds the oracle to the model)."""
import numpy as np
import pytest

import null_stack_cases as ns
from conftest import image_metrics, record_metric
from gpu_ab import assert_same_run, open_renderer, run_of
from gpu_cases import counters_within

pytestmark = pytest.mark.gpu

WALKS = list(ns.WALKS)
BUILD_WALKS = {b: [w for w in WALKS if ns.WALKS[w][0] == b] for b in ("fast", "exact")}


def _render(tup, w, h, spp, walk, null_surfaces=True, **kw):
    """-> (accumulated image / spp, stats) of the scene under the row `walk`, after asserting that the row's build and walk ran"""
    build, env, _, _ = ns.WALKS[walk]
    with open_renderer(tup, w, h, env=env, exact=(build == "exact"), volumetric=True, **kw) as r:
        r.render(n_spp=spp)
        ns.assert_walk(r, walk, null_surfaces)
        return r.color.to_numpy() / spp, r.stats()


def _side(walk, k, sheet=None):
    return _render(ns.side_stack(k, sheet), ns.SIDE_W, ns.SIDE_H, 1, walk, null_surfaces=(k > 0))


# ---------------------------------------------------------------- the side stack against the float64 model
@pytest.mark.parametrize("walk", WALKS)
def test_side_stack_follows_the_float64_model(walk):
    """pixel(k) / pixel(0) of the device's own 1 spp renders against the model's transmittance at every pixel the k = 0 image lights,
    within DEVICE_MARGIN x the oracle's measured maximum (in units of 2^-24 (1 + optical depth)); each light sample walks the model's
    segments; a sheet behind pane 1, 2 or 3 of five blocks, behind pane 4 or 5 it is never seen."""
    bound = ns.DEVICE_MARGIN * ns.oracle_max_error()
    img0, st0 = _side(walk, 0)
    assert st0["n_shadow_traced"] == ns.SIDE_W * ns.SIDE_H == st0["n_track"]
    worst = {}
    for k in ns.SIDE_KS[1:]:
        img, st = _side(walk, k)
        err, lit = ns.ratio_error(img, img0, k)
        per_sample = st["n_track"] / st["n_shadow_traced"]
        worst[f"k={k}"] = err
        print(f"side stack {walk} k={k}: error {err:.2f} of {bound:.2f}, {lit} lit pixels, {per_sample:.4f} segments per sample")
        assert lit == ns.SIDE_W * ns.SIDE_H
        assert per_sample >= ns.min_segments(k), (walk, k, per_sample)
        assert st["n_lit"] == st["n_shadow_traced"] == ns.SIDE_W * ns.SIDE_H
    record_metric(f"null stack side {walk}", dict(worst, bound=bound, oracle_max=ns.oracle_max_error()))
    assert max(worst.values()) <= bound, (walk, worst, bound)
    sheets = {j: _side(walk, 5, j) for j in ns.SIDE_SHEETS}
    ns.check_sheets({j: v[0] for j, v in sheets.items()}, img0)
    for j, seg in ((1, 3), (2, 5), (3, 7), (4, 7), (5, 7)):
        st = sheets[j][1]
        assert st["n_track"] / st["n_shadow_traced"] >= seg - 0.05 and st["n_lit"] == (0 if j <= 3 else st["n_shadow_traced"]), (walk, j, st)


@pytest.mark.parametrize("build", ["fast", "exact"])
def test_side_stack_segments_agree_across_the_walks_of_a_build(build):
    """segments walked and samples arrived are the same whichever walk of the build follows them; the product build's flat walk against
    its tiled walk also by the rule of test_gpu_fast.test_flat_transmittance_walk_against_the_tiled_walk"""
    for key in ((1, None), (3, None), (6, None), (5, 2), (5, 4)):
        runs = {w: _side(w, *key) for w in BUILD_WALKS[build]}
        first = runs[BUILD_WALKS[build][0]][1]
        for w, (_, st) in runs.items():
            assert (st["n_track"], st["n_lit"], st["n_shadow_traced"]) == (first["n_track"], first["n_lit"], first["n_shadow_traced"]), (key, w, st, first)
        if build == "fast":
            a, b = runs["fast/flat"], runs["fast/tile"]
            assert a[1]["n_shade"] == b[1]["n_shade"] and a[1]["n_draws"] == b[1]["n_draws"]
            m = image_metrics(a[0], b[0])
            assert m["frac_within"] >= 0.99 and m["relMSE"] <= 1e-4, (key, m)


# ---------------------------------------------------------------- the front stack against the oracle on the same stream
@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("case", ns.FRONT_CASES)
def test_front_stack_matches_the_oracle(case, walk):
    """the criterion of gpu_cases.volumetric_scene_vs_reference_run_and_oracle: 99 % of the pixels within 1e-3 (1 + x), relMSE <= 1e-3,
    vertices shaded, light samples and draws within 5e-4, samples exact, and no more segments walked than the oracle walks"""
    tup, rc, ref, ost = ns.front_reference(case)
    img, st = _render(tup, ns.FRONT_W, ns.FRONT_H, ns.FRONT_SPP, walk)
    m = image_metrics(img, ref / ns.FRONT_SPP)
    record_metric(f"null stack front {case} {walk}", dict(m, n_track=st["n_track"], n_track_oracle=ost["n_track"], n_extend=st["n_extend"], n_extend_oracle=ost["n_extend"]))
    print(f"front stack {case} {walk}: {m}, n_track {st['n_track']} of {ost['n_track']}")
    assert m["frac_within"] >= 0.99 and m["relMSE"] <= 1e-3, (case, walk, m)
    counters_within(st, ost, 5e-4, 0, label=(case, walk))
    assert st["n_samples"] == ost["n_samples"] == ns.FRONT_W * ns.FRONT_H * ns.FRONT_SPP
    assert 0 < st["n_track"] <= ost["n_track"] and st["n_lit"] <= ost["n_lit"] * (1 + 5e-4)


def test_front_stack_flat_walk_against_the_tiled_walk():
    """test_gpu_fast.test_flat_transmittance_walk_against_the_tiled_walk's rule where the flat kernel's own loop runs to the seventh segment"""
    tup = ns.front_reference("k6")[0]
    a, b = (_render(tup, ns.FRONT_W, ns.FRONT_H, 24, w) for w in ("fast/flat", "fast/tile"))
    assert a[1]["n_shadow_traced"] == b[1]["n_shadow_traced"] and a[1]["n_shade"] == b[1]["n_shade"] and a[1]["n_draws"] == b[1]["n_draws"]
    for k in ("n_track", "n_lit"):
        assert abs(a[1][k] - b[1][k]) <= max(1e-3 * b[1][k], 20), (k, a[1][k], b[1][k])
    m = image_metrics(a[0], b[0])
    assert m["frac_within"] >= 0.99 and m["relMSE"] <= 1e-4, m


# ---------------------------------------------------------------- invariances of the tail, six panes
@pytest.mark.parametrize("build", ["fast", "exact"])
def test_front_stack_invariances(build, monkeypatch):
    """bit for bit within a build: the same render twice, 8 spp in one call against 3 + 5, one render lane against the default number
    (two samples per batch: every lane gets batches, and tails), a crop window against the same window of the full frame"""
    tup = ns.front_reference("k6")[0]
    w, h, exact = ns.FRONT_W, ns.FRONT_H, build == "exact"

    def run(calls, **kw):
        with open_renderer(kw.pop("tup", tup), w, h, exact=exact, volumetric=True, **kw) as r:
            assert r.info()["arithmetic"] == build
            for n in calls:
                r.render(n_spp=n)
            return run_of(r, 0, calls=0), r.color.to_numpy().copy()
    base, img = run([8])
    assert base.stats["n_samples"] == w * h * 8 and base.stats["n_extend"] > 5 * base.stats["n_samples"]
    assert_same_run(base, run([8])[0], "twice")
    assert_same_run(base, run([3, 5])[0], "3 + 5")
    lanes = run([8], spp_per_batch=2)[0]
    monkeypatch.setenv("APT_LANES", "1")
    one = run([8], spp_per_batch=2)[0]
    monkeypatch.delenv("APT_LANES")
    assert_same_run(lanes, one, "lanes")
    assert_same_run(base, one, "batches")
    cx, cy, rx, ry = 26, 15, 13, 9
    crop_tup = (*tup[:3], dict(tup[3], film={"width": w, "height": h, "crop_x": cx, "crop_y": cy, "crop_rx": rx, "crop_ry": ry}))
    crop, cimg = run([8], tup=crop_tup)
    win = (slice(cx - rx, cx + rx), slice(cy - ry, cy + ry))
    assert np.array_equal(cimg[win].view(np.uint32), img[win].view(np.uint32))
    mask = np.ones((w, h), bool); mask[win] = False
    assert not cimg[mask].any() and crop.stats["n_samples"] == 8 * 4 * rx * ry
