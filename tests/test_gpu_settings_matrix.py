"""Every render pipeline under every sensor setting (tests/settings_cases.py), on the device, both builds.

The scene files carry a handful of combinations of the nine sensor settings, and every other device-vs-oracle image test takes its
settings from them.  Here each setting is flipped alone (and in a few pairs) on five scenes, and the render is held to

  (a) the oracle on the same Philox stream, exact build, 64 x 48 x 20 spp (twenty passes sample 16, where the stratified cell index wraps),
      SURVEY 8(d) as tests/test_gpu_parity.py::test_image_matches_oracle_same_stream holds it; two cases per scene also on a 50 x 30 film;
  (b) the reference's own kernel run with the same overrides (tests/golden/settings_matrix.npz), exact build, without the oracle in between;
  (c) the oracle on the same stream, product build, at the film and the bound of the scene's row in parity_bounds.PRODUCT_IMAGE_CASES
      (media_a: the bounds of the volumetric product test), counters at the product build's tolerance;
  (d) each other: the alternatives the environment switches select at renderer creation render what the default pipeline renders, by the
      criterion the existing test of that switch uses at the scene's own settings;
  (e) itself: splitting a render call or changing the batch size does not change a bit of the accumulation.

Every run asserts the pipeline it took (shade variant, traversal, camera fusion) against `expected_pipeline`, a restatement of
csrc/api.hip pick_traversal / pick_shading, and enters it into RAN; the last test reads RAN: every axis value has run on every pipeline
that can take it.  The number of light samples S chooses among five pipelines (S == 1 rays traced in place, S > 1 on the flat sweep
samples queued by vertex, 2..4 otherwise one radiance plane per sample, >= 5 one shared plane, 0 no shadow stage), so an axis value
"can take" a pipeline if it leaves S free or sets it inside that pipeline's range; (d) renders the flag cases of balls_mono once more
with S = 1 (traced, non-lean) and S = 5 (one shared plane) for that.

All measured figures go through record_metric; the log of record is profiles/r06_settings_matrix_metrics.log.
"""
from collections import namedtuple

import numpy as np
import pytest

import parity_bounds as PB                      # the bounds tests/test_gpu_parity.py and tests/test_gpu_fast.py assert: read, not copied
import settings_cases as SC
from conftest import golden, image_metrics, record_metric
from gpu_ab import COUNTERS, Run, differences, open_renderer
from gpu_cases import COUNTER_KEYS, OTHER_SEED_FILM, counters_within, other_seed_criterion
from adapt_amd.scene_pack import make_config, pack_scene

pytestmark = pytest.mark.gpu

BUILDS = ("exact", "fast")
EXACT_WITHIN, EXACT_REL, EXACT_COUNTERS = PB.EXACT          # SURVEY 8(d), as test_image_matches_oracle_same_stream holds the exact build to it
REFRUN_WITHIN, REFRUN_REL, REFRUN_DRAWS = PB.REFERENCE_RUN  # test_image_matches_reference_run: the exact build against a reference-run fixture
FILM_A = (64, 48, 20)
FILM_ODD = (50, 30, 20)                         # 1500 pixels: no multiple of 64
ODD_AXES = ("rr_off", "shadow_5")               # the two cases per scene that also run on the odd film (both axes exist on all five scenes)
FILM_D = (64, 48, 16)                           # test_rays_traced_in_place_render_the_staged_pipeline_s_image's film
FILM_TRAVERSAL = (64, 48, 8)                    # test_every_traversal_mode_gives_the_same_hits_and_image's film

# Same-stream figures of the product build on the cases that miss their scene's row in parity_bounds.PRODUCT_IMAGE_CASES although the exact build
# holds 8(d) on them in (a), the product build's counters stay inside their tolerance and the other-seed criterion holds (all three asserted,
# for each of them, by the tests below): case -> measured (frac_within, relMSE) at the row's film, profiles/r06_settings_matrix_metrics.log
# ("product same-stream <case>").  `_own_bound` makes the bound from them.  What moves them: more light samples per vertex or roulette at every vertex are more
# branches per vertex for an ulp in a hit point to flip; without jitter every sample of a pixel sends the same camera ray, so a flipped
# branch is repeated by all 64 samples; without MIS a path that runs into the emitter carries its whole radiance, and a re-drawn one moves
# its pixel by that much (glass_box, features_a: relMSE only, the fraction of pixels is the row's).
OWN_BOUNDS = {
    "cbox-rr_every_vertex": (0.998915, 1.161e-6),
    "cbox-no_jitter": (0.999349, 3.007e-6),
    "cbox-no_jitter+rr_off+mis_off": (0.999349, 3.006e-6),
    "cbox-shadow_2": (0.998589, 9.58e-7),
    "cbox-shadow_5": (0.998806, 1.399e-6),
    "cbox-shadow_5+two_sided": (0.998698, 1.746e-6),
    "cbox-shadow_8": (0.999457, 2.938e-6),
    "balls_mono-shadow_2": (0.995226, 1.337e-6),
    "balls_mono-no_jitter+rr_off+mis_off": (0.997613, 9.007e-6),
    "glass_box-mis_off": (0.961046, 9.193e-4),
    "features_a-mis_off": (0.884874, 4.430e-4),
}
# The same for (d): the product build under APT_TRAVERSAL=bvh against 8(d).  Its tree walk tests a leaf with the flat sweep's arithmetic (t
# within 1e-5 relative of the reference's loop), so a path is re-drawn now and then; without MIS one such path is a firefly: measured
# 99.90 % of the pixels (3 of 3072 differ) and relMSE 4.22e-4 at 64 x 48 x 8 on both cases, counters within 2e-4, and the exact build under
# the same switch holds 8(d) on them.  (switch value, case) -> measured (frac_within, relMSE).
TRAVERSAL_OWN_BOUNDS = {
    ("bvh", "balls_mono-mis_off"): (0.9990234, 4.221e-4),
    ("bvh", "balls_mono-mis_off+two_sided"): (0.9990234, 4.221e-4),
}


def _own_bound(row, measured):
    """this project's convention for a guard made from a measurement: the shortfall from 1 doubled, the relMSE doubled"""
    assert not (measured[0] >= row[0] and measured[1] <= row[1]), "the case meets its row: it needs no bound of its own"
    return 1.0 - 2.0 * (1.0 - measured[0]), 2.0 * measured[1]


PIPELINES = ("lean traced, camera-fused", "traced, non-lean", "class-sorted groups", "staged, l_planes 2..4", "staged, one shared plane",
             "nee_vm", "volumetric event-sorted", "BVH walk")
RAN = {p: set() for p in PIPELINES}             # pipeline -> axis labels that ran on it (filled by every render of this module)
MULTI_CLASS = {"cbox": False, "balls_mono": True, "glass_box": True, "features_a": True, "media_a": True}
Took = namedtuple("Took", "variant traversal fused")             # the pipeline a renderer took, as _enter asserts it


def expected_pipeline(scene, build, S, max_bounce, env):
    """csrc/api.hip pick_traversal / pick_shading / make_camera_strips restated for the five scenes of the matrix (all small enough for the
    flat sweep): -> (traversal or None where the exact build chooses between its two sweeps, kind of shade variant, camera fused)"""
    vol = SC.SCENES[scene][3]
    forced = env.get("APT_TRAVERSAL")
    trav = forced if forced else ("flat" if build == "fast" else None)
    is_sorted = MULTI_CLASS[scene] and env.get("APT_SORTED") != "0" and not vol
    traced = build == "fast" and trav == "flat" and not is_sorted and not vol and S == 1 and env.get("APT_FUSED", "2") != "0"
    kind = "volumetric" if vol else ("traced" if traced else ("sorted" if is_sorted else "plain"))
    return trav, kind, bool(traced and env.get("APT_CAMERA_FUSE") != "0" and max_bounce >= 1)


def _enter(r, case, build, env, axis=None):
    """assert the pipeline this renderer took and enter it into RAN; -> Took"""
    st = SC.settings(case)
    S, mb = r.num_shadow_ray, r.max_bounce
    info, fused = r.info(), r.camera_fused()
    name, trav = info["shade_variant"], info["traversal"]
    want_trav, kind, want_fused = expected_pipeline(case.scene, build, S, mb, env)
    what = (case.name, build, env, name, trav, fused)
    assert info["arithmetic"] == build, what
    assert trav == want_trav if want_trav else trav in ("sweep", "tile"), what
    assert fused is want_fused, what
    assert ("[rays traced in place]" in name) == (kind == "traced"), what
    assert name.startswith("sorted, launched in register-footprint groups:") == (kind == "sorted"), what
    assert name.startswith("volumetric, sorted by event:") == (kind == "volumetric"), what
    assert (r.use_rr, r.use_mis, r.anti_alias, r.stratified_sample) == (st["use_rr"], st["use_mis"], st["anti_alias"], st["stratified_sampling"]), what
    took = []
    if kind == "volumetric": took.append("volumetric event-sorted")
    if kind == "traced":
        lean = name.startswith("lambertian/point")
        if lean and fused: took.append("lean traced, camera-fused")
        if not lean: took.append("traced, non-lean")
    else:                                       # staged: a shadow stage of its own (if S > 0)
        if kind == "sorted": took.append("class-sorted groups")
        nee_vm = kind != "volumetric" and trav == "flat" and S > 1
        if nee_vm: took.append("nee_vm")
        elif 2 <= S <= 4: took.append("staged, l_planes 2..4")
        elif S >= 5: took.append("staged, one shared plane")
    if trav == "bvh": took.append("BVH walk")
    for p in took:
        RAN[p].add(axis or case.axis)
    return Took(name, trav, fused)


def _open(case, build, w, h, env=None, extra=None, **kw):
    tup = SC.with_overrides(SC.parse(case.scene), dict(case.overrides, **(extra or {})))
    return open_renderer(tup, w, h, env=env, exact=(build == "exact"), volumetric=case.volumetric, **kw)


_oracle_scenes, _oracle_images = {}, {}


def _oracle(case, w, h, spp, seed=0, extra=None):
    """the oracle's render of the case (cached: the exact and the product build, and the switches of (d), share it, unchanged)"""
    from oracle import binding as ob
    key = (case.name, w, h, spp, seed, tuple(sorted((extra or {}).items())))
    if key not in _oracle_images:
        tup = SC.parse(case.scene)
        if case.scene not in _oracle_scenes:
            _oracle_scenes[case.scene] = ob.OracleScene(pack_scene(*tup), make_config(tup[3]).cam_t)
        rc = make_config(SC.with_overrides(tup, dict(case.overrides, **(extra or {})))[3], width=w, height=h, seed=seed, volumetric=case.volumetric)
        img, cnt, st = _oracle_scenes[case.scene].render(rc, spp, threads=ob.num_threads())
        assert cnt == spp
        img.setflags(write=False)
        _oracle_images[key] = (img, st)
    return _oracle_images[key]


def _render(case, build, w, h, spp, env=None, extra=None, axis=None, **kw):
    """-> (accumulation, counters, Took); the renderer is closed before the next one opens"""
    with _open(case, build, w, h, env, extra, **kw) as r:
        took = _enter(r, case, build, env or {}, axis)
        r.render(n_spp=spp)
        return r.color.to_numpy(), r.stats(), took


def _against_oracle(label, case, acc, st, w, h, spp, extra=None):
    """-> (image metrics, largest relative counter deviation, problems with exact sample counts and the shadow stage)"""
    ref, ost = _oracle(case, w, h, spp, extra=extra)
    m = image_metrics(acc / spp, ref / spp)
    dev = {k: abs(st[k] - ost[k]) / max(1, ost[k]) for k in COUNTER_KEYS}
    record_metric(label, dict(m, **{f"{k}_rel_dev": v for k, v in dev.items()}, n_draws=st["n_draws"], n_shade=st["n_shade"], n_shadow=st["n_shadow"]))
    bad = []
    if not (st["n_samples"] == ost["n_samples"] == w * h * spp): bad.append(("n_samples", st["n_samples"], ost["n_samples"]))
    S = (extra or {}).get("num_shadow_ray", SC.settings(case)["num_shadow_ray"])
    if S == 0 and (st["n_shadow"] != 0 or ost["n_shadow"] != 0): bad.append(("n_shadow with no light samples", st["n_shadow"]))
    if S > 0 and st["n_shadow"] == 0 and ost["n_shadow"] > 0: bad.append(("no light sample taken", ost["n_shadow"]))
    return m, dev, bad


def _exact_8d(label, case, acc, st, film, extra=None):
    """8(d) on the exact build -> list of what missed"""
    m, dev, bad = _against_oracle(label, case, acc, st, *film, extra=extra)
    if not (m["frac_within"] >= EXACT_WITHIN and m["relMSE"] <= EXACT_REL): bad.append(m)
    bad += [(k, v) for k, v in dev.items() if not v <= EXACT_COUNTERS]
    return bad


def _report(failures):
    for f in failures: print(f)
    assert not failures, f"{len(failures)} case(s) missed: {[f[0] for f in failures]}"


# ---------------------------------------------------------------- (a) exact build vs the oracle, same stream
@pytest.mark.parametrize("scene", list(SC.SCENES))
def test_exact_build_matches_the_oracle_under_every_setting(scene):
    failures = []
    for case in SC.cases_of(scene):
        for film in (FILM_A,) + ((FILM_ODD,) if case.axis in ODD_AXES else ()):
            w, h, spp = film
            acc, st, _ = _render(case, "exact", w, h, spp)
            bad = _exact_8d(f"exact same-stream {case.name} {w}x{h}x{spp}", case, acc, st, film)
            if bad: failures.append((case.name, film, bad))
    assert sum(c.axis in ODD_AXES for c in SC.cases_of(scene)) == 2
    _report(failures)


# ---------------------------------------------------------------- (b) exact build vs the reference's own run
@pytest.mark.parametrize("scene", list(SC.SCENES))
def test_exact_build_matches_the_reference_run_under_every_setting(scene):
    g = golden("settings_matrix.npz")
    w, h, spp = SC.FIXTURE_W, SC.FIXTURE_H, SC.FIXTURE_SPP
    failures = []
    for case in SC.cases_of(scene):
        acc, st, _ = _render(case, "exact", w, h, spp, seed=SC.FIXTURE_SEED)
        ref, total = g[f"{case.name}:accum"], int(g[f"{case.name}:draws"].sum())
        m = image_metrics(acc / spp, ref / spp)
        dd = abs(st["n_draws"] - total) / total
        record_metric(f"exact vs reference run {case.name} {w}x{h}x{spp}", dict(m, n_draws=st["n_draws"], n_draws_reference=total))
        if not (m["frac_within"] >= REFRUN_WITHIN and m["relMSE"] <= REFRUN_REL and dd <= REFRUN_DRAWS and st["n_samples"] == w * h * spp):
            failures.append((case.name, m, st["n_draws"], total))
    _report(failures)


# ---------------------------------------------------------------- (c) product build vs the oracle, same stream
def _product_film_and_row(scene):
    """film, (min frac_within, max relMSE) and the counters' check: the scene's 96 x 96 x 64 row of parity_bounds.PRODUCT_IMAGE_CASES;
    media_a has none: the oracle leg of test_volumetric_product_build_vs_reference_run_and_oracle (its fixture's film, 16 spp)"""
    if SC.SCENES[scene][3]:
        b = PB.VPT_PRODUCT_BOUNDS
        g = golden(f"vptscene_{scene}.npz")
        return (int(g["width"]), int(g["height"]), 16), (b["within"], b["rel"]), lambda st, ost: counters_within(st, ost, b["stat_tol"], 0)
    rows = [r for r in PB.PRODUCT_IMAGE_CASES if r[0] == scene and r[4] == {}]
    assert len(rows) == 1 and rows[0][1:4] == (96, 96, 64), rows
    return rows[0][1:4], rows[0][5:7], counters_within


def _other_seed(case, env=None):
    """test_gpu_fast.test_statistical_cross_check_other_seed's criterion, film and spp on this case"""
    w, h, spp = OTHER_SEED_FILM
    cpu = {seed: _oracle(case, w, h, spp, seed=seed)[0].astype(np.float64) / spp for seed in (0, 1, 2)}
    acc, _, _ = _render(case, "fast", w, h, spp, env=env, seed=0)
    frac = PB.SAME_SEED_FRACTION_OF_NOISE.get(case.scene)          # (media_a has no entry: 8(d)'s 1e-4 outright)
    other_seed_criterion(case.name, acc.astype(np.float64) / spp, cpu, frac)


N_PARTS = 4          # the twenty cases of a full-matrix scene in four test functions of a few seconds each (96 x 96 x 64 on the oracle)


@pytest.mark.parametrize("part", range(N_PARTS))
@pytest.mark.parametrize("scene", list(SC.SCENES))
def test_product_build_matches_the_oracle_under_every_setting(scene, part):
    (w, h, spp), row, counters = _product_film_and_row(scene)
    failures = []
    for case in SC.cases_of(scene)[part::N_PARTS]:
        acc, st, _ = _render(case, "fast", w, h, spp)
        m, dev, bad = _against_oracle(f"product same-stream {case.name} {w}x{h}x{spp}", case, acc, st, w, h, spp)
        try:
            counters(st, _oracle(case, w, h, spp)[1])
        except AssertionError as e:
            bad.append(("counters", str(e)))
        if not SC.SCENES[scene][3]:
            mean_a, mean_b = float(np.nanmean(acc / spp)), float(np.nanmean(_oracle(case, w, h, spp)[0] / spp))
            if not abs(mean_a - mean_b) <= 0.01 * mean_b: bad.append(("energy", mean_a, mean_b))
        min_within, max_rel = _own_bound(row, OWN_BOUNDS[case.name]) if case.name in OWN_BOUNDS else row
        if not (m["frac_within"] >= min_within and m["relMSE"] <= max_rel):
            bad.append(("same-stream bound", min_within, max_rel, m))
        if case.name in OWN_BOUNDS or bad:
            # a bound of its own is earned: the estimator is the same one (and a case that misses says here whether it is)
            try:
                _other_seed(case)
            except AssertionError as e:
                bad.append(("other-seed criterion", str(e)))
        if bad: failures.append((case.name, bad))
    _report(failures)


# ---------------------------------------------------------------- (d) the pipelines agree with each other
def _traced_vs_staged(a, b, what):
    """test_rays_traced_in_place_render_the_staged_pipeline_s_image's criterion: b is the staged render (or, for APT_SORTED, the sorted one:
    sorting changes which kernel shades a vertex and the order of the adds into a radiance slot, not the arithmetic of a (ray, record) pair
    or of a shading model, so the same criterion holds: an add order changes a sum of at most 8 terms by 8 x 2^-24 << 1e-4)"""
    (img, st), (img0, st0) = a, b
    bad = []
    if not (st["n_samples"] == st0["n_samples"] and st["n_extend"] >= st["n_samples"]): bad.append(("n_samples", st["n_samples"], st0["n_samples"], st["n_extend"]))
    for k in ("n_extend", "n_shade", "n_shadow", "n_shadow_traced", "n_lit", "n_draws"):
        if not abs(st[k] - st0[k]) <= max(2, 1e-4 * st0[k]): bad.append((k, st[k], st0[k]))
    fin = np.isfinite(img0) & np.isfinite(img)
    close = np.abs(img - img0)[fin] <= 1e-4 * (1.0 + np.abs(img0[fin]))
    record_metric(what, {"finite": float(fin.mean()), "close": float(close.mean())})
    if not fin.mean() > 0.999: bad.append(("finite", float(fin.mean())))
    if not close.mean() >= 0.99: bad.append(("close", float(close.mean())))
    return bad


def _bit_identical(a, b):
    """tests/gpu_ab.py's bit identity, and no generate launch in the fused form; a, b: what _render returns, fused and two-launch"""
    run = lambda img, st, took: Run(took.variant, took.traversal, img, st, None, took.fused)
    bad = differences(run(*b), run(*a))
    l1, l0 = a[1]["launches"], b[1]["launches"]
    if not (l1["generate"] == 0 and l0["generate"] > 0): bad.append(("generate launches", l1, l0))
    return bad


D_PARTS = 10         # two cases a test function: a case of balls_mono is a dozen renders and three oracle images


@pytest.mark.parametrize("part", range(D_PARTS))
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("scene", ["cbox", "balls_mono"])
def test_pipeline_switches_render_the_same_image_under_every_setting(scene, build, part):
    failures = []
    w, h, spp = FILM_D
    for case in SC.cases_of(scene)[part::D_PARTS]:
        S, bad = SC.settings(case)["num_shadow_ray"], []
        free_S = "num_shadow_ray" not in case.overrides           # the case leaves the light-sample count to the scene
        run = lambda env, extra=None, film=FILM_D, axis=None: _render(case, build, *film, env=env, extra=extra, axis=axis)
        # APT_FUSED: rays traced in place against the staged pipeline.  Multi-class scenes take the traced kernels unsorted with one light
        # sample per vertex (as the existing test renders balls_mono): the flag cases get S = 1 for it, the light-sample cases keep theirs.
        one = {"num_shadow_ray": 1} if (MULTI_CLASS[scene] and free_S) else None
        S_f = 1 if one else S
        base = {"APT_SORTED": "0"}
        if expected_pipeline(scene, build, S_f, 1, base)[1] == "traced":
            on, st_on, took = run(base, one)
            off, st_off, took0 = run(dict(base, APT_FUSED="0"), one)
            assert "[rays traced in place]" in took.variant and "[rays traced in place]" not in took0.variant and took.traversal == took0.traversal == "flat"
            bad += [("APT_FUSED=0",) + b for b in _traced_vs_staged((on, st_on), (off, st_off), f"APT_FUSED {build} {case.name}")]
            # APT_CAMERA_FUSE: the camera-fed launch against k_generate_trace + the queue-fed bounce 0
            off, st_off, took0 = run(dict(base, APT_CAMERA_FUSE="0"), one)
            assert took.fused is True and took0.fused is False and took0.variant == took.variant
            bad += [("APT_CAMERA_FUSE=0",) + b for b in _bit_identical((on, st_on, took), (off, st_off, took0))]
        else:                                   # nothing to trace in place, nothing to fuse: the switches leave the pipeline as it is
            for env in ({"APT_FUSED": "0"}, {"APT_CAMERA_FUSE": "0"}):
                with _open(case, build, w, h, env) as r:
                    assert _enter(r, case, build, env).fused is False
        # APT_SORTED: one all-models kernel against the class kernels (a scene of one class is not sorted in the first place)
        if MULTI_CLASS[scene]:
            srt, st_s, took_s = run({})
            uns, st_u, took_u = run({"APT_SORTED": "0"})
            assert took_s.variant.startswith("sorted") and not took_u.variant.startswith("sorted") and took_s.traversal == took_u.traversal
            bad += [("APT_SORTED=0",) + b for b in _traced_vs_staged((uns, st_u), (srt, st_s), f"APT_SORTED {build} {case.name}")]
        # APT_TRAVERSAL: the BVH walk and the tiled sweep against the oracle (test_every_traversal_mode_gives_the_same_hits_and_image's image
        # criterion, 8(d)); the flag cases of balls_mono once more with five light samples - one shared radiance plane
        for mode in ("bvh", "tile"):
            routes = [(None, None)] + ([({"num_shadow_ray": 5}, case.axis)] if (scene == "balls_mono" and free_S and mode == "tile") else [])
            for extra, axis in routes:
                acc, st, took = run({"APT_TRAVERSAL": mode}, extra, FILM_TRAVERSAL, axis)
                assert took.traversal == mode
                label = f"APT_TRAVERSAL={mode} {build} {case.name}{' S=5' if extra else ''}"
                own = TRAVERSAL_OWN_BOUNDS.get((mode, case.name)) if (build == "fast" and not extra) else None
                if own is None:
                    b = _exact_8d(label, case, acc, st, FILM_TRAVERSAL, extra=extra)
                else:                           # (the exact build's run of this test holds 8(d) on the case under the same switch)
                    m, dev, b = _against_oracle(label, case, acc, st, *FILM_TRAVERSAL)
                    min_within, max_rel = _own_bound((EXACT_WITHIN, EXACT_REL), own)
                    if not (m["frac_within"] >= min_within and m["relMSE"] <= max_rel): b.append(("bound of its own", min_within, max_rel, m))
                    b += [(k, v) for k, v in dev.items() if not v <= EXACT_COUNTERS]
                    try:
                        _other_seed(case, {"APT_TRAVERSAL": mode})
                    except AssertionError as e:
                        b.append(("other-seed criterion", str(e)))
                bad += [(f"APT_TRAVERSAL={mode}", extra, x) for x in b]
        if bad: failures.append((case.name, bad))
    _report(failures)


# ---------------------------------------------------------------- (e) per-pixel sample independence under the settings
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("axis", ["mis_off", "rr_off", "uniform_jitter"])
def test_split_calls_and_batch_sizes_leave_the_accumulation_bit_identical(axis, build):
    """One light sample per vertex: every float is added in a fixed order, so 20 spp in one call, in calls of 7 + 13, and in batches of 3
    give the same accumulation, compared as uint32 (test_cbox_is_bit_reproducible_and_batch_invariant checks the scene's own settings)"""
    case = SC.BY_NAME[f"cbox-{axis}"]
    assert SC.settings(case)["num_shadow_ray"] == 1
    w, h = 64, 48
    out = {}
    for key, calls, kw in (("one call", (20,), {}), ("7 + 13", (7, 13), {}), ("batches of 3", (20,), {"spp_per_batch": 3})):
        with _open(case, build, w, h, **kw) as r:
            _enter(r, case, build, {})
            for n in calls:
                r.render(n_spp=n)
            assert r.cnt[None] == 20 and (key != "batches of 3" or r.info()["spp_per_batch"] == 3)
            out[key] = (r.color.to_numpy().view(np.uint32).copy(), {k: r.stats()[k] for k in COUNTERS})
    assert out["one call"][0].any()
    for key in ("7 + 13", "batches of 3"):
        assert np.array_equal(out[key][0], out["one call"][0]), (axis, build, key, int((out[key][0] != out["one call"][0]).sum()))
        assert out[key][1] == out["one call"][1], (axis, build, key)


# ---------------------------------------------------------------- every axis value ran on every pipeline that can take it
def _can_take(axis, pipeline):
    S = SC.AXES[axis].get("num_shadow_ray")
    if S is None:
        return True                             # a flag or a bounce limit leaves S free: every pipeline
    return {"lean traced, camera-fused": S == 1, "traced, non-lean": S == 1, "staged, l_planes 2..4": 2 <= S <= 4, "staged, one shared plane": S >= 5,
            "nee_vm": S >= 2}.get(pipeline, True)


def test_every_axis_value_ran_on_every_pipeline_that_can_take_it():
    """reads what the tests above entered into RAN: run the whole module (an `-k` selection of this test alone has nothing to read)"""
    missing = {p: sorted(a for a in SC.AXES if _can_take(a, p) and a not in RAN[p]) for p in PIPELINES}
    missing = {p: m for p, m in missing.items() if m}
    if missing:
        for p in PIPELINES: print(p, sorted(RAN[p]))
    assert not missing, missing
