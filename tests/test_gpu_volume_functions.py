"""The device's grid-volume functions (adapt_amd/csrc/volumetric.hpp: vol_intersect, vol_density, vol_pick_channel, vol_sample_mfp =
delta tracking, vol_transmittance = ratio tracking with roulette) through apt_volume_probe, on both builds.

Same stream (rows and seeds of tests/volume_cases.py; the oracle, orc_volume_probe, is pinned bit for bit to the reference's own
GridVolume by tests/test_volume_functions.py):
  * product build == exact build, every row of every mode, bit for bit: the volume code calls plain `/`, logf and expf, none of the
    helpers that differ between the builds;
  * intersect and lookup: device == oracle bit for bit (no transcendental on the chain), NaN for NaN;
  * sample_mfp and transmittance: device logf and glibc logf differ in the last bit, so once in about 1e-6 steps a row takes another
    decision.  Rows are split by the draw count.  Equal draws: same channel, same hit / no-hit flag, hit_t within the relative 2e-5
    test_medium_functions_vs_reference_vectors grants a free path, beta and the transmittance within the same bound (Tr is a product of
    values without a transcendental, the one division by pdf is IEEE on both sides).  Unequal draws: counted, at most 0.5 % of a
    stratum's rows (MAX_DIVERGED), the grazing stratum left to the float64 model.
  * grazing and zero-component strata against the float64 model (f64_models.volume_*), on the rows whose every decision is further
    from its branch than the float32 error the model derives for it (f64_models.VOLUME_SAFE); at most half a stratum may be left out.

Statistics (volume_cases.tracking_statistics): 27 rays x 2^16 streams against float64 quadrature of the trilinear field; thresholds
derived there.  The analytic image renders one absorbing volume in front of an area emitter through VolumeRenderer.
"""
import time

import numpy as np
import pytest

import volume_cases as VC
from conftest import record_metric
from oracle import binding as ob

pytestmark = pytest.mark.gpu

N_PER = 80                      # rows per (volume, stratum): 400 per stratum over the five volumes
MAX_DIVERGED = 0.005            # share of a stratum's rows whose draw count may differ from the oracle's
REL = 2e-5                      # hit_t, beta, transmittance on rows with equal draws
# share of rows on which the ORACLE's draw count differs from the float64 model's, sample_mfp and transmittance alike (measured on the
# CPU before the inputs were fixed; tests/test_f64_models.py test_volume_model_vs_oracle_divergence asserts each <= 0.25 %): every
# stratum was kept on this figure
ORACLE_VS_F64 = {"through": 0.0, "inside": 0.0, "clipped": 0.0, "short": 0.0, "miss": 0.0, "zero1": 0.0, "zero2": 0.0, "graze": 0.0}
T0 = time.time()


def _probe(variant, vol, mode, rows, seed=0):
    from adapt_amd import _lib
    from adapt_amd.renderer import volume_probe
    prev = _lib.use(variant)
    try:
        assert _lib.arithmetic(_lib.load()) == variant
        return volume_probe(*vol, mode, rows, seed=seed)
    finally:
        _lib.use(prev)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    """bit for bit, any NaN equal to any NaN"""
    a, b = np.float32(a), np.float32(b)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(_bits(a)[~nan], _bits(b)[~nan])


@pytest.fixture(scope="module")
def cases():
    vols, groups, dens = VC.same_stream_rows(N_PER, 120)
    return vols, groups, dens


def _by_volume(vols, groups):
    """one probe call per volume: rows of all strata concatenated, so a row's stream key is its index in that array"""
    for name, vol in vols.items():
        mine = [(s, r) for n, s, r in groups if n == name]
        rows = np.concatenate([r for _, r in mine])
        stratum = np.concatenate([[s] * len(r) for s, r in mine])
        yield name, vol, rows, stratum


def test_product_build_equals_exact_build_bit_for_bit(cases):
    vols, groups, dens = cases
    n = 0
    for name, vol, rows, _ in _by_volume(vols, groups):
        for mode, seed in ((0, 0), (2, VC.SEED_MFP), (3, VC.SEED_TR)):
            f, e = _probe("fast", vol, mode, rows, seed), _probe("exact", vol, mode, rows, seed)
            assert _same_bits(f, e), (name, mode, np.nonzero((_bits(f) != _bits(e)).any(axis=1))[0][:8])
            n += len(rows)
    for name, rows in dens:
        assert _same_bits(_probe("fast", vols[name], 1, rows), _probe("exact", vols[name], 1, rows)), name
        n += len(rows)
    record_metric("volume_functions.builds_bit_equal", {"rows": n, "different": 0})


@pytest.mark.parametrize("build", ["fast", "exact"])
def test_intersect_and_lookup_equal_the_oracle_bit_for_bit(build, cases):
    vols, groups, dens = cases
    for name, vol, rows, stratum in _by_volume(vols, groups):
        d, o = _probe(build, vol, 0, rows)[:, :3], ob.volume_probe(*vol, 0, rows)[:, :3]
        for s in VC.STRATA:
            m = stratum == s
            assert _same_bits(d[m], o[m]), (name, s, np.nonzero(m)[0][(_bits(d[m]) != _bits(o[m])).any(axis=1)][:8])
        for s, want in (("through", 1), ("inside", 1), ("clipped", 1), ("short", 0), ("miss", 0)):
            assert np.all(d[stratum == s, 0] == want), (name, s)
    for name, rows in dens:
        assert _same_bits(_probe(build, vols[name], 1, rows)[:, 0], ob.volume_probe(*vols[name], 1, rows)[:, 0]), name
    hit = np.concatenate([_probe(build, vol, 0, rows)[stratum == "graze", 0] for _, vol, rows, stratum in _by_volume(vols, groups)])
    gap = np.concatenate([np.diff(_probe(build, vol, 0, rows)[stratum == "graze", 1:3], axis=1)[:, 0] for _, vol, rows, stratum in _by_volume(vols, groups)])
    record_metric(f"volume_functions.intersect[{build}]", {"rows": 5 * len(VC.STRATA) * N_PER, "graze_hits": int(hit.sum()), "graze_gap_median": float(np.median(gap))})
    assert hit.sum() >= 0.25 * hit.size and np.median(np.abs(gap)) < 1e-4          # the stratum grazes: near_t and far_t a few 1e-5 apart


def _close(a, b):
    a, b = np.float64(a), np.float64(b)
    both_nan = np.isnan(a) & np.isnan(b)
    with np.errstate(invalid="ignore"):
        return both_nan | (np.abs(a - b) <= REL * np.abs(b))


def _rel_dev(a, b):
    a, b = np.float64(a), np.float64(b)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(a - b) / np.abs(b)
    r = r[np.isfinite(r)]
    return float(r.max()) if r.size else 0.0


@pytest.mark.parametrize("build", ["fast", "exact"])
@pytest.mark.parametrize("mode", [2, 3])
def test_tracking_on_the_oracle_stream(build, mode, cases):
    vols, groups, dens = cases
    seed, width, draws = (VC.SEED_MFP, 5, 4) if mode == 2 else (VC.SEED_TR, 4, 3)
    D, O, S = [], [], []
    for name, vol, rows, stratum in _by_volume(vols, groups):
        D.append(_probe(build, vol, mode, rows, seed)[:, :width]); O.append(ob.volume_probe(*vol, mode, rows, seed=seed)[:, :width]); S.append(stratum)
    D, O, S = np.concatenate(D), np.concatenate(O), np.concatenate(S)
    failures = []
    for s in VC.STRATA:
        m = S == s
        d, o = D[m], O[m]
        same = d[:, draws] == o[:, draws]
        share = 1.0 - same.mean()
        vec = slice(1, 4) if mode == 2 else slice(0, 3)
        ok = _close(d[same][:, vec], o[same][:, vec]).all(axis=1)
        ok &= ((d[same][:, vec] != 0) == (o[same][:, vec] != 0)).all(axis=1)      # the channel, and a roulette's zero
        if mode == 2:
            ok &= (d[same][:, 0] > 0) == (o[same][:, 0] > 0)                  # hit / no hit
            ok &= _close(d[same][:, 0], o[same][:, 0])
        record_metric(f"volume_functions.{'sample_mfp' if mode == 2 else 'transmittance'}[{build}][{s}]",
                      {"rows": int(m.sum()), "share_unequal_draws": float(share), "oracle_vs_f64_share": ORACLE_VS_F64.get(s, float("nan")),
                       "bit_equal_rows": int(sum(_same_bits(a, b) for a, b in zip(d, o))), "most_draws": int(o[:, draws].max()),
                       "max_rel_hit_t": _rel_dev(d[same][:, 0], o[same][:, 0]) if mode == 2 else 0.0, "max_rel_vector": _rel_dev(d[same][:, vec], o[same][:, vec])})
        if s != "graze" and share > MAX_DIVERGED:
            failures.append((s, "unequal draws", share))
        if not ok.all():
            failures.append((s, "rows", np.nonzero(m)[0][same][~ok][:8].tolist()))
    assert not failures, failures


@pytest.mark.parametrize("build", ["fast", "exact"])
def test_tracking_statistics_vs_quadrature(build):
    """the comparisons of tests/test_volume_functions.py::test_oracle_tracking_statistics_vs_quadrature on the device: same rays, stream
    counts, seeds and thresholds"""
    vols, rays = VC.stat_rays()
    failures = []
    for i, ray in enumerate(rays):
        vol = vols[ray["name"]]
        res = VC.tracking_statistics(lambda mode, rows, seed: _probe(build, vol, mode, rows, seed), vol, ray, VC.STAT_N, VC.STAT_SEED + 2 * i)
        record_metric(f"volume_functions.statistics[{build}][{i}:{ray['name']}/{ray['kind']}]", {k: float(v[0]) for k, v in res.items()})
        failures += [(i, ray["name"], ray["kind"], k, v) for k, v in res.items() if not v[0] <= v[1]]
    assert not failures, failures


@pytest.mark.parametrize("build", ["fast", "exact"])
def test_edge_strata_vs_the_float64_model(build, cases):
    """grazing and zero-component rays, all four functions against f64_models.volume_* on the device's own Philox words: every row whose
    decisions are all further than VOLUME_SAFE float32 errors (derived per operation in the model) from their branch has the model's
    draw count, channel, hit flag and, within 2e-5, its values.  At most half a stratum may be within that distance of a branch."""
    from adapt_amd.renderer import rng_stream
    vols, groups, dens = cases
    tally = {(s, mode): [0, 0, 0.0] for s in ("graze", "zero1", "zero2") for mode in (0, 2, 3)}
    failures = []
    for name, vol, rows, stratum in _by_volume(vols, groups):
        for mode, seed in ((0, 0), (2, VC.SEED_MFP), (3, VC.SEED_TR)):
            d = _probe(build, vol, mode, rows, seed)
            for s in ("graze", "zero1", "zero2"):
                idx = np.nonzero(stratum == s)[0]
                m, margin = VC.model_rows(vol, mode, rows[idx], seed, rng_stream, key0=int(idx[0]))
                safe, ok = VC.compare_with_model(d[idx], m, margin, mode)
                t = tally[(s, mode)]
                t[0] += len(idx); t[1] += int((~safe).sum())
                vec = slice(0, 5) if mode == 2 else slice(0, 3)
                t[2] = max(t[2], _rel_dev(d[idx][safe][:, vec], m[safe][:, vec]))
                failures += [(name, s, mode, int(k)) for k in idx[safe & ~ok]]
    for (s, mode), (n, out, dev) in tally.items():
        record_metric(f"volume_functions.f64_model[{build}][{s}][mode {mode}]", {"rows": n, "share_left_out": out / n, "max_rel_dev": dev})
        if out > 0.5 * n:
            failures.append((s, mode, "left out", out / n))
    assert not failures, failures[:12]


@pytest.mark.parametrize("build", ["fast", "exact"])
def test_analytic_image_through_the_renderer(build):
    """VolumeRenderer on the scene of VC.analytic_scene at the scene's default traversal: every 8 x 8 pixel block within 5 standard
    errors of the closed form (derived in VC.analytic_scene from renderer/vpt.py and checked on the oracle's loop by
    tests/test_volume_functions.py), the standard error from the closed form's own second moment."""
    from adapt_amd.renderer import VolumeRenderer
    tup, vol = VC.analytic_scene()
    rdr = VolumeRenderer(*tup, device=0, exact=(build == "exact"))
    try:
        assert rdr.arithmetic == build
        rdr.render(n_spp=VC.ANALYTIC_SPP)
        img = rdr.pixels.to_numpy()
        st = rdr.stats()
        z, expected, diff = VC.analytic_z_scores(img, rdr.rc, vol, VC.ANALYTIC_SPP)
    finally:
        rdr.close()
    record_metric(f"volume_functions.analytic_image[{build}]", {"block_z": np.round(z[..., 0], 3).tolist(), "max_abs_z": float(np.abs(z).max()),
                                                                 "max_abs_diff": float(np.abs(diff).max()), "samples": int(st["n_samples"])})
    assert st["n_samples"] == VC.ANALYTIC_W * VC.ANALYTIC_H * VC.ANALYTIC_SPP
    assert np.abs(z).max() <= VC.Z_MAX, z


@pytest.mark.parametrize("build", ["fast", "exact"])
def test_decisions_on_an_exact_boundary(build):
    """the two comparisons no random row reaches: a tentative collision at t == far_t is not accepted (rows built from the device's own
    first step, VC.far_boundary_rows), and a roulette draw equal to Tr ends the walk (streams searched for that draw, VC.roulette_boundary)"""
    const = VC.volumes()["const"]
    n = VC.check_far_boundary(lambda mode, rows, seed: _probe(build, const, mode, rows, seed))
    VC.check_roulette_boundary(lambda vol, mode, rows, seed: _probe(build, vol, mode, rows, seed))
    record_metric(f"volume_functions.exact_boundary[{build}]", {"far_t_rows": n, "roulette_streams": len(VC.ROULETTE_SEEDS)})


def test_module_wall_time():
    """not a check: the module's wall time so far goes to the metrics log, next to tests/test_gpu_product_functions.py's in the same run"""
    record_metric("volume_functions.wall_time", {"seconds": time.time() - T0})
