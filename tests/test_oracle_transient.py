"""The oracle's per-contribution log (pt_oracle.c orc_render_contributions) and the float32 binning rule of the transient renderer
 restated in numpy (oracle/binding.py transient_bins).  CPU only: these are the references
tests/test_gpu_transient_oracle.py holds the device's bins to, so they are pinned here against the steady oracle, against float64
path lengths and against analytic arrival times."""
import numpy as np
import pytest

from adapt_amd.scene_pack import make_config, pack_scene
from oracle import binding as ob

U32 = 2.0 ** -24                 # float32 unit roundoff
LOG_TAGS = ["cbox", "balls_mono", "glass_box", "features_a", "features_c", "textured", "microfacet"]


@pytest.fixture(scope="module")
def logs(parsed, oracle_scene):
    cache = {}

    def get(tag, w=40, h=24, spp=4):
        key = (tag, w, h, spp)
        if key not in cache:
            rc = make_config(parsed(tag)[3], width=w, height=h)
            sc = oracle_scene(tag)
            cache[key] = (rc, sc, *sc.contributions(rc, spp))
        return cache[key]
    return get


@pytest.mark.parametrize("tag", LOG_TAGS)
def test_log_adds_up_to_the_steady_render(tag, logs):
    rc, sc, recs, per, st = logs(tag)
    spp = per.shape[2]
    acc, cnt, ost = sc.render(rc, spp)
    # the same samples on the same stream: the per-sample colours add up to orc_render's accumulation bit for bit, with the same statistics
    run = np.zeros_like(acc)
    for s in range(spp):
        run += per[:, :, s, :3]
    assert np.array_equal(run, acc, equal_nan=True) and st == ost
    # sorted by pixel, sample, bounce, kind; kinds are the emitter hit (0) and the light samples 1 .. S
    key = np.stack([recs["pixel"], recs["sample"], recs["bounce"], recs["kind"]])
    order = np.lexsort(key[::-1])
    assert np.array_equal(order, np.arange(len(recs)))
    assert not np.any((np.diff(recs["pixel"]) == 0) & (np.diff(recs["sample"]) == 0) & (np.diff(recs["bounce"]) == 0) & (np.diff(recs["kind"]) == 0))
    assert recs["kind"].min() >= 0 and recs["kind"].max() <= rc.num_shadow_ray and recs["bounce"].max() < rc.max_bounce
    assert np.all(recs["sample"] >= 1) and np.all(recs["sample"] <= spp)
    rgb = recs["rgb"].astype(np.float64)
    assert not np.isnan(rgb).any() and np.all(np.any(rgb != 0, axis=1))      # NaN components zeroed, all-zero records left out
    # per pixel-sample: the records sum to the sample's colour up to float32 summation order (relative to the sum of |terms|), except the
    # pixel-samples whose colour is NaN - a NaN MIS weight, or a throughput that turned NaN - which the steady renderer drops whole (their
    # colour is 0) and the log only loses the NaN terms of
    slot = recs["pixel"].astype(np.int64) * spp + (recs["sample"] - 1)
    n_slots = rc.width * rc.height * spp
    tot, mag = np.zeros((n_slots, 3)), np.zeros((n_slots, 3))
    fin = np.isfinite(rgb).all(axis=1)
    np.add.at(tot, slot[fin], rgb[fin])
    np.add.at(mag, slot[fin], np.abs(rgb[fin]))
    inf_slot = np.zeros(n_slots, bool)
    inf_slot[slot[~fin]] = True
    col = per[..., :3].reshape(n_slots, 3).astype(np.float64)
    poisoned, dropped = per[..., 3].reshape(n_slots) > 0, per[..., 4].reshape(n_slots) > 0
    ok = ~dropped & ~inf_slot
    assert np.all(np.abs(tot[ok] - col[ok]) <= 1e-6 * mag[ok] + 1e-30)
    assert np.all(col[dropped] == 0) and np.all(dropped[poisoned])
    assert np.array_equal(inf_slot & ~dropped, ~np.isfinite(col).all(axis=1) & ~dropped)      # a sample is infinite where one of its terms is
    assert dropped.mean() <= 0.05, dropped.mean()                     # measured: at most 2.9 % (microfacet), none on cbox
    if tag == "cbox":
        assert not dropped.any()


def test_log_does_not_depend_on_the_thread_count(parsed, oracle_scene):
    rc = make_config(parsed("balls_mono")[3], width=40, height=24)
    a = oracle_scene("balls_mono").contributions(rc, 3, threads=1)
    b = oracle_scene("balls_mono").contributions(rc, 3, threads=5)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1], equal_nan=True) and a[2] == b[2]


@pytest.mark.parametrize("tag", LOG_TAGS)
def test_float32_time_tracks_the_float64_path_length(tag, logs):
    """|t32 - t64| <= 8 u (t_scale) + t_dir for every record.  t_scale sums, per segment, ior x (its length + the largest coordinate
    of each end): t32 adds min_depth * ior per segment (two roundings) and min_depth is the distance from one float32 vertex to the next,
    o + d * t, rounded relative to those coordinates (measured: at most 1.0 u t_scale on these scenes, so the factor 8 is the margin).
    t_dir is not rounding: the device - as upstream (bdpt.py:253) - measures a segment by its ray parameter, and a sampled direction is
    unit only to the frames' accuracy, ||d| - 1| up to 4.5e-5 here and up to ~7 % behind a normal map (textured)."""
    rc, sc, recs, per, st = logs(tag)
    err = np.abs(recs["t32"].astype(np.float64) - recs["t64"])
    assert np.all(err <= 8 * U32 * recs["t_scale"] + recs["t_dir"])
    assert np.all(recs["t_scale"] <= 10 * recs["t64"])               # the bound is a few ulp of the time, not a free pass
    if tag != "textured":
        assert np.all(recs["t_dir"] <= 5e-5 * recs["t64"])
    # times grow along a path: a vertex's light samples leave after it
    assert np.all(recs["t32"] > 0) and np.all(recs["t64"] > 0)


@pytest.mark.parametrize("slab", [False, True])
def test_direct_light_times_match_the_analytic_path(slab):
    """_direct_light_scene (tests/transient_cases.py): t64 of the light sample on the diffuse plane is the analytic optical length, the
    slab's in-glass segment weighted by its ior 1.5.  The analytic path uses exact ray directions, the oracle float32 ones: the two
    differ at float32 rounding of the camera ray (measured 2.1e-7 relative; the slab's ior moves the time by 0.5 x 5 / 23 ~ 1e-1)."""
    from transient_cases import _direct_light_scene, _predicted_times
    w = h = 32
    scene = _direct_light_scene(w, h, slab)
    rc = make_config(scene[3], width=w, height=h)
    sc = ob.OracleScene(pack_scene(*scene), rc.cam_t)
    recs, per, st = sc.contributions(rc, 2)
    plane = 2 if slab else 0                                         # the vertex on the plane: after the slab's two faces
    r = recs[(recs["bounce"] == plane) & (recs["kind"] == 1)]
    assert len(r) >= 0.9 * w * h * 2 and np.all(np.isin(recs["kind"], [1]))
    t_ior, t_geo = _predicted_times(rc, (2.78, 2.73, 6.0), slab)
    pred = t_ior[r["pixel"] // h, r["pixel"] % h]
    assert np.all(np.abs(r["t64"] - pred) <= 1e-6 * pred)
    assert np.all(np.abs(r["t32"] - pred) <= 1e-6 * pred)
    if slab:
        geo = t_geo[r["pixel"] // h, r["pixel"] % h]
        assert np.all(r["t64"] - geo > 1.0)                         # 0.5 x the in-slab length (>= 2.5)


# ---------------------------------------------------------------- the binning rule
def _q(x):
    return np.float32(x)


def test_binning_edges_on_hand_picked_times():
    lo, step, n = _q(2.5), _q(0.25), 8
    top = ob.transient_max_time(lo, step, n)
    assert top == _q(4.5)
    inf = np.float32(np.inf)
    t = np.float32([lo, np.nextafter(lo, inf), _q(2.75), np.nextafter(_q(2.75), -inf), top, np.nextafter(top, -inf),
                    np.nan, np.inf, -np.inf, _q(-1.0), _q(100.0)])
    want = [-1, 0, 1, 0, -1, n - 1, -1, -1, -1, -1, -1]
    assert ob.transient_bin_index(t, lo, step, n).tolist() == want
    # max_time is min_time + interval * n in double, rounded once: here the float32 product and sum would give another float
    lo, step, n = _q(-7.1), _q(0.013), 400
    assert ob.transient_max_time(lo, step, n) == np.float32(float(lo) + float(step) * n)
    assert ob.transient_max_time(lo, step, n) != np.float32(lo + np.float32(step * np.float32(n)))


def test_a_quotient_that_rounds_up_stays_in_the_last_bin():
    from transient_cases import _rounding_up_window
    lo, step, n, t = _rounding_up_window()
    assert lo < t < ob.transient_max_time(lo, step, n) and (t - lo) / step == np.float32(n)
    assert ob.transient_bin_index([t], lo, step, n).tolist() == [n - 1]


def test_transient_bins_sums_counts_and_near_edge_records():
    recs = np.zeros(6, ob.CONTRIB_DTYPE)
    recs["pixel"] = [0, 0, 1, 1, 1, 2]
    recs["rgb"] = [[1, 2, 3], [1, 1, 1], [4, 0, 0], [0, 5, 0], [9, 9, 9], [7, 7, 7]]
    recs["t32"] = [1.1, 1.9, 2.0, 2.0000002, 0.5, np.nan]
    recs["t64"] = [1.1, 1.9, 2.0, 2.0000002, 0.5, 1.5]
    sums, counts, near_cnt, near_e = ob.transient_bins(recs, 3, 1.0, 0.5, 4)
    assert counts.tolist() == [[1, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 0]]
    assert sums[0, 0].tolist() == [1, 2, 3] and sums[2, 1].tolist() == [4, 5, 0] and sums.sum() == 6 + 3 + 9
    # edge 2 (t = 2.0) has both of pixel 1's records within 2e-5 t of it; a NaN t32 is in no bin and near no edge (whatever its t64)
    assert near_cnt[2].tolist() == [0, 2, 0] and near_cnt.sum() == 2 and near_e[2, 1].tolist() == [4, 5, 0]
