"""Feature buffers (albedo, normal, depth) on the device, both builds unless a case says otherwise: against the oracle
ray by ray with anti-aliasing off, against the render's own rays with it on, the bookkeeping around them, and the render path they must
leave untouched."""
import numpy as np
import pytest

import aov_cases as ac
from conftest import record_metric

pytestmark = pytest.mark.gpu

BUILDS = ["fast", "exact"]
_reference = {}


@pytest.fixture
def renderer():
    """factory: Renderer(*scene, exact=..., **kw); every renderer a test makes is closed when the test ends"""
    from adapt_amd import renderer as rmod
    made = []

    def make(scene, build, cls="Renderer", **kw):
        r = getattr(rmod, cls)(*scene, exact=(build == "exact"), **kw)
        made.append(r)
        return r
    yield make
    for r in made:
        r.close()


def _centre_reference(name, film, parsed):
    """the oracle's answer for the rays through the pixel centres of `film`, computed once per scene and film and left unchanged"""
    key = (name, film)
    if key not in _reference:
        scene = ac.scene_of(name, parsed, anti_alias=False)
        osc, rc, fs = ac.oracle_of(scene, *film)
        d = ac.centre_rays(osc, rc)
        o = np.tile(np.float32(rc.cam_t), (len(d), 1))
        _reference[key] = (scene, fs, osc, o, d, ac.oracle_aov(osc, fs, rc, d))
    return _reference[key]


# ---------------------------------------------------------------- 3. against the oracle, rays through the pixel centres
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("film", ac.FILMS, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("case", list(ac.CASES))
def test_aov_matches_the_oracle_ray_by_ray(case, film, build, renderer, parsed, monkeypatch):
    """Exact build: depth sums, hit counts, albedo and normal sums bit for bit (two samples through the same centre: twice the oracle's
    value, exactly).  Product build: the hit distance within 1e-5 relative and the oracle's primitive, except on rays
    where the device's primitive is another candidate within 1e-5 of the oracle's best: those are counted and capped at 0.1 % of the
    rays.  (A device distance there may sit 1e-5 from either candidate: 2e-5 from the oracle's.)"""
    name, traversal = ac.CASES[case]
    if traversal:
        monkeypatch.setenv("APT_TRAVERSAL", traversal)
    w, h = film
    scene, fs, osc, o, d, (hit, prim, t, kd, ns) = _centre_reference(name, film, parsed)
    r = renderer(scene, build, width=w, height=h)
    if traversal:
        assert r.info()["traversal"] == traversal
    elif name == "bunnies1":
        assert r.info()["traversal"] == "bvh"
    r.render(n_spp=2)
    raw = r.tile_aov().reshape(-1, 8)
    two = np.float32(2)
    assert np.array_equal(raw[:, 7] > 0, raw[:, 7] == two)
    if build == "exact":
        assert np.array_equal(raw[:, 7], two * hit)
        assert np.array_equal(raw[:, 3], two * t)
        assert np.array_equal(raw[:, 0:3], two * kd)
        assert np.array_equal(raw[:, 4:7], two * ns)
        return
    # the pass traces with the renderer's own traversal: what apt_intersect finds for the same rays, to the bit
    prim_d, t_d, uv_d = r.intersect(o, d)
    got_hit = raw[:, 7] > 0
    assert np.array_equal(got_hit, prim_d >= 0)
    assert np.array_equal(raw[got_hit, 3], two * t_d[got_hit])
    # ... and opens the vertex as the shade stage does: the oracle's vertex at the device's own primitive and barycentrics (meshes), the
    # material's colour and the normal through the device's own hit point (spheres).  1e-5 (1 + |x|): float32 rounding over the few dozen
    # operations of the maps, the product build's v_rsq among them.
    info = np.int32(fs.obj_info).reshape(-1, 3)
    prim_obj, prim_sphere = np.zeros(fs.n_prims, np.int32), np.zeros(fs.n_prims, bool)
    for k, (first, count, kind) in enumerate(info):
        prim_obj[first:first + count], prim_sphere[first:first + count] = k, kind != 0
    want_kd, want_ns = np.zeros((len(d), 3)), np.zeros((len(d), 3))
    mesh = got_hit & ~prim_sphere[np.maximum(prim_d, 0)]
    ball = got_hit & ~mesh
    if mesh.any():
        want_kd[mesh], want_ns[mesh], _ = osc.surface_maps(prim_d[mesh], uv_d[mesh], True)
    if ball.any():
        want_kd[ball] = np.float32(fs.bxdf_f).reshape(-1, 13)[prim_obj[prim_d[ball]], 0:3]
        n = (np.float64(o[ball]) + np.float64(d[ball]) * np.float64(t_d[ball])[:, None]) - np.float64(fs.prims).reshape(-1, 9)[prim_d[ball], 0:3]
        want_ns[ball] = n / np.linalg.norm(n, axis=1, keepdims=True)
    err_kd = np.abs(raw[:, 0:3] / two - want_kd) / (1 + np.abs(want_kd)); err_ns = np.abs(raw[:, 4:7] / two - want_ns) / (1 + np.abs(want_ns))
    assert err_kd.max() <= 1e-5 and err_ns.max() <= 1e-5, (float(err_kd.max()), float(err_ns.max()))
    # against the oracle: the distance within 1e-5 relative and the same primitive ...
    both = hit & got_hit
    rel = np.abs(t_d[both].astype(np.float64) - t[both]) / t[both]
    other = (hit != got_hit) | (both & (prim_d != prim))
    other[both] |= rel > 1e-5
    # ... except where the device's primitive is another candidate within 1e-5 of the oracle's best
    cand = ac.candidate_distances(fs, o[other], d[other]) if other.any() else np.zeros((0, 1))
    explained = np.zeros(int(other.sum()), bool)
    for k, ray in enumerate(np.flatnonzero(other)):
        if hit[ray] and got_hit[ray]:
            near = np.abs(cand[k] - float(t[ray])) <= 1e-5 * float(t[ray])
            explained[k] = near.sum() >= 2 and near[prim_d[ray]] and abs(float(t_d[ray]) - float(t[ray])) <= 2e-5 * float(t[ray])
    record_metric(f"aov_vs_oracle[{case},{w}x{h},{build}]", {"rays": len(hit), "hits": int(hit.sum()), "max_rel_t": float(rel.max()) if len(rel) else 0.0,
                                                             "other": int(other.sum()), "explained": int(explained.sum()),
                                                             "max_err_albedo": float(err_kd.max()), "max_err_normal": float(err_ns.max())})
    assert explained.all(), (int(other.sum()), int(explained.sum()), np.flatnonzero(other)[:5])
    assert other.sum() <= ac.TIE_CAP * len(hit)


# ---------------------------------------------------------------- 4. the render's own rays (anti-aliasing on)
@pytest.mark.parametrize("name", ["cbox", "balls_mono"])
def test_aov_sums_the_first_hits_of_the_renders_own_rays(name, renderer, parsed):
    """Exact build, 8 jittered samples: per pixel, the depth sum and the hit count are the float32 in-order sums of event 0 of
    OracleScene.trace_sample(rc, i, j, s), s = 1..8 - the camera rays the render traced (tests/test_aov_host.py: event 0 is the camera
    ray's hit, and a sample without one logs nothing)."""
    w, h, spp = 64, 48, 8
    scene = ac.scene_of(name, parsed, anti_alias=True)
    osc, rc, _ = ac.oracle_of(scene, w, h)
    r = renderer(scene, "exact", width=w, height=h)
    r.render(n_spp=spp)
    raw = r.tile_aov()
    depth, count = np.zeros((w, h), np.float32), np.zeros((w, h), np.float32)
    for i in range(w):
        for j in range(h):
            for s in range(1, spp + 1):
                _, ev, _ = osc.trace_sample(rc, i, j, s, max_events=1)
                if len(ev):
                    depth[i, j] = depth[i, j] + ev[0, 2]
                    count[i, j] = count[i, j] + np.float32(1)
    assert np.array_equal(raw[..., 7], count)
    assert np.array_equal(raw[..., 3], depth)
    a = r.aov()
    assert np.array_equal(a["hit_fraction"], count / np.float32(spp))
    n = np.linalg.norm(a["normal"].astype(np.float64), axis=-1)
    assert np.all(np.abs(n[count > 0] - 1) <= 1e-6) and np.all(n[count == 0] == 0)


# ---------------------------------------------------------------- 5. bookkeeping
@pytest.mark.parametrize("build", BUILDS)
def test_aov_top_up_limit_clear_and_checkpoint(build, renderer, parsed):
    scene = parsed("cbox")
    kw = dict(width=50, height=30)
    whole = renderer(scene, build, **kw)
    whole.render(n_spp=8)
    ref = whole.tile_aov()
    assert ref[..., 7].max() == 8
    parts = renderer(scene, build, **kw)
    parts.render(n_spp=5)
    five = parts.tile_aov()
    assert five[..., 7].max() == 5
    parts.render(n_spp=3)
    assert np.array_equal(parts.tile_aov(), ref)                       # topped up after more rendering: the same bits as in one go
    assert np.array_equal(whole.tile_aov(), ref)                       # asked again: nothing is added twice
    a, b = whole.aov(), parts.aov()
    assert set(a) == {"albedo", "normal", "depth", "hit_fraction"} and all(np.array_equal(a[k], b[k]) for k in a)
    assert a["albedo"].shape == (50, 30, 3) and a["normal"].shape == (50, 30, 3) and a["depth"].shape == (50, 30) and a["hit_fraction"].shape == (50, 30)
    # aov_spp = 4 stops at 4
    capped = renderer(scene, build, aov_spp=4, **kw)
    capped.render(n_spp=8)
    four = capped.tile_aov()
    assert four[..., 7].max() == 4 and capped.aov()["hit_fraction"].max() == 1.0
    early = renderer(scene, build, **kw)
    early.render(n_spp=4)
    assert np.array_equal(early.tile_aov(), four)
    # checkpoint round trip: the buffers travel, and a checkpoint without them still loads (the buffers are then restated)
    chk = parts.get_check_point()
    assert chk["aov_samples"] == 8 and np.array_equal(chk["aov_sums"], ref)
    fresh = renderer(scene, build, **kw)
    fresh.load_check_point(chk)
    assert fresh._aov_n == 8 and np.array_equal(fresh.tile_aov(), ref) and np.array_equal(fresh.color.to_numpy(), parts.color.to_numpy())
    old = {k: v for k, v in chk.items() if not k.startswith("aov_")}
    fresh.load_check_point(old)
    assert fresh._aov_n == 0 and np.array_equal(fresh.tile_aov(), ref)
    plain = renderer(scene, build, **kw)
    plain.render(n_spp=2)
    assert "aov_sums" not in plain.get_check_point()                   # a renderer that never asked for them writes today's checkpoint
    # clear()
    parts.clear()
    assert parts._aov_n == 0 and not parts.tile_aov().any()
    parts.render(n_spp=8)
    assert np.array_equal(parts.tile_aov(), ref)
    parts.reset()
    assert parts._aov_n == 0 and np.array_equal(parts.tile_aov(), ref) and np.array_equal(parts.color.to_numpy(), whole.color.to_numpy())


@pytest.mark.parametrize("build", BUILDS)
def test_aov_of_a_crop_window(build, renderer, parsed):
    em, arr, objs, prop = parsed("cbox")
    full = renderer((em, arr, objs, prop), build, width=64, height=48)
    full.render(n_spp=4)
    crop_prop = dict(prop); crop_prop["film"] = {"width": 64, "height": 48, "crop_x": 30, "crop_y": 20, "crop_rx": 11, "crop_ry": 7}
    crop = renderer((em, arr, objs, crop_prop), build)
    assert crop.do_crop and (crop.w, crop.h) == (64, 48)
    crop.render(n_spp=4)
    a, b = full.tile_aov(), crop.tile_aov()
    inside = np.zeros((64, 48), bool); inside[crop.start_x:crop.end_x, crop.start_y:crop.end_y] = True
    assert 0 < inside.sum() < inside.size
    assert not b[~inside].any()
    assert np.array_equal(b[inside], a[inside])


@pytest.mark.parametrize("build", BUILDS)
def test_aov_and_denoiser_refuse_the_volumetric_tracer_and_ranks(build, renderer, parsed):
    from adapt_amd._lib import AptError
    vol = renderer(parsed("cbox"), build, cls="VolumeRenderer", width=32, height=32)
    vol.render(n_spp=1)
    ranked = renderer(parsed("cbox"), build, width=32, height=32, rank=1, world_size=2)
    for r, word in ((vol, "volumetric = 0"), (ranked, "world_size = 1")):
        for call in (r.aov, r.denoised, r.firefly_filtered):
            with pytest.raises(AptError, match=word):
                call()
        r.clear()                                                      # ... and nothing else about them changed


# ---------------------------------------------------------------- 8. the render path is untouched
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", ["cbox", "balls_mono"])      # the traced pipeline (product build) | the class groups
def test_render_is_the_same_after_aov_and_denoise(name, build, renderer, parsed):
    kw = dict(width=64, height=48, spp_per_batch=4)
    plain = renderer(parsed(name), build, **kw)
    plain.render(n_spp=8); plain.render(n_spp=8)
    used = renderer(parsed(name), build, **kw)
    used.render(n_spp=8)
    used.aov(); used.denoised(); used.firefly_filtered()
    used.render(n_spp=8)
    assert np.array_equal(used.color.to_numpy(), plain.color.to_numpy(), equal_nan=True)
    a, b = used.stats(), plain.stats()
    for k in a:
        if k not in ("kernel_ms", "render_ms"):
            assert a[k] == b[k], (k, a[k], b[k])
