"""Live rows in the lean traced shade kernels (csrc/shade_stage.hpp shade_traced LIVE) on the device: every lane of a row
computes on a valid record and `alive` masks only what a dead lane must not do - vote, count, append, store.  A render under the default
(the live-row kernels) and under APT_LIVE_ROWS=0 (the kernels that give dead lanes default values) must give the same accumulation,
compared as uint32, and the same counters.  The shapes are the smallest at which the form can go wrong: partly filled last rows, sub-queues
shorter than a row or empty (lanes past the end shade the last entry's record), one and two bounces (the last bounce's continuation is
skipped at the first queue-fed launch), a roulette that ends lanes in the middle of a row (their draws are tallied apart), the throughput
cut without roulette, two lights (second index draw, per-lane emitter), a cropped render (queue-fed bounce 0), one rank of two (the
pixel-key load), every ray through the reference-order code, one lane and three."""
import copy

import pytest

from gpu_ab import assert_same_run, open_renderer, render_run

pytestmark = pytest.mark.gpu

OFF = {"APT_LIVE_ROWS": "0"}
LEAN = "lambertian/point"


def _pair(tup, w, h, spp, what, env=None, **kw):
    """the render under the default and under APT_LIVE_ROWS=0 (each with the further switches given), held to assert_same_run -> (on, off)"""
    on = render_run(tup, w, h, spp, env=dict(env or {}), **kw)
    assert on.traced and LEAN in on.variant, (what, on.variant)
    off = render_run(tup, w, h, spp, env=dict(env or {}, **OFF), **kw)
    assert_same_run(on, off, what)
    assert on.stats["n_shade"] > 0 and on.stats["n_draws"] > 0, what
    return on, off


def _with(tup, **cfg):
    *scene, prop = tup
    return (*scene, dict(prop, **cfg))


def _dark(tup, scale=0.2):
    """the scene with every albedo scaled down: the throughput falls under the roulette's threshold within a bounce or two"""
    emitters, arrays, objects, prop = tup
    objects = copy.deepcopy(objects)
    for o in objects: o.bsdf.k_d = o.bsdf.k_d * scale
    return emitters, arrays, objects, prop


def test_a_renderer_reports_the_form_it_runs(parsed):
    tup = parsed("cbox")
    for env, live in (({}, True), ({"APT_LIVE_ROWS": "1"}, True), (OFF, False)):
        with open_renderer(tup, 64, 64, env=env) as r:
            assert LEAN in r.info()["shade_variant"]
            assert r.live_rows() is live, (env, r.live_rows())
    with open_renderer(tup, 64, 64, env={"APT_FUSED": "0"}) as r:      # staged pipeline: no traced kernel, no rows to keep live
        assert r.live_rows() is False
    with open_renderer(parsed("balls_mono"), 64, 64) as r:            # another shade variant: it has no live-row form
        assert r.live_rows() is False


@pytest.mark.parametrize("film", [(61, 47, 3), (64, 48, 8)])
def test_live_rows_with_partial_short_and_empty_sub_queues(parsed, film):
    w, h, spp = film
    on, _ = _pair(parsed("cbox"), w, h, spp, f"{w}x{h}x{spp}")
    assert on.stats["n_samples"] == w * h * spp


@pytest.mark.parametrize("max_bounce", [1, 2])
def test_live_rows_where_the_last_bounce_is_the_first_launch(parsed, max_bounce):
    """max_bounce = 1: the camera-fed launch is the last bounce (with APT_CAMERA_FUSE=0: the first queue-fed one); 2: the first queue-fed launch is"""
    on, _ = _pair(parsed("cbox"), 64, 48, 8, f"max_bounce={max_bounce}", max_bounce=max_bounce)
    two, _ = _pair(parsed("cbox"), 64, 48, 8, f"max_bounce={max_bounce}, queue-fed bounce 0", env={"APT_CAMERA_FUSE": "0"}, max_bounce=max_bounce)
    assert_same_run(on, two, f"max_bounce={max_bounce}: camera-fed against queue-fed")


def test_live_rows_with_a_roulette_that_ends_lanes_mid_row(parsed):
    tup = _with(parsed("cbox"), use_rr=True, rr_bounce_th=1)
    on, _ = _pair(tup, 64, 48, 8, "roulette from bounce 1")
    dark, _ = _pair(_dark(tup), 64, 48, 8, "roulette from bounce 1, dark albedo")
    assert dark.stats["n_shade"] < on.stats["n_shade"]             # the roulette did end paths
    _pair(_with(_dark(parsed("cbox")), use_rr=True, rr_bounce_th=0, rr_threshold=2.0), 64, 48, 8, "roulette at every vertex, the camera's included")


def test_live_rows_with_the_throughput_cut_instead_of_a_roulette(parsed):
    """use_rr off: a path ends where its throughput falls under 1e-4, nothing drawn - reached within eight bounces with albedo 0.05"""
    tup = _with(_dark(parsed("cbox"), 0.05), use_rr=False)
    dark, _ = _pair(tup, 64, 48, 8, "no roulette, albedo 0.05")
    plain, _ = _pair(_with(parsed("cbox"), use_rr=False), 64, 48, 8, "no roulette")
    assert dark.stats["n_shade"] < plain.stats["n_shade"]          # the cut did end paths


def test_live_rows_with_two_point_lights(parsed):
    emitters, arrays, objects, prop = parsed("cbox")
    _pair((list(emitters) * 2, arrays, objects, prop), 64, 48, 8, "two lights")


def test_live_rows_on_a_cropped_render(parsed):
    *scene, cfg = parsed("cbox")
    tup = (*scene, dict(cfg, film={"width": 128, "height": 128, "crop_x": 70, "crop_y": 40, "crop_rx": 30, "crop_ry": 20}))
    on, _ = _pair(tup, None, None, 8, "crop")
    assert on.fused is False and on.stats["n_samples"] == 60 * 40 * 8


def test_live_rows_on_one_rank_of_two(parsed):
    on, _ = _pair(parsed("cbox"), 128, 64, 8, "rank 1 of 2", rank=1, world_size=2, band_width=4)
    assert on.accum.shape[0] == 64


def test_live_rows_with_every_ray_through_the_reference_order_code(parsed):
    on, _ = _pair(parsed("cbox"), 64, 48, 8, "defer all", env={"APT_FLAT_DEFER_ALL": "1"})
    assert on.stats["n_samples"] == 64 * 48 * 8


def test_live_rows_on_one_lane_and_on_three(parsed):
    runs = {}
    for lanes in ("1", "3"):
        runs[lanes], _ = _pair(parsed("cbox"), 96, 64, 7, f"{lanes} lanes", env={"APT_LANES": lanes}, spp_per_batch=2)
    assert_same_run(runs["1"], runs["3"], "1 lane against 3")
