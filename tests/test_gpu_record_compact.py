"""The 56-byte path record of the lean traced kernels (csrc/stages.hpp TrRecord, csrc/shade_stage.hpp shade_traced C56) on
the device: the record carries the vertex's hit point, made by the kernel that appends it, instead of the ray's origin and hit distance,
and no pdf.  A render under the default (the 56-byte kernels) and under APT_RECORD_COMPACT=0 (the 64-byte record) must give the same
accumulation, compared as uint32, and the same counters.  The shapes are the smallest at which each writer or reader of a record can go
wrong: partly filled last rows, short and empty sub-queues; one and two bounces, camera-fed and queue-fed bounce 0 (the camera-fed kernel as
the only writer, k_generate_trace56 as writer, a last bounce that writes nothing); every ray through the staging area and the prologue,
where a staged ray's origin becomes the resolved record's hit point; the three queue-fed and both camera-fed forms; two lights; a
roulette and the throughput cut; a cropped and an adaptive render (k_generate_trace56 and its adaptive sibling), one rank of two; one lane
and three over several render() calls; the capacity scenes - spheres, whose normal comes from the carried point, coplanar groups, 96 records."""
import pytest

from flat_cases import capacity
from gpu_ab import assert_same_run, open_renderer, run_of
from test_gpu_live_rows import _dark, _with

pytestmark = pytest.mark.gpu

OFF = {"APT_RECORD_COMPACT": "0"}
LEAN = "lambertian/point"


def _run(tup, w, h, spp, env, **kw):
    """-> Run, record_compact() of the renderer that made it"""
    calls = kw.pop("calls", 1)
    with open_renderer(tup, w, h, env=env, **kw) as r:
        return run_of(r, spp, calls), r.record_compact()


def _pair(tup, w, h, spp, what, env=None, **kw):
    """the render under the default and under APT_RECORD_COMPACT=0 (each with the further switches given), held to assert_same_run -> (on, off)"""
    on, compact = _run(tup, w, h, spp, dict(env or {}), **dict(kw))
    assert compact is True and on.traced and LEAN in on.variant, (what, compact, on.variant)
    off, compact_off = _run(tup, w, h, spp, dict(env or {}, **OFF), **dict(kw))
    assert compact_off is False, what
    assert_same_run(on, off, what)
    assert on.stats["n_shade"] > 0 and on.stats["n_draws"] > 0, what
    return on, off


def test_a_renderer_reports_the_record_it_carries(parsed):
    tup = parsed("cbox")
    for env, compact in (({}, True), ({"APT_RECORD_COMPACT": "1"}, True), (OFF, False)):
        with open_renderer(tup, 64, 64, env=env) as r:
            assert LEAN in r.info()["shade_variant"]
            assert r.record_compact() is compact, (env, r.record_compact())
    with open_renderer(tup, 64, 64, env={"APT_FUSED": "0"}) as r:      # staged pipeline: no traced kernel, no path record
        assert r.record_compact() is False
    with open_renderer(parsed("balls_mono"), 64, 64) as r:            # another shade variant
        assert r.record_compact() is False
    with open_renderer(parsed("glass_box"), 64, 64, unsorted=True) as r:      # an area light: the plain traced kernel reads origin, distance and pdf
        assert "[rays traced in place]" in r.info()["shade_variant"] and LEAN not in r.info()["shade_variant"], r.info()["shade_variant"]
        assert r.record_compact() is False


@pytest.mark.parametrize("film", [(61, 47, 3), (64, 48, 8)])
def test_compact_record_with_partial_short_and_empty_sub_queues(parsed, film):
    w, h, spp = film
    on, _ = _pair(parsed("cbox"), w, h, spp, f"{w}x{h}x{spp}")
    assert on.stats["n_samples"] == w * h * spp


@pytest.mark.parametrize("max_bounce", [1, 2])
def test_compact_record_where_the_last_bounce_is_the_first_launch(parsed, max_bounce):
    """max_bounce = 1: the camera-fed launch writes staged rays only, the queue-fed one nothing; 2: the camera-fed kernel is the only writer
    of resolved records.  With APT_CAMERA_FUSE=0 k_generate_trace56 writes them."""
    on, _ = _pair(parsed("cbox"), 64, 48, 8, f"max_bounce={max_bounce}", max_bounce=max_bounce)
    two, _ = _pair(parsed("cbox"), 64, 48, 8, f"max_bounce={max_bounce}, queue-fed bounce 0", env={"APT_CAMERA_FUSE": "0"}, max_bounce=max_bounce)
    assert_same_run(on, two, f"max_bounce={max_bounce}: camera-fed against queue-fed")


@pytest.mark.parametrize("env", [{}, {"APT_CAMERA_FUSE": "0"}], ids=["fused", "two-launch"])
def test_compact_record_with_every_ray_through_the_reference_order_code(parsed, env):
    """every record goes through the staging area and the prologue: origin in, hit point out"""
    on, _ = _pair(parsed("cbox"), 64, 48, 8, f"defer all {env}", env=dict(env, APT_FLAT_DEFER_ALL="1"))
    assert on.stats["n_samples"] == 64 * 48 * 8
    plain, _ = _run(parsed("cbox"), 64, 48, 8, dict(env))
    assert plain.stats["n_samples"] == on.stats["n_samples"]


@pytest.mark.parametrize("env", [{"APT_RECORD_STAGE": "0"}, {"APT_LIVE_ROWS": "0"}, {"APT_RECORD_STAGE": "0", "APT_LIVE_ROWS": "0"}], ids=["direct", "staged", "direct,no-live-cam"])
def test_compact_record_in_every_queue_fed_and_camera_fed_form(parsed, env):
    _pair(parsed("cbox"), 64, 48, 8, str(env), env=env)


def test_compact_record_with_two_point_lights(parsed):
    emitters, arrays, objects, prop = parsed("cbox")
    _pair((list(emitters) * 2, arrays, objects, prop), 64, 48, 8, "two lights")


def test_compact_record_with_a_roulette_and_with_the_throughput_cut(parsed):
    tup = _with(parsed("cbox"), use_rr=True, rr_bounce_th=1)
    on, _ = _pair(tup, 64, 48, 8, "roulette from bounce 1")
    dark, _ = _pair(_dark(tup), 64, 48, 8, "roulette from bounce 1, dark albedo")
    assert dark.stats["n_shade"] < on.stats["n_shade"]             # the roulette did end paths
    cut, _ = _pair(_with(_dark(parsed("cbox"), 0.05), use_rr=False), 64, 48, 8, "no roulette, albedo 0.05")
    plain, _ = _pair(_with(parsed("cbox"), use_rr=False), 64, 48, 8, "no roulette")
    assert cut.stats["n_shade"] < plain.stats["n_shade"]           # the cut did end paths


def test_compact_record_on_a_cropped_render(parsed):
    *scene, cfg = parsed("cbox")
    tup = (*scene, dict(cfg, film={"width": 128, "height": 128, "crop_x": 70, "crop_y": 40, "crop_rx": 30, "crop_ry": 20}))
    on, _ = _pair(tup, None, None, 8, "crop")
    assert on.fused is False and on.stats["n_samples"] == 60 * 40 * 8


def test_compact_record_on_an_adaptive_render(parsed):
    ad = {"threshold": 0.05, "min_spp": 8, "step": 4}
    on, _ = _pair(parsed("cbox"), 64, 64, 12, "adaptive", calls=4, adaptive=ad)
    assert "[adaptive]" in on.variant and on.fused is False


def test_compact_record_on_one_rank_of_two(parsed):
    on, _ = _pair(parsed("cbox"), 128, 64, 8, "rank 1 of 2", rank=1, world_size=2, band_width=4)
    assert on.accum.shape[0] == 64


def test_compact_record_on_one_lane_and_on_three(parsed):
    runs = {}
    for lanes in ("1", "3"):
        runs[lanes], _ = _pair(parsed("cbox"), 96, 64, 7, f"{lanes} lanes", env={"APT_LANES": lanes}, spp_per_batch=2, calls=3)
    assert_same_run(runs["1"], runs["3"], "1 lane against 3")


@pytest.mark.parametrize("name", ["capacity_mixed", "capacity_tris"])
def test_compact_record_on_the_capacity_scenes(name):
    """spheres (the normal from the carried point), coplanar groups (runner-ups staged on their own), 96 records"""
    tup, _ = capacity(name, "lean")
    on, _ = _pair(tup, 48, 40, 8, name)
    assert on.stats["n_samples"] == 48 * 40 * 8 and 0 < on.stats["n_lit"] < on.stats["n_shadow"]
