"""The path record staged in LDS a row ahead (csrc/shade_stage.hpp shade_traced STAGE) on the device: every render whose
queue-fed shade kernel stages its record (APT_RECORD_STAGE=1, the default where the kernel has the form: Lambertian surfaces under point
lights, rays traced in place) gives the same accumulation and the same counters, bit for bit, as the kernel that loads the record where
it is used (APT_RECORD_STAGE=0).  The shapes are the smallest at which the staging can go wrong: rows that are partly filled (the clamp of
the staged address), sub-queues that are empty or shorter than a row, the bounces at which plane D is skipped and first read, a prologue
that appends before the queue's length is read, a queue-fed bounce 0, two lights, several lane-batches, one lane against three, one
rank of two."""
import pytest

from gpu_ab import assert_same_run, open_renderer, render_run, traced_pairs

pytestmark = pytest.mark.gpu

ON, OFF = {"APT_RECORD_STAGE": "1"}, {"APT_RECORD_STAGE": "0"}
LEAN = "lambertian/point"


def _pair(tup, w, h, spp, what, on_env=None, off_env=None, **kw):
    """the render under the default and under APT_RECORD_STAGE=0 (each with the further switches given), held to assert_same_run -> (on, off)"""
    on = render_run(tup, w, h, spp, env=dict(on_env or {}), **kw)
    assert on.traced and LEAN in on.variant, (what, on.variant)
    off = render_run(tup, w, h, spp, env=dict(off_env or on_env or {}, **OFF), **kw)
    assert_same_run(on, off, what)
    return on, off


def test_a_renderer_reports_the_form_it_runs(parsed):
    tup = parsed("cbox")
    for env, staged in (({}, True), (ON, True), (OFF, False)):
        with open_renderer(tup, 64, 64, env=env) as r:
            assert LEAN in r.info()["shade_variant"]
            assert r.record_staged() is staged, (env, r.record_staged())
    with open_renderer(tup, 64, 64, env={"APT_FUSED": "0"}) as r:      # staged pipeline: no traced kernel, nothing to stage
        assert r.record_staged() is False


@pytest.mark.parametrize("unsorted", [False, True])
def test_record_stage_leaves_every_traced_scene_bit_identical(parsed, unsorted):
    staged = []
    for tag, on, _ in traced_pairs(parsed, unsorted, {}, OFF):
        assert on.stats["n_extend"] > 0 and on.stats["n_shade"] > 0, tag
        if LEAN in on.variant: staged.append(tag)
    assert "cbox" in staged, staged


def test_record_stage_with_partly_filled_last_rows(parsed):
    """50 x 30 = 1500 pixels: no sub-queue's length is a multiple of 64, so every sub-queue's last row stages clamped addresses"""
    on, _ = _pair(parsed("cbox"), 50, 30, 8, "50x30")
    assert on.stats["n_samples"] == 50 * 30 * 8


def test_record_stage_with_empty_and_short_sub_queues(parsed):
    """64 rays: most sub-queues are empty (nothing may be staged) or shorter than one row"""
    on, _ = _pair(parsed("cbox"), 8, 8, 1, "8x8x1")
    assert on.stats["n_samples"] == 64


@pytest.mark.parametrize("max_bounce", [1, 2])
def test_record_stage_where_plane_d_is_skipped_and_first_read(parsed, max_bounce):
    """max_bounce = 1: only bounce 0, plane D is never staged; 2: bounce 1 stages and reads it for the first time"""
    _pair(parsed("cbox"), 64, 64, 8, f"max_bounce={max_bounce}", on_env={"APT_CAMERA_FUSE": "0"}, max_bounce=max_bounce)
    _pair(parsed("cbox"), 64, 64, 8, f"max_bounce={max_bounce}, camera-fed", max_bounce=max_bounce)


def test_record_stage_with_every_ray_through_the_reference_order_code(parsed):
    """APT_FLAT_DEFER_ALL=1: every record of a queue is appended by the launch's own prologue, before the length is read and the first row staged"""
    on, _ = _pair(parsed("cbox"), 64, 48, 8, "defer all", on_env={"APT_FLAT_DEFER_ALL": "1"})
    assert on.stats["n_samples"] == 64 * 48 * 8


def test_record_stage_with_a_queue_fed_bounce_0(parsed):
    on, off = _pair(parsed("cbox"), 64, 64, 8, "camera fuse off", on_env={"APT_CAMERA_FUSE": "0"})
    assert on.fused is False and off.fused is False


def test_record_stage_with_two_point_lights(parsed):
    emitters, arrays, objects, prop = parsed("cbox")
    _pair((list(emitters) * 2, arrays, objects, prop), 64, 64, 8, "two lights")


def test_record_stage_over_consecutive_renders(parsed):
    """three render() calls of 200 spp, each split into several lane-batches"""
    on, _ = _pair(parsed("cbox"), 96, 80, 200, "3 x 200 spp", calls=3)
    assert on.stats["n_samples"] == 96 * 80 * 600
    assert on.stats["launches"]["finalize"] >= 6


def test_record_stage_on_one_lane_and_on_three(parsed):
    runs = {}
    for lanes in ("1", "3"):
        runs[lanes], _ = _pair(parsed("cbox"), 96, 64, 7, f"{lanes} lanes", on_env={"APT_LANES": lanes}, spp_per_batch=2)
    assert_same_run(runs["1"], runs["3"], "1 lane against 3")


def test_record_stage_on_one_rank_of_two(parsed):
    on, _ = _pair(parsed("cbox"), 128, 64, 8, "rank 1 of 2", rank=1, world_size=2, band_width=4)
    assert on.accum.shape[0] == 64
