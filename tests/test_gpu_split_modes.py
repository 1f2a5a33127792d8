"""The three split renders against each other: a transient render with one bin that holds every path, a path-length
render and a light-group render walk the same records in the same order, so their framebuffers agree bit for bit, their cells hold the
same number of contributions per pixel, and each mode's cells sum to the framebuffer within that mode's own bound."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BUILDS = ["fast", "exact"]
ALL_TIME = {"sample_count": 1, "min_time": -1.0, "interval": 1e6}      # one bin that holds every path
KW = dict(width=50, height=30, spp_per_batch=3)                          # 1500 pixels: no multiple of 64; 8 spp in batches of 2 | 3, 2 | 1


@pytest.fixture
def renderer():
    """factory: Renderer(*scene, exact=..., **kw); every renderer a test makes is closed when the test ends"""
    from adapt_amd.renderer import Renderer
    made = []

    def make(scene, build, **kw):
        r = Renderer(*scene, exact=(build == "exact"), **kw)
        made.append(r)
        return r
    yield make
    for r in made:
        r.close()


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("n_light_samples", [1, 2])      # one and two radiance planes per path
@pytest.mark.parametrize("tag", ["cbox", "features_b"])
def test_three_modes_split_the_same_records(tag, n_light_samples, build, renderer, parsed):
    scene = parsed(tag)
    raw, color, stray = {}, {}, {}
    for mode, kw, tile in (("transient", {"transient": ALL_TIME}, "tile_transient"), ("lengths", {"path_lengths": True}, "tile_path_lengths"),
                           ("lights", {"light_groups": True}, "tile_light_groups")):
        r = renderer(scene, build, num_shadow_ray=n_light_samples, **kw, **KW)
        for n in (2, 5, 1):
            r.render(n_spp=n)
        cells = getattr(r, tile)().astype(np.float64)
        raw[mode] = cells.reshape(-1, 50, 30, 4)          # every cell of a pixel, whatever the mode's leading axes
        color[mode] = r.color.to_numpy()
        stray[mode] = r.stats()["n_stray_light"]
    assert stray == {"transient": 0, "lengths": 0, "lights": 0}
    assert np.array_equal(color["transient"], color["lengths"], equal_nan=True)
    assert np.array_equal(color["transient"], color["lights"], equal_nan=True)
    counts = {mode: cells[..., 3].sum(0) for mode, cells in raw.items()}
    for c in counts.values():
        assert np.array_equal(c, np.round(c))
    assert np.array_equal(counts["transient"].astype(np.int64), counts["lengths"].astype(np.int64))
    assert np.array_equal(counts["transient"].astype(np.int64), counts["lights"].astype(np.int64))
    assert counts["transient"].sum() > 0
    # each mode's cells against its framebuffer, with the bound of the mode's own test file (test_gpu_transient.py
    # test_bins_sum_to_steady_image; test_gpu_path_lengths.py and test_gpu_light_groups.py test_planes_sum_to_the_image)
    c = color["transient"].astype(np.float64)
    fin = np.isfinite(c).all(axis=2)
    a = raw["transient"][0, ..., :3]
    assert np.all(np.abs(c - a)[fin] <= 1e-5 * np.abs(a)[fin] + 1e-12)
    for mode in ("lengths", "lights"):
        a, mag = raw[mode][..., :3].sum(0), np.abs(raw[mode][..., :3]).sum(0)
        assert np.all(np.abs(a - c)[fin] <= 1e-5 * mag[fin] + 1e-12), mode
