"""The path-length rule of DESIGN.md §4.8 restated in numpy over the oracle's per-contribution log (oracle/binding.py CONTRIB_DTYPE),
and the cases the host and device tests of the path-length planes share."""
import numpy as np

# case id: (scene, film width, height, spp, APT_TRAVERSAL, make_config / Renderer overrides) - the scenes and overrides of
# tests/test_gpu_transient_oracle.py CASES that do not concern time, and cbox cut off after one and two bounces
CASES = {
    "cbox": ("cbox", 48, 32, 8, None, {}),
    "cbox-bvh": ("cbox", 48, 32, 8, "bvh", {}),
    "cbox-sweep": ("cbox", 48, 32, 8, "sweep", {}),
    "cbox-tile": ("cbox", 48, 32, 8, "tile", {}),
    "balls_mono": ("balls_mono", 48, 32, 8, None, {}),                      # S = 4, class-sorted group kernels
    "glass_box": ("glass_box", 48, 32, 8, None, {}),
    "features_a": ("features_a", 48, 32, 8, None, {}),
    "features_c": ("features_c", 48, 32, 8, None, {}),
    "textured": ("textured", 48, 32, 8, None, {}),
    "microfacet": ("microfacet", 48, 32, 8, None, {}),
    "bunnies_small": ("bunnies_small", 64, 48, 8, None, {}),                # the 8-wide tree
    "cbox-S2": ("cbox", 48, 32, 8, None, {"num_shadow_ray": 2}),
    "cbox-S3": ("cbox", 48, 32, 8, None, {"num_shadow_ray": 3}),
    "cbox-mb1": ("cbox", 48, 32, 8, None, {"max_bounce": 1}),
    "cbox-mb2": ("cbox", 48, 32, 8, None, {"max_bounce": 2}),
}
# the cases the rule itself was checked on (CPU): (scene, overrides), at 48 x 32 x 8 spp
HOST_CASES = {
    "cbox": ("cbox", {}),
    "cbox-mb1": ("cbox", {"max_bounce": 1}),
    "cbox-mb2-S3": ("cbox", {"max_bounce": 2, "num_shadow_ray": 3}),
    "balls_mono": ("balls_mono", {}),
    "glass_box": ("glass_box", {}),
    "features_a": ("features_a", {}),
}


def path_length_sums(records, n_pixels, max_bounce):
    """-> (sums (L, 2, n_pixels, 3) float64, counts (L, 2, n_pixels) int64) with L = max_bounce + 1 planes, plane = length - 1.
    The emitter hit of vertex b (kind 0) has length b + 1 and is part 0; light sample s of vertex b (kind 1 + s) has length b + 2 and is
    part 1.  NaN components are dropped per contribution; an all-zero contribution (after that) is neither added nor counted."""
    L = int(max_bounce) + 1
    sums, counts = np.zeros((L, 2, n_pixels, 3)), np.zeros((L, 2, n_pixels), np.int64)
    rgb = records["rgb"].astype(np.float64)
    rgb = np.where(np.isnan(rgb), 0.0, rgb)
    part = (records["kind"] > 0).astype(np.int64)
    plane = records["bounce"].astype(np.int64) + part              # length - 1
    lit = np.any(rgb != 0, axis=1)
    if lit.any():
        assert plane[lit].min() >= 0 and plane[lit].max() < L, (int(plane[lit].min()), int(plane[lit].max()), L)
    idx = (plane[lit], part[lit], records["pixel"][lit].astype(np.int64))
    np.add.at(sums, idx, rgb[lit])
    np.add.at(counts, idx, 1)
    return sums, counts
