"""The light-group rule of DESIGN.md §4.9 restated over the oracle's per-contribution log (oracle/binding.py CONTRIB_DTYPE), and the cases
the host and device tests of the light-group planes share.

The oracle picks an emitter, samples it and plays Russian roulette on throughput alone: nothing on a path but the final product reads an
emitter's intensity.  So the log of the scene with every emitter but k at zero intensity - `single_lit(fs, k)` - is exactly emitter k's
share of the full log (tests/test_light_groups_host.py pins that), and the E single-lit logs are the reference the planes are held to."""
import dataclasses

import numpy as np

# case id: (scene, film width, height, spp, environment, make_config / Renderer overrides)
CASES = {
    "features_b": ("features_b", 48, 32, 8, {}, {}),                               # class-sorted group twins, every emitter type
    "features_a": ("features_a", 48, 32, 8, {}, {}),                               # S = 2
    "features_b-S4": ("features_b", 48, 32, 8, {}, {"num_shadow_ray": 4}),
    "features_b-unsorted": ("features_b", 48, 32, 8, {"APT_SORTED": "0"}, {}),     # the unsorted twin
    "features_b-bvh": ("features_b", 48, 32, 8, {"APT_TRAVERSAL": "bvh"}, {}),
    "textured": ("textured", 48, 32, 8, {}, {}),                                   # the textured twin
    "microfacet": ("microfacet", 48, 32, 8, {}, {}),
    "cbox": ("cbox", 48, 32, 8, {}, {}),                                           # one emitter: the planes are the whole render
}
# the cases the premise is pinned on (CPU): (scene, overrides), at 48 x 32 x 8 spp
HOST_CASES = {
    "features_a": ("features_a", {}),
    "features_b": ("features_b", {}),
    "features_b-S4": ("features_b", {"num_shadow_ray": 4}),
    "textured": ("textured", {}),
    "microfacet": ("microfacet", {}),
}


def single_lit(fs, k):
    """a copy of the FlatScene with every emitter but k at zero intensity"""
    src_f = np.array(fs.src_f, np.float32, copy=True)
    src_f[np.arange(src_f.shape[0]) != k, :3] = 0
    return dataclasses.replace(fs, src_f=src_f)


def scaled_lights(fs, gains):
    """a copy of the FlatScene with emitter e's intensity multiplied by gains[e] (rgb), in float32 as the scene stores it"""
    src_f = np.array(fs.src_f, np.float32, copy=True)
    src_f[:, :3] *= np.asarray(gains, np.float32).reshape(src_f.shape[0], -1)
    return dataclasses.replace(fs, src_f=src_f)


def light_group_sums(logs, n_pixels):
    """logs: the E single-lit logs, emitters in scene order -> (sums (E, 2, n_pixels, 3) float64, counts (E, 2, n_pixels) int64).
    Part 0: the emitter hit of a vertex (kind 0), part 1: a light sample (kind 1 + s).  NaN components are dropped per contribution; an
    all-zero contribution (after that) is neither added nor counted - path_length_sums' rule."""
    E = len(logs)
    sums, counts = np.zeros((E, 2, n_pixels, 3)), np.zeros((E, 2, n_pixels), np.int64)
    for e, records in enumerate(logs):
        rgb = records["rgb"].astype(np.float64)
        rgb = np.where(np.isnan(rgb), 0.0, rgb)
        part = (records["kind"] > 0).astype(np.int64)
        lit = np.any(rgb != 0, axis=1)
        idx = (part[lit], records["pixel"][lit].astype(np.int64))
        np.add.at(sums[e], idx, rgb[lit])
        np.add.at(counts[e], idx, 1)
    return sums, counts


def record_keys(records):
    """(pixel, sample, bounce, kind) of every record, as rows"""
    return np.stack([records[k].astype(np.int64) for k in ("pixel", "sample", "bounce", "kind")], axis=1)
