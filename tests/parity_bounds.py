"""The parity bounds that more than one test module reads, per build, each written once with what it was measured from.  A bound that a
single test uses stays a literal at that test's call of its body (tests/gpu_cases.py).  Not collected by pytest (no `test_` prefix);
nothing here needs a device.  tests/test_gpu_cases_host.py restates the two SURVEY 8(d) rows once, on purpose."""
from collections import namedtuple

Row = namedtuple("Row", "within rel counters")          # min fraction of pixels within 1e-3 (1 + |x|), max relMSE, counters: relative

# ---------------------------------------------------------------- exact build (libadapt_mi_exact.so)
# SURVEY 8(d), project policy: images, device vs oracle with the SAME Philox stream: >= 99.5 % of pixels within 1e-3 (1 + |x|) per channel
# and relMSE <= 1e-4 (an ulp-level difference can flip a branch and re-draw a path; nothing else may differ); path statistics (vertices
# shaded, light samples taken, random numbers drawn) within 2e-4.  tests/test_gpu_parity.py::test_image_matches_oracle_same_stream holds
# it on the scenes' own settings, tests/test_gpu_settings_matrix.py under every sensor setting.
EXACT = Row(0.995, 1e-4, 2e-4)
# the exact build against a fixture recorded from the reference's own kernel (tests/test_gpu_parity.py::test_image_matches_reference_run,
# tests/test_gpu_settings_matrix.py (b)): 2-6 spp on ~1000 pixels, the last figure bounds the number of random numbers drawn
REFERENCE_RUN = Row(0.99, 2e-4, 2e-3)

# ---------------------------------------------------------------- product build (libadapt_mi.so)
# tag, width, height, spp, overrides, min fraction of pixels within 1e-3 (1 + |x|), max relMSE.
#
# SURVEY 8(d) states its tolerance ON C1: ">= 99 % of pixels within 1e-3 (1 + |x|) per channel at 64 spp (C1), image relMSE <= 1e-4".  The
# product build meets it on C1 and on every BASELINE config (C2 / C3 at full film size: the two *_full_frame_every_pixel_* tests of
# tests/test_gpu_fast.py; C4 / C5: its crop tests) and on the diffuse Cornell renders.  On the FEATURE scenes of this repo (glass, mirrors,
# glossy lobes in a closed box at 96 x 96) the SAME-STREAM per-pixel criterion is not met, and the bounds below are NOT 8(d)'s: they are
# regression guards,
# the value measured on MI355X (the GPU path is bit-reproducible, so the measurement is a property of the build; profiles/
# r06_parity_metrics.log - round 6's product build: float transcendentals, 1-ulp divisions in the non-delta shading code - re-recorded every round by record_metric) with a margin of two on the failing fraction and on relMSE.
# Side by side, so that the relaxation is visible:
#
#   scene            8(d) asks (same stream)     product build, measured     exact build (asserted)     bound asserted here
#   cbox 256 (C1)    >= 99 %, relMSE <= 1e-4     99.945 %, 2.9e-7            >= 99.5 %, <= 1e-4         99.89 %, 6e-7      (inside 8(d))
#   cbox 96          >= 99 %, relMSE <= 1e-4     99.946 %, 5.2e-7            >= 99.5 %, <= 1e-4         99.89 %, 1.1e-6    (inside 8(d))
#   balls_mono (C3)  >= 99 %, relMSE <= 1e-4     99.60 %, 4.8e-7             >= 99.5 %, <= 1e-4         99.2 %, 1e-6       (inside 8(d))
#   microfacet       >= 99 %, relMSE <= 1e-4     99.45 %, 3.9e-5             >= 99.5 %, <= 1e-4         98.9 %, 8e-5       (inside 8(d))
#   textured         >= 99 %, relMSE <= 1e-4     98.0 %, 1.4e-4              >= 99.5 %, <= 1e-4         96 %, 3e-4         (OUTSIDE: per-pixel and relMSE)
#   glass_box        >= 99 %, relMSE <= 1e-4     95.8 %, 4.1e-5              >= 99.5 %, <= 1e-4         91.6 %, 8.2e-5     (OUTSIDE: per-pixel)
#   features_a       >= 99 %, relMSE <= 1e-4     88.2 %, 1.74e-4             >= 99.5 %, <= 1e-4         76.4 %, 3.5e-4     (OUTSIDE: per-pixel and relMSE)
#   features_b       >= 99 %, relMSE <= 1e-4     91.3 %, 6.0e-4              >= 99.5 %, <= 1e-4         82.6 %, 1.2e-3     (OUTSIDE: per-pixel and relMSE)
#   features_c       >= 99 %, relMSE <= 1e-4     88.4 %, 1.66e-4             >= 99.5 %, <= 1e-4         76.8 %, 3.4e-4     (OUTSIDE: per-pixel and relMSE)
#
# Why outside, and what stands in for the per-pixel criterion there: a specular or glossy path is chaotic in its hit point - an ulp of
# difference in one hit (the flat sweep's precomputed-transform test against the reference's adjugate solve, both within 1e-5 t) is amplified
# by every bounce until a branch flips and the REST of the path is re-drawn; the pixel then carries another, equally valid sample.  That is
# a property of comparing two float32 intersectors on one random stream, not an error of the estimator, and 8(d) provides the check that
# separates the two: "relMSE(HIP, CPU-other-seed) within 1.5x of relMSE(CPU-seedA, CPU-seedB)".  test_statistical_cross_check_other_seed
# asserts exactly that for EVERY scene of this table (round 6: features_a / b / c, glass_box, microfacet added), and
# test_no_systematic_difference_between_the_builds holds the product build's vertex counts, energy and image to the exact build's on every
# one of them at 1 024 - 2 048 spp.  The exact build (tests/test_gpu_parity.py) holds 8(d) verbatim on all of these scenes.
PRODUCT_IMAGE_CASES = [
    ("cbox", 256, 256, 64, {"max_bounce": 4}, 0.9989, 6e-7),
    ("cbox", 96, 96, 64, {}, 0.9989, 1.1e-6),
    ("balls_mono", 96, 96, 64, {}, 0.992, 1e-6),
    ("glass_box", 96, 96, 64, {}, 0.916, 8.2e-5),
    ("features_a", 96, 96, 64, {}, 0.764, 3.5e-4),
    ("features_b", 96, 96, 64, {}, 0.826, 1.2e-3),
    ("features_c", 96, 96, 64, {}, 0.768, 3.4e-4),
    ("textured", 64, 48, 16, {}, 0.96, 3e-4),           # (its normal-mapped wall sends out rays that are not of unit length: traverse.hpp flat_needs_cull)
    ("microfacet", 64, 48, 16, {}, 0.989, 8e-5),
]

# The capacity scenes of tests/flat_cases.py (96 primitives, tests/test_gpu_flat_capacity.py) have no measured row of their own: each
# variant is held to the row of the bundled scene whose pipeline it runs - `lean` (Lambertian surfaces, one point light: the lean traced
# kernels) to cbox at 96 x 96, `delta` (a glass box, mirrors: the non-lean traced kernel) to glass_box, `sorted` (three material classes,
# area emitters, four light samples per vertex: the class-sorted pipeline) to balls_mono - and `volumetric` to VPT_PRODUCT_BOUNDS below.
# What they measure at 48 x 40 x 8 spp stands in profiles/NOTES.md ("The flat sweep at capacity").
CAPACITY_PRODUCT_ROWS = {"lean": ("cbox", 96), "delta": ("glass_box", 96), "sorted": ("balls_mono", 96)}
# One case misses the row it borrows, on the per-pixel fraction alone: capacity_mixed `sorted` measures 98.65 % and relMSE 4.0e-7 (inside
# balls_mono's 1e-6) against the oracle, its path statistics equal to the last count.  Per-pixel evidence: the 26 pixels outside are
# outside by 1.06 .. 3.5 times the threshold, the size of ONE of a vertex's 4 x 8 light samples changing between lit and blocked
# (n_lit 143 774 against 143 818 of the same build's reference-order sweep, 3e-4 of them); the same build with its traversal forced to
# `sweep` - the exact build's intersector under the product build's shading arithmetic - measures 98.75 % against the oracle, on 24
# pixels of which 17 are the same: the flips come with the product build's 1-ulp shading arithmetic, not with the flat sweep.  Their
# likely seat - what the scene has and balls_mono has not - is the SPHERE emitter: the reference samples its whole surface, a sample near the silhouette reaches it
# at a grazing angle, where a sphere hit is uncertain by ~sqrt(2^-24) of the distance (flat_build.cpp flat_occluders) - more than the
# 1e-4 the shadow test leaves before the light -, and 54 shards put silhouettes in front of both emitters.  Noise of that geometry, as
# the features_* rows above carry for their sphere light: the measured fraction with the table's margin of two on the failing part, the
# borrowed relMSE kept.  The all-triangle scene (a mesh emitter alone) holds balls_mono's row as it stands: 99.95 %, 6.7e-7.
CAPACITY_MEASURED_WITHIN = {("capacity_mixed", "sorted"): 0.9729}


def capacity_product_row(name, variant):
    """-> (min fraction of pixels within 1e-3 (1 + |x|), max relMSE): the PRODUCT_IMAGE_CASES row the variant borrows, with the one
    measured fraction above in its place"""
    tag, width = CAPACITY_PRODUCT_ROWS[variant]
    (row,) = [c for c in PRODUCT_IMAGE_CASES if c[0] == tag and c[1] == width]
    return CAPACITY_MEASURED_WITHIN.get((name, variant), row[5]), row[6]


COUNTER_TOL = (5e-4, 150)          # path statistics against the oracle on the same stream: relative, and an absolute floor for small renders

# same-seed relMSE bound at 48 x 48 x 64 spp as a fraction of the seed-to-seed noise floor (measured x 2, recorded by record_metric): the scenes
# that hold 8(d)'s 1e-4 outright carry None
SAME_SEED_FRACTION_OF_NOISE = {"cbox": None, "balls_mono": None, "microfacet": None, "textured": 1e-2, "glass_box": 5e-2, "features_a": 5e-2, "features_b": 5e-2, "features_c": 5e-2}

# the five vpt scenes against their reference-run fixtures and the oracle (tests/gpu_cases.py volumetric_scene_vs_reference_run_and_oracle):
# the product build's closest-hit queries go through the flat sweep where the exact build (that body's defaults) runs the reference's loop
VPT_PRODUCT_BOUNDS = dict(within=0.97, rel=2e-3, draws_tol=3e-3, stat_tol=1e-3)
