"""The sensor-settings matrix (helper module: no tests in here).

A render is driven by nine sensor settings - use_rr, rr_bounce_th, rr_threshold, use_mis, anti_alias, stratified_sampling, brdf_two_sides,
num_shadow_ray, max_bounce - and the scene files carry only a handful of their combinations.  CASES flips each of them alone (and a few
pairs) from the scene's own values, on scenes that both this repo's parser and the reference's read.  One list, shared by

  * tests/golden/gen/gen_goldens.py --only settings: the reference's own kernel on every case -> tests/golden/settings_matrix.npz,
  * tests/test_settings_matrix.py (CPU): the oracle reproduces that fixture bit for bit,
  * tests/test_gpu_settings_matrix.py (device, both builds): image, counters and pipeline of every case.

An override dict uses the sensor's own key names (what `scene_parsing` puts into its property dict, what the reference's renderer reads).
"""
import os
from collections import namedtuple

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

Case = namedtuple("Case", "name scene axis overrides volumetric")

# scene -> (directory under scenes/, file of this repo, (directory under the reference's scenes/, its file) or None: the reference reads
# this repo's file, volumetric tracer).  cbox / balls_mono / glass_box are the reference's cbox.xml / balls-mono.xml / complex.xml.
SCENES = {
    "cbox": ("cbox", "c2_cbox.xml", ("cbox", "cbox.xml"), False),                    # point light, Lambertian: the lean traced kernels
    "balls_mono": ("csphere", "c3_balls_mono.xml", ("csphere", "balls-mono.xml"), False),     # class-sorted kernels
    "glass_box": ("cbox", "glass_box.xml", ("cbox", "complex.xml"), False),          # delta BSDFs: the non-lean traced kernel
    "features_a": ("test", "features_a.xml", None, False),                           # all five emitter types
    "media_a": ("test", "media_a.xml", None, True),                                  # VolumeRenderer: the event-sorted volumetric pipeline
}
# given to BOTH sides on every case of the scene: this repo's c2_cbox.xml and the reference's cbox.xml differ in max_bounce (8 / 12)
COMMON = {"cbox": {"max_bounce": 8}}

# axis label -> override, each flipped alone from the scene's own values
FLAG_AXES = {
    "rr_off": {"use_rr": False},
    "rr_bounce_0": {"rr_bounce_th": 0},
    "rr_bounce_1": {"rr_bounce_th": 1},
    "rr_every_vertex": {"rr_threshold": 2.0, "rr_bounce_th": 0},        # max throughput component < 2.0 holds everywhere: roulette at every vertex
    "mis_off": {"use_mis": False},
    "no_jitter": {"anti_alias": False},
    "uniform_jitter": {"stratified_sampling": False},
    "two_sided": {"brdf_two_sides": True},
}
SHADOW_COUNTS = (0, 1, 2, 3, 5, 8)
BOUNCE_LIMITS = (1, 2)
AXES = dict(FLAG_AXES)
AXES.update({f"shadow_{s}": {"num_shadow_ray": s} for s in SHADOW_COUNTS})
AXES.update({f"bounce_{b}": {"max_bounce": b} for b in BOUNCE_LIMITS})
FULL_MATRIX_SCENES = ("cbox", "balls_mono", "media_a")
SUBSET_SCENES = ("glass_box", "features_a")
SUBSET_AXES = ("mis_off", "two_sided", "rr_off", "shadow_2", "shadow_5")
PAIR_SCENES = ("cbox", "balls_mono")
PAIRS = {
    "mis_off+two_sided": ("mis_off", "two_sided"),
    "rr_off+shadow_0": ("rr_off", "shadow_0"),
    "no_jitter+rr_off+mis_off": ("no_jitter", "rr_off", "mis_off"),
    "shadow_5+two_sided": ("shadow_5", "two_sided"),
}


def _case(scene, axis, parts):
    ov = dict(COMMON.get(scene, {}))
    for p in parts:
        ov.update(AXES[p])
    return Case(f"{scene}-{axis}", scene, axis, ov, SCENES[scene][3])


CASES = ([_case(s, a, (a,)) for s in FULL_MATRIX_SCENES for a in AXES]
         + [_case(s, a, (a,)) for s in SUBSET_SCENES for a in SUBSET_AXES]
         + [_case(s, a, parts) for s in PAIR_SCENES for a, parts in PAIRS.items()])
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# film of the reference-run fixture (tests/golden/settings_matrix.npz)
FIXTURE_W, FIXTURE_H, FIXTURE_SPP, FIXTURE_SEED = 16, 12, 3, 0
SETTING_KEYS = ("use_rr", "rr_bounce_th", "rr_threshold", "use_mis", "anti_alias", "stratified_sampling", "brdf_two_sides", "num_shadow_ray", "max_bounce")


def cases_of(scene):
    return [c for c in CASES if c.scene == scene]


def within_queue_limit(num_shadow_ray, max_bounce):
    """apt_renderer_create's own limit on the draw window of a path"""
    return (5 * num_shadow_ray + 8) * max_bounce + 4 < 65536


_parsed = {}


def parse(scene):
    """this repo's front end on the scene's file (cached): the 4-tuple `scene_parsing` returns"""
    if scene not in _parsed:
        from adapt_amd.parsers import scene_parsing
        cwd = os.getcwd()
        os.chdir(ROOT)                              # asset paths in the scene files are relative to the repository root
        try:
            _parsed[scene] = scene_parsing(os.path.join(ROOT, "scenes", SCENES[scene][0]), SCENES[scene][1])
        finally:
            os.chdir(cwd)
    return _parsed[scene]


def with_overrides(tup, overrides):
    """the parsed scene with the case's settings written into a COPY of its property dict"""
    prop = dict(tup[3])
    prop.update(overrides)
    return tup[0], tup[1], tup[2], prop


def settings(case):
    """all nine settings the case renders with: the scene's own values, the overrides on top"""
    prop = with_overrides(parse(case.scene), case.overrides)[3]
    d = {"rr_bounce_th": 4, "rr_threshold": 0.1, "brdf_two_sides": False}         # the reference's defaults where the file is silent
    d.update({k: prop[k] for k in SETTING_KEYS if k in prop})
    return d
