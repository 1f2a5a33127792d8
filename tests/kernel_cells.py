"""The shade kernels' members, one scene each: surface model x emitter set x pipeline (tests/test_kernel_cells_host.py on the CPU,
tests/test_gpu_kernel_cells.py on the device).  Every shading kernel is a template over a surface-model mask and an emitter mask, and
csrc/api.hip picks the instantiation from tables (kShadeVariants, kClass, kGroupShade, kGroupShadeTr, kVGroup, kVEventAll); a wrong mask
or a slot mix-up shows only in a scene that holds exactly that model, under that emitter set, in that pipeline.  `scene` makes that
scene, `CELLS` declares the matrix, `expected` says what `info()` must report for a cell.  Not collected by pytest (no `test_` prefix);
nothing here needs a device."""
import os
import xml.etree.ElementTree as xet

import numpy as np

from conftest import ROOT
from flat_cases import _area, _attach, _box, _point

FILM = (64, 48, 64)                     # width, height, samples per pixel of every cell (tests/test_kernel_cells_host.py holds the scenes to it)
MAX_BOUNCE = 6

# ---------------------------------------------------------------- the models: kClass's rows (and clear glass, the delta class's other model)
# parameters chosen to tell the models apart on the object: a colour of its own each, wide lobes, a large sigma
_MODEL_XML = {
    "lambertian": '<brdf type="lambertian" id="m"><rgb name="k_d" value="#E07030"/></brdf>',
    "blinn-phong": '<brdf type="phong" id="m"><rgb name="k_d" value="#3060D0"/><rgb name="k_g" value="12.0"/><rgb name="k_s" value="#707070"/></brdf>',
    "oren-nayar": '<brdf type="oren-nayar" id="m"><rgb name="k_d" value="#D0C040"/><rgb name="sigma" value="40.0"/></brdf>',
    "delta": '<brdf type="specular" id="m"><rgb name="k_d" value="#E0E0E0"/></brdf>',
    "glass": '<bsdf type="det-refraction" id="m"><rgb name="k_d" value="#F0F0F0"/><medium type="transparent"><float name="ior" value="1.5"/></medium></bsdf>',
    "mod-phong": '<brdf type="mod-phong" id="m"><rgb name="k_d" value="#30B060"/><rgb name="k_g" value="8.0"/><rgb name="k_s" value="#808080"/></brdf>',
    "fresnel-blend": '<brdf type="fresnel-blend" id="m"><rgb name="k_d" value="#B040B0"/><rgb name="k_s" value="#404040"/><rgb name="k_g" r="20" g="200"/></brdf>',
    "thin-coat": '<brdf type="thin-coat" id="m"><rgb name="k_d" value="#40B0C0"/><rgb name="k_s" value="0.9"/><rgb name="sigma" r="20" g="20" b="1.5"/></brdf>',
    "lambert-trans": '<bsdf type="lambertian" id="m"><rgb name="k_d" value="#D05050"/><medium type="transparent"><float name="ior" value="1.4"/></medium></bsdf>',
    "microfacet": '<brdf type="microfacet" id="m"><rgb name="k_d" value="#C09050"/><rgb name="roughness" value="0.25"/><rgb name="ref_ior" r="1.0" g="1.5" b="0.0"/></brdf>',
    "blinn-phong(no lobe)": '<brdf type="phong" id="m"><rgb name="k_d" value="#8050C0"/><rgb name="k_g" value="1.0"/><rgb name="k_s" value="0.0"/></brdf>',
}
CLASSES = ("lambertian", "blinn-phong", "oren-nayar", "delta", "mod-phong", "fresnel-blend", "thin-coat", "lambert-trans", "microfacet",
           "blinn-phong(no lobe)")                                         # the names csrc/api.hip kClass gives its rows
VCLASSES = CLASSES[:-1]                                                    # the volumetric tracer does not split Blinn-Phong by lobe
MODELS = CLASSES + ("glass",)
ALL_MODELS = "all-models"                                                  # the scene of more classes than queues (volumetric: one surface queue)
# members of each surface group kernel and of each volumetric one (which models a wrong slot would shade an object with)
GROUPS = (("lambertian", "delta", "lambert-trans", "blinn-phong(no lobe)"), ("blinn-phong", "oren-nayar", "thin-coat", "microfacet", "mod-phong", "fresnel-blend"))
VGROUPS = (("lambertian", "oren-nayar", "delta", "lambert-trans"), ("thin-coat", "microfacet"), ("blinn-phong", "mod-phong", "fresnel-blend", "blinn-phong(no lobe)"))
EMITTER_SETS = ("P+A", "ALL", "P+S")
EMITTER_TYPES = {"P+A": ("point", "area"), "ALL": ("point", "area", "spot", "collimated", "area"), "P+S": ("point", "spot")}
_WALL_XML = {"lambertian": '<brdf type="lambertian" id="{i}"><rgb name="k_d" value="{c}"/></brdf>',
             "blinn-phong": '<brdf type="phong" id="{i}"><rgb name="k_d" value="{c}"/><rgb name="k_g" value="6.0"/><rgb name="k_s" value="#282828"/></brdf>'}
_ALL_MODELS_OBJECTS = ("blinn-phong", "oren-nayar", "delta", "mod-phong", "fresnel-blend", "thin-coat", "lambert-trans")      # + the Lambertian room: eight classes


def walls_of(model):
    """the room's model: Lambertian, and Blinn-Phong with a lobe around the Lambertian object - two material classes either way"""
    return "blinn-phong" if model == "lambertian" else "lambertian"


def _material(xml):
    """parsed with the microfacet switch on (materials.ENABLE_MICROFACET), as the microfacet scenes of the suite are"""
    from adapt_amd import materials, synth
    switch = materials.ENABLE_MICROFACET
    materials.ENABLE_MICROFACET = True
    try:
        return synth._mat(xml)
    finally:
        materials.ENABLE_MICROFACET = switch


def _emitters(emitter_set):
    from adapt_amd.emitters import SOURCE_MAP
    from adapt_amd.synth import _spot
    point = _point((2.78, 4.2, -0.5), 25.0)
    if emitter_set == "P+A":
        return [point, SOURCE_MAP["area"](xet.fromstring('<emitter type="area" id="quad"><rgb name="emission" value="20.0, 18.0, 16.0"/></emitter>'))]
    spot = _spot("4.0, 4.0, 6.0", "30.0", (4.8, 4.8, -0.3), (-2.2, -3.9, 1.9), 25.0, "spot")
    if emitter_set == "P+S":
        return [point, spot]
    beam = SOURCE_MAP["collimated"](xet.fromstring('<emitter type="collimated" id="beam"><rgb name="emission" value="12.0, 20.0, 12.0"/><point name="pos" x="0.6" y="4.6" z="-0.6"/>'
                                                   '<point name="dir" x="1.0" y="-3.45" z="2.2"/><float name="radius" value="0.7"/></emitter>'))
    return [point, _area(20.0, "quad"), spot, beam, _area(40.0, "ball")]


_volume = []


def _grid_volume():
    """the grid volume of scenes/test/volgrid_a.xml, read once"""
    if not _volume:
        from adapt_amd.volumes import GridVolume_np
        path = os.path.join(ROOT, "scenes", "test", "vol", "puffs_20x16x12.vol")
        _volume.append(GridVolume_np(xet.fromstring(
            f'<volume name="puffs" type="mono" phase_type="hg"><string name="density_grid" path="{path}"/><rgb name="albedo" value="#F0F0F0"/>'
            '<rgb name="density_scaling" value="3.0"/><rgb name="par" value="0.5"/><bool name="mono2rgb" value="true"/>'
            '<transform name="toWorld"><translate x="1.6" y="0.4" z="1.4"/><rotate type="euler" r="0" p="0.0" y="0"/><scale x="0.12" y="0.12" z="0.12"/></transform></volume>')))
    return _volume[0]


def scene(model, emitter_set, volumetric=False, grid_volume=False, walls=None, only_emitter=None):
    """The Cornell room with one analytic sphere and one box mesh of `model` under the emitters of `emitter_set`, every one of which
    lights the two objects -> the 4-tuple `scene_parsing` returns.  Two material classes: the room's walls (`walls`, default walls_of(model))
    and the model.  model ALL_MODELS: seven objects of a class each in the Lambertian room.  volumetric: a thin scattering world medium;
    grid_volume: volgrid_a's density grid on top.  only_emitter: every other emitter's intensity is zero (the streams stay as they are).
    The objects of the model under test carry `under_test` on their material."""
    from adapt_amd import synth
    from adapt_amd.parsers.world import World_np
    assert emitter_set in EMITTER_SETS and (model in MODELS or model == ALL_MODELS), (model, emitter_set)
    wall = _WALL_XML[walls or walls_of(model)]
    white, red, green, lamp = (_material(wall.format(i=i, c=c)) for i, c in (("white", "#BDBDBD"), ("left", "#DD2525"), ("right", "#25DD25"), ("lamp", "#555555")))
    b = synth._Builder()
    synth._room(b, white, red, green)
    emitters = _emitters(emitter_set)
    if emitter_set != "P+S":
        b.cornell("luminaire", lamp, (0.0, -0.001, 0.0), emitter=1)
    if emitter_set == "ALL":
        b.sphere((5.0, 3.2, 0.6), 0.25, lamp)
        _attach(b, 4, sphere=True)
    if model == ALL_MODELS:
        spots = [(1.0, 0.0, 3.4), (2.78, 0.0, 3.6), (4.5, 0.0, 3.4), (0.8, 0.0, 1.4), (2.15, 0.0, 1.0), (3.5, 0.0, 1.0), (4.78, 0.0, 1.5)]
        for k, (name, (x, y, z)) in enumerate(zip(_ALL_MODELS_OBJECTS, spots)):
            mat = _material(_MODEL_XML[name]); mat.under_test = True
            if k % 2: b.mesh(_box((x - 0.55, 0.0, z - 0.55), (x + 0.55, 3.0 if k == 1 else 1.3, z + 0.55)), mat)
            else: b.sphere((x, 2.2 if k < 3 else 0.68, z), 0.68, mat)      # (the back row floats above the front row)
    else:
        mat = _material(_MODEL_XML[model]); mat.under_test = True
        b.sphere((1.6, 1.3, 1.5), 1.3, mat)
        b.mesh(_box((3.2, 0.0625, 0.6), (4.9, 1.9625, 2.2)), mat)      # (clear of the floor: a ray inside a transmissive box must not find two faces at one distance)
    tup = b.finish(emitters, synth._sensor(FILM[0], FILM[1], MAX_BOUNCE, 1))
    prop = tup[3]
    if volumetric:
        prop["world"] = World_np(xet.fromstring('<world><medium type="hg"><rgb name="u_a" value="0.01"/><rgb name="u_s" value="0.06"/>'
                                                '<rgb name="par" value="0.3"/><float name="ior" value="1.0"/></medium></world>'))
    if grid_volume:
        assert volumetric
        prop["volume"] = [_grid_volume()]
    if only_emitter is not None:
        for k, e in enumerate(emitters):
            if k != only_emitter: e.intensity = np.zeros(3, np.float32)
    return tup


def object_region(tup, oracle, rc):
    """(w, h) bool: the pixels whose centre ray first hits an object of the model under test, by the oracle's closest hit"""
    W, H = rc.width, rc.height
    i, j = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), indexing="ij")
    cd = np.stack([(rc.half_w + 0.5 - i) * rc.inv_focal, (j - rc.half_h - 0.5) * rc.inv_focal, np.ones_like(i)], -1)      # pixel centres (tests/transient_cases.py _predicted_times)
    d = cd @ np.float64(rc.cam_r).T
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.broadcast_to(np.float32(rc.cam_t), d.shape)
    obj, prim, _, _, _ = oracle.intersect(o.reshape(-1, 3), d.reshape(-1, 3))
    tested = np.array([bool(getattr(ob.bsdf, "under_test", False)) for ob in tup[2]])
    return ((prim >= 0) & tested[np.clip(obj, 0, len(tested) - 1)]).reshape(W, H)


# ---------------------------------------------------------------- the matrix
SORTED, TRANSIENT, STAGED, TRACED, VOLUMETRIC, VOLUMETRIC_GRID = "sorted", "sorted-transient", "staged", "traced", "volumetric", "volumetric+grid"
PRODUCT_ONLY = (TRACED,)               # the kernels that trace their own rays exist on the flat sweep, which the exact build has not
# staged / traced: one cell on kShadeVariants[1], two on [2] (a mirror, clear glass), and on [3] every model that [0..2] do not hold
_PLAIN_NAMES = ("phong+lambertian/point+area", "phong+lambertian+mirror+glass/point+area", "all models")
_UNSORTED = [("blinn-phong", "P+A", 0), ("delta", "P+A", 1), ("glass", "P+A", 1)] + \
            [(m, s, 2) for m in ("oren-nayar", "mod-phong", "fresnel-blend", "thin-coat", "lambert-trans", "microfacet") for s in ("P+A", "ALL")]
CELLS = [(m, s, p) for p in (SORTED, TRANSIENT) for m in CLASSES for s in EMITTER_SETS] + \
        [(m, s, p) for p in (STAGED, TRACED) for m, s, _ in _UNSORTED] + \
        [(m, s, p) for p in (VOLUMETRIC, VOLUMETRIC_GRID) for m in VCLASSES + (ALL_MODELS,) for s in ("P+A", "ALL")]
SWITCHES = {SORTED: {}, TRANSIENT: {}, STAGED: {"APT_SORTED": "0", "APT_FUSED": "0"}, TRACED: {"APT_SORTED": "0"}, VOLUMETRIC: {}, VOLUMETRIC_GRID: {}}


def cells_of(build):
    return [c for c in CELLS if build == "fast" or c[2] not in PRODUCT_ONLY]


def is_volumetric(cell):
    return cell[2] in (VOLUMETRIC, VOLUMETRIC_GRID)


def scene_key(cell):
    """cells with the same key render the same scene under the same configuration (the oracle's images are shared among them)"""
    model, emitter_set, pipeline = cell
    return (model, emitter_set, is_volumetric(cell), pipeline == VOLUMETRIC_GRID)


def scene_of(cell):
    return scene(*scene_key(cell))


def class_names(model):
    """the material classes of the cell's scene, by kClass's names"""
    if model == ALL_MODELS:
        return {"lambertian"} | set(_ALL_MODELS_OBJECTS)
    return {"delta" if model == "glass" else model, walls_of(model)}


def expected(cell, build):
    """-> (check(shade_variant) -> bool, the traversals info() may report) for the cell on `build` ("exact" / "fast"): csrc/api.hip
    pick_traversal and pick_shading restated for scenes of at most 96 primitives"""
    model, emitter_set, pipeline = cell
    traversal = ("flat",) if build == "fast" else ("sweep", "tile")
    names = class_names(model)
    if pipeline in (SORTED, TRANSIENT):
        head, tail = "sorted, launched in register-footprint groups:", " [transient]" if pipeline == TRANSIENT else ""
        return (lambda v: v.startswith(head) and v.endswith(tail) and set(v[len(head):len(v) - len(tail)].split("+")) == names), traversal
    if pipeline in (STAGED, TRACED):
        (row,) = [k for m, s, k in _UNSORTED if (m, s) == (model, emitter_set)]
        return (lambda v: v == _PLAIN_NAMES[row] + (" [rays traced in place]" if pipeline == TRACED else "")), traversal
    head = "volumetric + grid volume, sorted by event: medium | " if pipeline == VOLUMETRIC_GRID else "volumetric, sorted by event: medium | "
    if model == ALL_MODELS:                     # eight classes and the medium: more than the event queues, one surface queue
        return (lambda v: v == head + "all surface models"), traversal
    return (lambda v: v.startswith(head) and set(v[len(head):].split("+")) == names), traversal


# ---------------------------------------------------------------- the oracle's side of a scene, rendered once and shared (read-only)
class Reference:
    """scene tuple, configuration, oracle scene, object region, the oracle's accumulation and counters with seed 0 and its images
    (float64, divided by the sample count) with seeds 0, 1, 2 at FILM (`spp`: another sample count)"""
    def __init__(self, key, walls=None, only_emitter=None, seeds=(0, 1, 2), use_mis=True, spp=FILM[2]):
        from adapt_amd.scene_pack import make_config, pack_scene
        from oracle import binding as ob
        model, emitter_set, volumetric, grid = key
        self.tup = scene(model, emitter_set, volumetric, grid, walls=walls, only_emitter=only_emitter)
        self.tup[3]["use_mis"] = use_mis
        self.packed = pack_scene(*self.tup)
        self.config = lambda seed=0: make_config(self.tup[3], width=FILM[0], height=FILM[1], seed=seed, volumetric=volumetric)
        self.rc = self.config()
        self.oracle = ob.OracleScene(self.packed, self.rc.cam_t)
        self.region = object_region(self.tup, self.oracle, self.rc)
        self.cpu, self._log_sum = {}, None
        for seed in seeds:
            acc, cnt, st = self.oracle.render(self.config(seed), spp, threads=ob.num_threads())
            assert cnt == spp
            acc.setflags(write=False)
            if seed == 0: self.accum, self.stats = acc, st
            self.cpu[seed] = acc.astype(np.float64) / spp

    def render(self, rc, n_spp, threads=0):
        """OracleScene.render's answer for this reference's own configuration (what gpu_cases.render_with_oracle asks for)"""
        assert n_spp == FILM[2] and rc is self.rc
        return self.accum, n_spp, self.stats

    def log_sum(self):
        """What a transient render's framebuffer holds, by the oracle (seed 0): the sum of its per-contribution log, (accumulation
        float64, image).  Where no sample of a pixel has a NaN colour it is the steady accumulation up to summation order; a sample whose
        colour is NaN is zeroed whole by the steady renderer (vanilla_renderer.py:119) while the log, like the device's bins, keeps its
        finite terms (DESIGN.md "Transient rendering") - the microfacet and Fresnel-blend objects have such samples by the thousand."""
        if self._log_sum is None:
            from oracle import binding as ob
            w, h, spp = FILM
            recs, per, st = self.oracle.contributions(self.rc, spp, threads=ob.num_threads())
            assert st["n_draws"] == self.stats["n_draws"]
            rgb = recs["rgb"].astype(np.float64)
            fin = np.isfinite(rgb).all(axis=1)
            total = np.zeros((w * h, 3))
            np.add.at(total, recs["pixel"][fin], rgb[fin])
            total = total.reshape(w, h, 3)
            clean = ~per[..., 4].any(axis=2)                     # pixels without a NaN-coloured sample
            assert np.all(np.abs(total - self.accum)[clean] <= 1e-5 * np.abs(self.accum)[clean] + 1e-4), "the log does not sum to the steady image"
            total.setflags(write=False)
            self._log_sum, self.nan_colour_samples = total, int(per[..., 4].sum())
        return self._log_sum, self._log_sum / FILM[2]

    def noise(self, mask=None):
        """relMSE between the oracle's seeds 1 and 2, over the whole film or over `mask`"""
        from gpu_cases import _rel
        m = np.ones(self.region.shape, bool) if mask is None else mask
        return _rel(self.cpu[1][m], self.cpu[2][m])


_references = {}


def reference(key):
    if key not in _references:
        _references[key] = Reference(key)
    return _references[key]


PRODUCT_FRACTION_OF_NOISE = 0.02       # the product build's same-seed relMSE as a fraction of the oracle's seed-to-seed noise: the bound
#                                        tests/test_gpu_fast.py::test_no_systematic_difference_between_the_builds holds between the two builds
SENSITIVITY_FACTOR = 10.0              # a wrong member's image is at least this many times that bound away from the right one


def swap_partners(model):
    """the models a wrong slot or mask could shade `model`'s object with: the other members of its surface group kernel and of its
    volumetric group kernel, and Lambertian"""
    (g,) = [g for g in GROUPS if model in g]
    (v,) = [v for v in VGROUPS if model in v]
    return sorted((set(g) | set(v) | {"lambertian"}) - {model})
