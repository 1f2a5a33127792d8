"""Helpers shared by the tests of the flat sweep's record builder (tests/test_flat_records.py, tests/test_shadow_cull.py,
tests/test_camera_cull.py on the CPU; tests/test_gpu_fast.py on the device), and the scenes that fill the flat sweep to its 96 primitives
(capacity_mixed, capacity_tris and their kin, below; tests/test_gpu_flat_capacity.py on the device).  Not collected by pytest (no `test_`
prefix); nothing here needs a device."""
import ctypes as C

import numpy as np

from adapt_amd import _lib


def flat_records(prims, obj_info):
    lib = _lib.load()
    prims = np.ascontiguousarray(prims, np.float32).reshape(-1, 9); obj_info = np.ascontiguousarray(obj_info, np.int32).reshape(-1, 3)
    counts = np.zeros(7, np.int32); ns, nt = C.c_int32(0), C.c_int32(0)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)); ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    _lib.check(lib.apt_flat_records(fp(prims), prims.shape[0], ip(obj_info), obj_info.shape[0], ip(counts), None, 0, None, 0, C.byref(ns), C.byref(nt)), "apt_flat_records", lib)
    stream, tab = np.zeros(ns.value, np.float32), np.zeros(nt.value, np.float32)
    _lib.check(lib.apt_flat_records(fp(prims), prims.shape[0], ip(obj_info), obj_info.shape[0], ip(counts), fp(stream), ns.value, fp(tab), nt.value, C.byref(ns), C.byref(nt)), "apt_flat_records", lib)
    return counts, stream, tab


def sections(counts):
    """per record: section (0 parallelogram, 1 convex quad, 2 triangle, 3 sphere) and its offset in the stream"""
    n = [counts[0] + counts[1], counts[2] + counts[3], counts[4] + counts[5], counts[6]]
    out, at = [], 0
    for sec, w in enumerate((12, 18, 12, 4)):
        for _ in range(n[sec]):
            out.append((sec, at)); at += w
    return out


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _quad_soup(seed):
    """A scene of planar shapes for the flat sweep's record builder (csrc/flat_build.cpp): convex quadrilaterals, parallelograms, concave
    quadrilaterals (their two triangles must NOT be merged into a convex-quad record), slightly folded quads (not coplanar: not merged),
    triangle fans, coplanar triangles that share no edge, lone triangles - every triangle with a random vertex rotation."""
    from adapt_amd import synth
    rs = np.random.RandomState(seed)
    b = synth._Builder()
    white = synth._brdf("lambertian", "#BDBDBD")

    def frame():
        n = rs.normal(size=3); n /= np.linalg.norm(n)
        a = np.cross(n, rs.normal(size=3)); a /= np.linalg.norm(a)
        return rs.uniform(1.0, 4.5, 3), a, np.cross(n, a), n

    def rot(tri):
        k = rs.randint(3)
        return np.roll(tri, k, axis=0)

    def emit(tris):
        b.mesh(np.float32([rot(np.asarray(t)) for t in tris]), white)

    for kind in ["convex"] * 6 + ["para"] * 3 + ["concave"] * 3 + ["folded"] * 2:
        c, a, bb, n = frame()
        if kind == "convex":
            ang = np.sort(rs.uniform(0, 2 * np.pi, 4)); ang += np.float64([0.0, 0.3, 0.6, 0.9])      # four points around a centre, in order
            rad = rs.uniform(0.5, 1.2, 4)
            pts = [c + r * (np.cos(t) * a + np.sin(t) * bb) for r, t in zip(rad, ang)]
            hull_ok = all(np.dot(np.cross(pts[(i + 1) % 4] - pts[i], pts[(i + 2) % 4] - pts[(i + 1) % 4]), n) > 0 for i in range(4))
            if not hull_ok:
                pts = [c + 0.8 * (np.cos(t) * a + np.sin(t) * bb) for t in (0.2, 1.9, 3.3, 4.9)]
        elif kind == "para":
            e1, e2 = rs.uniform(0.5, 1.2) * a + rs.uniform(-0.3, 0.3) * bb, rs.uniform(0.5, 1.2) * bb
            pts = [c, c + e1, c + e1 + e2, c + e2]
        elif kind == "concave":
            pts = [c + 1.0 * a, c + 0.15 * (a + bb), c + 1.0 * bb, c - 0.8 * (a + bb)]                # reflex corner at pts[1]: split along 1-3
            emit([[pts[1], pts[2], pts[3]], [pts[1], pts[3], pts[0]]])
            continue
        else:
            pts = [c, c + a, c + a + bb + 2e-3 * n, c + bb]
        emit([[pts[0], pts[1], pts[2]], [pts[0], pts[2], pts[3]]])
    c, a, bb, n = frame()                                                                            # a fan of five coplanar triangles
    ring = [c + 0.9 * (np.cos(t) * a + np.sin(t) * bb) for t in np.linspace(0, 2 * np.pi, 6)[:-1]]
    emit([[c, ring[i], ring[(i + 1) % 5]] for i in range(5)])
    c, a, bb, n = frame()                                                                            # coplanar, no shared edge
    emit([[c, c + a, c + bb], [c + 1.5 * a, c + 2.5 * a, c + 1.5 * a + bb]])
    emit([[rs.uniform(0.5, 5.0, 3) for _ in range(3)] for _ in range(10)])                           # lone triangles
    em = [synth._spot("6.0, 6.0, 6.0", "100.0", (2.7, 5.0, 2.7), (0.0, -1.0, 0.0), 40.0, "s")]
    return b.finish(em, synth._sensor(64, 64, 4, 1))


# ---------------------------------------------------------------- scenes at the flat sweep's capacity (traverse.hpp APT_FLAT_MAX_PRIMS)
# The bundled scenes stop at 36 primitives and 9 record pairs.  These fill the stream: 96 primitives, over 40 pairs - so the strip words of
# the three culls (flat_build.cpp camera_strips, flat_occluders, light_strips) carry bits in their upper half -, every section with an odd
# tail, pairs that straddle a section's plain / coplanar-group border, and one primitive more, where the renderer leaves the flat sweep.
# Geometry: a closed room of 5.5 units with the camera inside; every coordinate is a multiple of 1/64, so quads in dyadic planes are
# planar to the last bit.  Deterministic (numpy's RandomState with a fixed seed for the shards).
VARIANTS = ("lean", "delta", "sorted", "volumetric")
ROOM = 5.5
CAMERA = ((0.0, 0.0, 1.0), (2.75, 2.75, 0.3125))      # direction, position: inside the room, behind every shard
FOV = 80.0                                            # the side walls are in the picture


def _para(p0, e1, e2, facing):
    """the two triangles of the parallelogram p0, p0 + e1, p0 + e1 + e2, p0 + e2, wound so that their normal points along `facing`"""
    p0, e1, e2 = np.float64(p0), np.float64(e1), np.float64(e2)
    if np.dot(np.cross(e1, e2), facing) < 0: e1, e2 = e2, e1
    return np.float32([[p0, p0 + e1, p0 + e1 + e2], [p0, p0 + e1 + e2, p0 + e2]])


def _quad(p):
    """the two triangles of the convex quadrilateral p[0..3], split along p[0] - p[2]"""
    p = np.float64(p)
    return np.float32([[p[0], p[1], p[2]], [p[0], p[2], p[3]]])


def _box(lo, hi):
    """the twelve triangles of an axis-aligned box, normals outward: one object, so each face merges into a parallelogram"""
    lo, hi = np.float64(lo), np.float64(hi)
    d = hi - lo
    faces = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        eb, ec, n = np.zeros(3), np.zeros(3), np.zeros(3)
        eb[b], ec[c], n[a] = d[b], d[c], 1.0
        faces.append(_para(lo, eb, ec, -n))
        faces.append(_para(lo + n * d[a], eb, ec, n))
    return np.concatenate(faces)


_WALLS = [((0, 0, 0), (ROOM, 0, 0), (0, 0, ROOM), (0, 1, 0)),          # floor, ceiling, back, left, right, front: normals into the room
          ((0, ROOM, 0), (ROOM, 0, 0), (0, 0, ROOM), (0, -1, 0)),
          ((0, 0, ROOM), (ROOM, 0, 0), (0, ROOM, 0), (0, 0, -1)),
          ((0, 0, 0), (0, ROOM, 0), (0, 0, ROOM), (1, 0, 0)),
          ((ROOM, 0, 0), (0, ROOM, 0), (0, 0, ROOM), (-1, 0, 0)),
          ((0, 0, 0), (ROOM, 0, 0), (0, ROOM, 0), (0, 0, 1))]
_WALL_COLOURS = ["#BDBDBD", "#BDBDBD", "#BDBDBD", "#DD2525", "#25DD25", "#9090C0"]
_ZERO_AREA = [(3.0, 3.0, 3.0), (3.25, 3.25, 3.0), (3.5, 3.5, 3.0)]       # collinear: e1 x e2 = 0 exactly, a record of all-zero rows


def _shards(n, seed, lo, hi, balls=()):
    """n lone triangles of random orientation and an edge of about 0.3 - 0.7, inside the box lo .. hi, vertices on the 1/64 grid; none is
    degenerate, none comes nearer than 0.1 to one of `balls` (centre, radius): no shard pierces a sphere, the emitting one least of all"""
    rs = np.random.RandomState(seed)
    w = np.array([(a, b, 16 - a - b) for a in range(17) for b in range(17 - a)]) / 16.0      # barycentric grid, spacing 1/16 of an edge
    out = []
    while len(out) < n:
        c = rs.uniform(lo, hi)
        t = np.round((c + rs.uniform(-0.35, 0.35, size=(3, 3))) * 64.0) / 64.0
        if np.linalg.norm(np.cross(t[1] - t[0], t[2] - t[0])) < 0.08 or (t < 0.25).any() or (t > ROOM - 0.25).any(): continue
        if any(np.linalg.norm(w @ t - np.float64(centre), axis=1).min() < radius + 0.15 for centre, radius in balls): continue      # (0.15: 0.1 and the grid's spacing)
        out.append(t)
    return np.float32(out)


def _point(pos, power, ident="p"):
    from adapt_amd.emitters import SOURCE_MAP
    import xml.etree.ElementTree as xet
    return SOURCE_MAP["point"](xet.fromstring(f'<emitter type="point" id="{ident}"><rgb name="emission" value="{power}, {power}, {power}"/>'
                                              f'<point name="center" x="{pos[0]}" y="{pos[1]}" z="{pos[2]}"/></emitter>'))


def _area(power, ident):
    from adapt_amd.emitters import SOURCE_MAP
    import xml.etree.ElementTree as xet
    return SOURCE_MAP["area"](xet.fromstring(f'<emitter type="area" id="{ident}"><rgb name="emission" value="{power}, {power}, {power}"/></emitter>'))


class _Palette:
    """the materials of a variant: `of(role, k)` -> material of the k-th object of a role (wall, box, ball, shard, quad, twin).
    `lean` is the variant that also runs on the tree (over_by_one), whose product-build leaf test lets the first face tested win between
    two faces at the same distance where the flat sweep reproduces the reference's choice (traverse.hpp walk_scalar_test, flat_tie_break):
    there the two faces of a coplanar group share a material, in every other variant they differ - so the image tells which one won."""
    def __init__(self, variant):
        from adapt_amd import synth
        assert variant in VARIANTS, variant
        self.variant = variant
        lam = lambda c: synth._brdf("lambertian", c)
        self.walls = [lam(c) for c in _WALL_COLOURS]
        self.diffuse = [lam(c) for c in ("#BDBDBD", "#C8B496", "#9696C8", "#E0C080")]
        self.glass = synth._glass()
        self.mirror = synth._brdf("specular", "#DEDEDE")
        self.phong = synth._brdf("phong", "#BCBCBC", "8.0", "#303030")
        # (not Oren-Nayar: with it in the `sorted` variant the oracle's own render of the mixed room had 11 pixels of negative radiance,
        # down to -37.7 - the reference's behaviour - and sums that cancel are no basis for a comparison to a few ulp)
        self.glossy = synth._mat('<brdf type="mod-phong" id="mp"><rgb name="k_d" value="#BCBCBC"/><rgb name="k_g" value="10.0"/><rgb name="k_s" value="#424242"/></brdf>')
        self.light = lam("#555555")

    def of(self, role, k):
        v = self.variant
        if role == "wall": return self.walls[k]
        if role == "twin":                               # the k-th pair of overlapping coplanar faces, member m = 0, 1
            k, m = k
            return self.diffuse[(1 + k) % 4] if v == "lean" else self.diffuse[(3 * m + 2 * k) % 4]
        if v == "delta":
            if role == "box": return self.glass
            if role == "ball" and k == 0: return self.mirror
            if role == "shard" and k % 9 == 4: return self.mirror if k % 2 else self.glass     # (the all-triangle scene has neither box nor ball)
        if v == "sorted":
            if role == "box": return self.phong
            if role == "ball": return (self.mirror, self.glossy, self.phong)[k % 3]
            if role == "shard" and k % 3 == 1: return self.phong if k % 2 else self.glossy
        return self.diffuse[k % len(self.diffuse)]


def _finish(b, variant, lights, emitters):
    """sensor, camera and world of a variant; `lights`: the point lights of the variants that are lit by them, `emitters`: the area
    emitters already attached to objects (variant `sorted`)"""
    from adapt_amd import synth
    from adapt_amd.parsers.world import World_np
    import xml.etree.ElementTree as xet
    bounce, nshadow = {"lean": (6, 1), "delta": (8, 1), "sorted": (6, 4), "volumetric": (6, 1)}[variant]
    tup = b.finish(emitters if variant == "sorted" else lights, synth._sensor(64, 64, bounce, nshadow))
    prop = tup[3]
    prop["transform"] = (np.float32(CAMERA[0]), np.float32(CAMERA[1]), None)
    prop["fov"] = FOV
    if variant == "volumetric":
        prop["world"] = World_np(xet.fromstring('<world><medium type="hg"><rgb name="u_a" value="0.02"/><rgb name="u_s" value="0.12"/>'
                                                '<rgb name="par" value="0.0"/><float name="ior" value="1.0"/></medium></world>'))
    return tup


def _attach(b, emitter_index, sphere=False):
    """make the builder's last object the shape of area emitter `emitter_index`"""
    from adapt_amd.parsers.obj_loader import calculate_surface_area
    obj = b.objs[-1]
    obj.emitter_ref_id = emitter_index
    b.area_of[emitter_index] = calculate_surface_area(obj.meshes, 1 if sphere else 0)


def _zero_area(b, material):
    tri = np.float32([_ZERO_AREA])
    up = np.float32([[0, 1, 0]])
    with np.errstate(invalid="ignore"):
        b.mesh(tri, material, vns=np.repeat(up[:, None, :], 3, axis=1))
    b.ng[-1][:] = up                                     # (its geometric normal is 0 / 0; nothing can hit it, nothing may read a NaN)


LIGHT_POS = (2.75, 4.75, 2.25)


def capacity_mixed(variant="lean", lights=None):
    """96 primitives in every section of the stream, each section with an odd tail:
        parallelograms  11 + 2 in a coplanar group (the floor and the bottom of the box resting on it)    13 records, 26 primitives
        convex quads     3 + 2 in a coplanar group (two overlapping shelves)                               5 records, 10 primitives
        triangles       55 (one of zero area) + 2 in a coplanar group (two overlapping shards)            57 records
        spheres          3, all left of the camera: the strips to its right see none                       3 records
    7 + 3 + 29 + 2 = 41 pairs.  `lights`: point lights instead of the variant's own (many_lights)."""
    from adapt_amd import synth
    pal = _Palette(variant)
    b = synth._Builder()
    emitters = [_area(30.0, "panel"), _area(40.0, "ball")]
    for k, (p0, e1, e2, n) in enumerate(_WALLS): b.mesh(_para(p0, e1, e2, n), pal.of("wall", k))
    b.mesh(_box((3.5, 0.0, 3.0), (4.75, 1.5, 4.25)), pal.of("box", 0))                                # rests on the floor
    b.mesh(_para((1.75, 5.0, 2.0), (1.5, 0, 0), (0, 0, 1.0), (0, -1, 0)), pal.light if variant == "sorted" else pal.of("quad", 1))      # a panel under the ceiling
    if variant == "sorted": _attach(b, 0)
    quads = [[(2.5, 2.0, 1.5), (3.5, 2.0, 1.5), (3.75, 2.0, 2.5), (2.5, 2.0, 2.25)],                  # in y = 2
             [(5.0, 2.5, 3.0), (5.0, 2.5, 4.0), (5.0, 3.75, 4.25), (5.0, 3.25, 3.0)],                 # in x = 5
             [(1.75, 3.0, 4.0), (2.75, 3.0, 4.0), (3.0, 4.0, 5.0), (1.75, 3.5, 4.5)],                 # in z = y + 1
             [(2.0, 1.0, 3.5), (2.75, 1.0, 3.5), (3.0, 1.0, 4.25), (2.0, 1.0, 4.0)],                  # two shelves in y = 1 that overlap
             [(2.5, 1.0, 3.75), (3.25, 1.0, 3.75), (3.375, 1.0, 4.75), (2.5, 1.0, 4.5)]]
    for k, q in enumerate(quads): b.mesh(_quad(q), pal.of("quad", k) if k < 3 else pal.of("twin", (0, k - 3)))
    balls = [((0.875, 0.75, 4.25), 0.5), ((1.0, 2.25, 3.0), 0.375), ((0.75, 3.75, 4.5), 0.3125)]
    shards = _shards(54, 96, (0.5, 0.4, 1.25), (5.0, 5.0, 5.0), balls)
    for k, t in enumerate(shards[:27]): b.mesh(t[None], pal.of("shard", k))
    _zero_area(b, pal.of("shard", 0))
    for k, t in enumerate(shards[27:]): b.mesh(t[None], pal.of("shard", 27 + k))
    b.mesh(np.float32([[(2.0, 0.5, 1.0), (2.0, 1.25, 1.0), (2.0, 0.5, 1.75)]]), pal.of("twin", (1, 0)))     # two shards in x = 2 that overlap
    b.mesh(np.float32([[(2.0, 0.75, 1.25), (2.0, 1.5, 1.25), (2.0, 0.75, 2.0)]]), pal.of("twin", (1, 1)))
    for k, (c, r) in enumerate(balls):
        b.sphere(c, r, pal.light if (variant == "sorted" and k == 2) else pal.of("ball", k))
        if variant == "sorted" and k == 2: _attach(b, 1, sphere=True)
    return _finish(b, variant, lights or [_point(LIGHT_POS, 40.0)], emitters)


def capacity_tris(variant="lean"):
    """96 triangles, one per object, so none is merged: 96 triangle records, 48 pairs.  The walls are two single-triangle objects each.
    (`sorted` puts its emitter, a triangle under the ceiling, in the first shard's place.)"""
    from adapt_amd import synth
    pal = _Palette(variant)
    b = synth._Builder()
    emitters = [_area(60.0, "shard")]
    for k, (p0, e1, e2, n) in enumerate(_WALLS):
        for t in _para(p0, e1, e2, n): b.mesh(t[None], pal.of("wall", k))
    shards = _shards(84, 48, (0.5, 0.4, 1.25), (5.0, 5.0, 5.0))
    for k, t in enumerate(shards):
        lit = variant == "sorted" and k == 0
        if lit: t = np.float32([(2.25, 5.0, 2.0), (3.25, 5.0, 2.0), (2.25, 5.0, 3.0)])                 # facing down, under the ceiling
        b.mesh(t[None], pal.light if lit else pal.of("shard", k))
        if lit: _attach(b, 0)
    return _finish(b, variant, [_point(LIGHT_POS, 40.0)], emitters)


def over_by_one(tup):
    """a capacity scene plus one triangle behind the back wall of the closed room, where no ray gets: 97 primitives"""
    from adapt_amd import synth
    from adapt_amd.parsers.obj_desc import ObjDescriptor
    em, arr, objs, prop = tup
    tri = np.float32([[(1.0, 1.0, 7.0), (2.0, 1.0, 7.0), (1.0, 2.0, 7.0)]])
    ng = synth._geo_normals(tri); vns = np.repeat(ng[:, None, :], 3, axis=1)
    arr = dict(arr, primitives=np.concatenate([arr["primitives"], tri]), n_g=np.concatenate([arr["n_g"], ng]), n_s=np.concatenate([arr["n_s"], vns]),
               uvs=np.concatenate([arr["uvs"], np.zeros((1, 3, 2), np.float32)]))
    extra = ObjDescriptor(tri, ng, objs[0].bsdf, vns, None, {"albedo": None, "normal": None, "bump": None, "roughness": None}, None, None, -1, 0)
    return em, arr, list(objs) + [extra], prop


def many_lights(n):
    """capacity_mixed("lean") under n point lights on a ring below the ceiling: 16 is the last count that gets light-strip rows
    (bvh_build.hpp APT_LIGHT_STRIP_EMITTERS), 17 the first that does not"""
    ring = [(2.75 + 1.5 * np.cos(2 * np.pi * k / n), 4.75, 2.5 + 1.5 * np.sin(2 * np.pi * k / n)) for k in range(n)]
    return capacity_mixed("lean", lights=[_point(tuple(round(float(c) * 64) / 64 for c in p), 40.0 / n, f"p{k}") for k, p in enumerate(ring)])


CAPACITY_SCENES = {"capacity_mixed": capacity_mixed, "capacity_tris": capacity_tris}
_capacity_cache = {}


def capacity(name, variant="lean"):
    """-> (the 4-tuple `scene_parsing` returns, its packed scene), built once per session; treat both as read-only"""
    from adapt_amd.scene_pack import pack_scene
    key = (name, variant)
    if key not in _capacity_cache:
        tup = CAPACITY_SCENES[name](variant)
        _capacity_cache[key] = (tup, pack_scene(*tup))
    return _capacity_cache[key]
