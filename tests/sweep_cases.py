"""Scenes and ray batches that put the reference-order sweeps of csrc/traverse.hpp - the wave sweep `sweep_wg`, the tiled sweep
`sweep_tile`, the plain loop `sweep` the tile's redo falls back on - at their list, LDS and key limits (tests/test_sweep_cases_host.py
proves on the CPU that they get there; tests/test_gpu_sweep_limits.py runs them on the device).  Not collected by pytest (no `test_`
prefix); nothing here needs a device.

  tile_34     34 objects, 75 primitives: the last object count whose per-object lists fit the CU's LDS at 512 threads (api.hip
              pick_traversal) - the exact build takes the tile by itself.  A 12-triangle box, fans of 5, 6 and 7 triangles (both sides
              of APT_SWEEP_LIST_MIN, odd pair tails), spheres between the meshes, lone triangles and quads.
  tile_35     tile_34 and one lone triangle: the first object count that must take the wave sweep.
  lists_130   the room and 142 objects of six or more triangles: 128 small ones on a lattice at the back of the room, then - past
              APT_SWEEP_MAX_LISTS - fourteen large ones in the middle, where the rays are; spheres and small objects in between.
  keys_16     the room and four bunnies, 55 452 primitives: every primitive from 32 768 on has bit 15 of the tile's reduction key set.
  ties        the room and seven stacks of four parallel quads, each quad an object: coincident, 2^-20 .. 2^-17 apart, tilted against
              each other by 1e-5 - the tile's redo rule fires on every ray that meets a stack first.

Geometry as in tests/flat_cases.py: a closed room of 5.5 units, coordinates on multiples of 1/64 wherever planarity matters, fixed seeds."""
import numpy as np

from flat_cases import ROOM, _WALLS, _box, _finish, _Palette, _para, _point, _quad, _shards

SWEEP_LIST_MIN = 6              # traverse.hpp APT_SWEEP_LIST_MIN: objects of fewer primitives get no LDS work list
SWEEP_MAX_LISTS = 128           # traverse.hpp APT_SWEEP_MAX_LISTS
TILE_NT, BLOCK = 512, 256       # stages.hpp APT_TILE_NT, the wave sweep's workgroup
N_RANDOM = 4099
PREFIXES = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025)
N_AIMED = 1024                  # two tiles of 512 rays, four workgroups of 256
LIGHT_POS = (2.75, 4.75, 2.25)


def tile_lds_bytes(nt, n_obj):
    """traverse.hpp APT_TILE_LDS_BYTES"""
    return nt * 40 + n_obj * (nt * 8 + 4) + 16


def _fan(centre, axis, radius, n):
    """n triangles around `centre` in the plane perpendicular to `axis`, the ring on the 1/64 grid: one planar object"""
    c = np.float64(centre)
    a, b = (axis + 1) % 3, (axis + 2) % 3
    ring = np.tile(c, (n, 1))
    ang = 2 * np.pi * (np.arange(n) + 0.25) / n
    ring[:, a] += np.round(radius * np.cos(ang) * 64) / 64
    ring[:, b] += np.round(radius * np.sin(ang) * 64) / 64
    tris = np.float32([[c, ring[i], ring[(i + 1) % n]] for i in range(n)])
    assert np.linalg.norm(np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]), axis=1).min() > 1e-4
    return tris


def _walls(b, pal):
    for k, (p0, e1, e2, n) in enumerate(_WALLS): b.mesh(_para(p0, e1, e2, n), pal.of("wall", k))


# ---------------------------------------------------------------- tile_34, tile_35
_TILE_BALLS = [((1.0, 0.75, 4.25), 0.5), ((4.5, 3.75, 4.5), 0.375), ((0.875, 3.5, 2.5), 0.3125)]
_TILE_QUADS = [[(2.5, 2.0, 1.5), (3.5, 2.0, 1.5), (3.75, 2.0, 2.5), (2.5, 2.0, 2.25)],                  # in y = 2
               [(5.0, 2.5, 3.0), (5.0, 2.5, 4.0), (5.0, 3.75, 4.25), (5.0, 3.25, 3.0)],                 # in x = 5
               [(1.75, 3.0, 4.0), (2.75, 3.0, 4.0), (3.0, 4.0, 5.0), (1.75, 3.5, 4.5)],                 # in z = y + 1
               [(2.0, 1.0, 3.5), (2.75, 1.0, 3.5), (3.0, 1.0, 4.25), (2.0, 1.0, 4.0)],                  # in y = 1
               [(0.5, 4.5, 1.5), (1.5, 4.5, 1.5), (1.5, 4.5, 2.5), (0.5, 4.5, 2.25)],                   # in y = 4.5
               [(3.0, 0.5, 1.25), (4.0, 0.5, 1.25), (4.25, 1.25, 1.25), (3.0, 1.5, 1.25)],              # in z = 1.25
               [(0.5, 1.5, 1.5), (0.5, 2.5, 1.5), (0.5, 2.75, 2.5), (0.5, 1.5, 2.25)],                  # in x = 0.5
               [(3.5, 4.0, 2.0), (4.5, 4.0, 2.0), (4.5, 4.0, 3.0), (3.5, 4.0, 2.75)],                   # in y = 4
               [(2.0, 3.25, 1.0), (3.0, 3.25, 1.0), (3.0, 4.0, 1.0), (2.0, 4.25, 1.0)]]                 # in z = 1


def tile_34(extra=0, volumetric=False):
    """-> the 4-tuple scene_parsing returns.  Scene order: walls 0-5, triangle, the box, sphere, fan of 5, fan of 6, quad, fan of 7,
    sphere, then triangles and quads in turn with the third sphere among them.  `extra`: lone triangles appended (tile_35: one).
    volumetric: the box is a null-surface pane holding a scattering medium, in a scattering world (tests/null_stack_cases.py
    front_stack, its `scatter` pane and its `world`): a light sample through the pane walks three segments."""
    from adapt_amd import synth
    pal = _Palette("lean")
    b = synth._Builder()
    _walls(b, pal)
    shards = _shards(12 + extra, 34, (0.5, 0.4, 1.25), (5.0, 5.0, 5.0), _TILE_BALLS)
    b.mesh(shards[0][None], pal.of("shard", 0))
    if volumetric:
        import null_stack_cases as ns
        b.mesh(ns.box((3.5, 0.25, 3.0), (4.75, 1.5, 4.25)), ns._null((0.05, 0.1, 0.2), (0.5, 0.4, 0.3), 0.4))
    else:
        b.mesh(_box((3.5, 0.25, 3.0), (4.75, 1.5, 4.25)), pal.of("box", 0))
    b.sphere(*_TILE_BALLS[0], pal.of("ball", 0))
    b.mesh(_fan((1.5, 2.5, 3.5), 2, 0.75, 5), pal.of("quad", 1))
    b.mesh(_fan((4.0, 2.75, 3.75), 0, 0.75, 6), pal.of("quad", 2))
    b.mesh(_quad(_TILE_QUADS[0]), pal.of("quad", 0))
    b.mesh(_fan((2.75, 0.75, 2.75), 1, 0.875, 7), pal.of("quad", 3))
    b.sphere(*_TILE_BALLS[1], pal.of("ball", 1))
    for k in range(1, 9):
        b.mesh(shards[k][None], pal.of("shard", k))
        b.mesh(_quad(_TILE_QUADS[k]), pal.of("quad", k))
        if k == 4: b.sphere(*_TILE_BALLS[2], pal.of("ball", 2))
    for k in range(9, 12 + extra): b.mesh(shards[k][None], pal.of("shard", k))
    tup = _finish(b, "lean", [_point(LIGHT_POS, 40.0)], [])
    if volumetric:
        import xml.etree.ElementTree as xet
        from adapt_amd.parsers.world import World_np
        tup[3]["world"] = World_np(xet.fromstring('<world name="w"><medium type="hg"><rgb name="u_a" value="0.01"/><rgb name="u_s" r="0.04" g="0.05" b="0.06"/>'
                                                  '<rgb name="par" value="0.5"/><float name="ior" value="1.0"/></medium></world>'))
    return tup


def tile_35():
    return tile_34(extra=1)


# ---------------------------------------------------------------- lists_130
def lists_130():
    """Scene order: walls; 128 listed objects (boxes of side 1/4, every seventh a fan of 6, 7 or 9 triangles) on an 8 x 4 x 4 lattice in
    z >= 3.25, with a sphere after every 20th and a lone triangle after every 17th; then fourteen listed objects - boxes of side 3/4 and
    fans of radius 1/2 - in 0.75 <= z <= 2.75, with a quad, a sphere, a fan of 5 and a lone triangle among them.  Random rays start
    anywhere in the room: the large objects past the 128th list are what they meet most often."""
    from adapt_amd import synth
    pal = _Palette("lean")
    b = synth._Builder()
    _walls(b, pal)
    k = 0
    for iz in range(4):
        for iy in range(4):
            for ix in range(8):
                c = np.float64((0.5 + 0.625 * ix, 0.625 + 1.25 * iy, 3.375 + 0.5 * iz))
                if k % 7 == 3: b.mesh(_fan(c, k % 3, 0.125, (6, 7, 9)[(k // 7) % 3]), pal.of("quad", k))
                else: b.mesh(_box(c - 0.125, c + 0.125), pal.of("shard", k))
                k += 1
                if k % 20 == 0: b.sphere(tuple(c + (0.3125, 0.0, 0.0)), 0.125, pal.of("ball", k))
                if k % 17 == 0: b.mesh(np.float32([[c + (0.0, 0.25, 0.0), c + (0.25, 0.5, 0.0), c + (0.0, 0.5, 0.125)]]), pal.of("shard", k))
    assert k == SWEEP_MAX_LISTS
    big = 0
    for iy in range(2):
        for ix in range(4):
            for iz in range(2):
                if (ix + iy + iz) % 4 == 3: continue
                c = np.float64((0.875 + 1.25 * ix, 1.25 + 2.5 * iy, 1.125 + 1.25 * iz))
                if big % 3 == 2: b.mesh(_fan(c, (big // 3) % 3, 0.5, (6, 7, 9)[(big // 3) % 3]), pal.of("quad", big))
                else: b.mesh(_box(c - 0.375, c + 0.375), pal.of("shard", big))
                big += 1
                if big == 2: b.mesh(_quad([c + (0.5, -0.5, 0.0), c + (0.75, -0.5, 0.0), c + (0.75, 0.5, 0.0), c + (0.5, 0.25, 0.0)]), pal.of("quad", 0))
                if big == 5: b.sphere(tuple(c + (0.0, 0.75, 0.0)), 0.25, pal.of("ball", 0))
                if big == 8: b.mesh(_fan(c + (0.0, -0.75, 0.0), 1, 0.375, 5), pal.of("quad", 1))
                if big == 11: b.mesh(np.float32([[c + (0.5, 0.0, 0.0), c + (0.75, 0.5, 0.0), c + (0.5, 0.5, 0.25)]]), pal.of("shard", 1))
    for c in ((3.5, 2.5, 1.75), (1.5, 2.5, 2.875)):                                                   # two fans between the layers of boxes
        b.mesh(_fan(c, 2, 0.5, 7), pal.of("quad", 2)); big += 1
    assert big == 14
    return _finish(b, "lean", [_point(LIGHT_POS, 40.0)], [])


# ---------------------------------------------------------------- keys_16
def keys_16():
    """The room, two bunnies of subdivision level 2 (7 920 triangles each), one of level 3 (31 680: primitives 15 852 .. 47 531) in the
    middle of the room, one more of level 2 (47 532 .. 55 451): 10 objects, 55 452 primitives."""
    from adapt_amd import synth
    pal = _Palette("lean")
    b = synth._Builder()
    _walls(b, pal)
    l2, l3 = synth._bunny(2), synth._bunny(3)
    b.mesh(synth._place(l2, 0.3, (1.0, 0.0, 4.25)), pal.of("shard", 0))
    b.mesh(synth._place(l2, 0.3, (4.5, 0.0, 4.25)), pal.of("shard", 1))
    b.mesh(synth._place(l3, 1.2, (2.75, 0.0, 3.0)), pal.of("shard", 2))
    b.mesh(synth._place(l2, 0.6, (1.25, 0.0, 1.75)), pal.of("shard", 3))
    return _finish(b, "lean", [_point(LIGHT_POS, 40.0)], [])


# ---------------------------------------------------------------- ties
_TIE_STACKS = [  # (axis n of the normal, plane coordinate, lower corner along axes n + 1 and n + 2 (mod 3), side, how the four quads differ)
    (2, 4.0, (0.5, 0.5), 3.5, ("offset", 0.0)),                  # coincident
    (2, 3.0, (1.75, 0.25), 3.5, ("offset", 2.0 ** -20)),
    (1, 3.5, (1.0, 0.5), 3.5, ("offset", 2.0 ** -17)),
    (0, 3.75, (1.75, 1.5), 3.5, ("tilt", 1e-5)),
    (2, 2.0, (1.5, 1.75), 3.5, ("offset", 2.0 ** -19)),
    (1, 1.5, (1.75, 1.75), 3.5, ("offset", 2.0 ** -18)),
    (0, 1.25, (0.5, 1.5), 3.5, ("tilt", -1e-5)),
]


def tie_stack_quads():
    """-> 28 x (2, 3, 3) float32: the quads of _TIE_STACKS, stack by stack"""
    out = []
    for axis, x, (lo_a, lo_b), side, (kind, step) in _TIE_STACKS:
        a, b = (axis + 1) % 3, (axis + 2) % 3
        for m in range(4):
            p = np.zeros((4, 3))
            p[:, a] = (lo_a, lo_a + side, lo_a + side, lo_a)
            p[:, b] = (lo_b, lo_b, lo_b + side, lo_b + side)
            p[:, axis] = x + m * step if kind == "offset" else x + m * step * (p[:, a] - lo_a)      # tilt: about the edge a = lo_a
            out.append(_quad(p))
    return out


def ties():
    from adapt_amd import synth
    pal = _Palette("lean")
    b = synth._Builder()
    _walls(b, pal)
    for k, q in enumerate(tie_stack_quads()): b.mesh(q, pal.of("quad", k))
    return _finish(b, "lean", [_point(LIGHT_POS, 40.0)], [])


SCENES = {"tile_34": tile_34, "tile_35": tile_35, "lists_130": lists_130, "keys_16": keys_16, "ties": ties}
# the modes APT_TRAVERSAL can force each scene into (api.hip pick_traversal), and what the exact build takes with nothing forced
MODES = {"tile_34": ("sweep", "tile"), "tile_35": ("sweep",), "lists_130": ("sweep",), "keys_16": ("sweep", "tile"), "ties": ("sweep", "tile")}
DEFAULT_MODE = {"tile_34": "tile", "tile_35": "sweep", "lists_130": "bvh", "keys_16": "bvh", "ties": "sweep"}
_scene_cache = {}


def scene(name, **kw):
    """-> (the 4-tuple `scene_parsing` returns, its packed scene), built once per session; treat both as read-only"""
    from adapt_amd.scene_pack import pack_scene
    key = (name, tuple(sorted(kw.items())))
    if key not in _scene_cache:
        tup = SCENES[name](**kw)
        _scene_cache[key] = (tup, pack_scene(*tup))
    return _scene_cache[key]


def listed_objects(fs):
    """the objects sweep_wg gives an LDS work list while lists last, in scene order: meshes of APT_SWEEP_LIST_MIN primitives or more"""
    info = np.int32(fs.obj_info).reshape(-1, 3)
    return np.flatnonzero((info[:, 2] == 0) & (info[:, 1] >= SWEEP_LIST_MIN))


def prim_object(fs):
    info = np.int32(fs.obj_info).reshape(-1, 3)
    return np.repeat(np.arange(len(info)), info[:, 1])


# ---------------------------------------------------------------- ray batches: (scene, seed) -> float32 o, d, tmax
def slab_pass(o, d, box, pad=0.0):
    """float64 slab test of rays (n, 3) against the boxes (m, 2, 3), each grown by `pad` on every side -> (n, m) bool: the ray's line
    from its origin onwards has a stretch of positive length inside the box.  (A zero direction component: inside the slab or not.)"""
    o, d, box = np.float64(o)[:, None, :], np.float64(d)[:, None, :], np.float64(box)[None]
    lo, hi = box[:, :, 0] - pad, box[:, :, 1] + pad
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - o) / d, (hi - o) / d
    par = d == 0
    inside = (o >= lo) & (o <= hi)
    tn = np.where(par, np.where(inside, -np.inf, np.inf), np.minimum(t0, t1)).max(axis=2)
    tf = np.where(par, np.where(inside, np.inf, -np.inf), np.maximum(t0, t1)).min(axis=2)
    return (tn < tf) & (tf > 0)


def _unit(d):
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def random_rays(fs=None, seed=7, n=N_RANDOM):
    """origins anywhere in the room, directions uniform; rays 0 .. 127 have zero direction components (infinite and NaN slabs) and
    rays 64 .. 95 start on a wall's plane, as in tests/test_gpu_parity.py test_every_traversal_mode_gives_the_same_hits_and_image"""
    rs = np.random.RandomState(seed)
    o = rs.uniform([0.1, 0.1, 0.1], [5.4, 5.3, 5.4], size=(n, 3)).astype(np.float32)
    d = rs.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:64, 1] = 0.0; d[64:128, 0] = 0.0; d[64:128, 2] = 0.0
    o[64:96, 0] = 0.0
    d[:128] /= np.linalg.norm(d[:128], axis=1, keepdims=True)
    tmax = rs.uniform(0.2, 8.0, n).astype(np.float32)
    return o, d, tmax


def aimed_rays(fs, seed, obj, n=N_AIMED):
    """origins spread over the room, every direction through a point inside object `obj`'s box (its middle half along each axis, so that
    float32 rounding of the direction leaves the ray inside): whole blocks of 256 and 512 rays need the same list"""
    rs = np.random.RandomState(seed)
    lo, hi = np.float64(fs.obj_aabb[obj][0]), np.float64(fs.obj_aabb[obj][1])
    o = rs.uniform([0.1, 0.1, 0.1], [5.4, 5.3, 5.4], size=(n, 3)).astype(np.float32)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    target = mid + rs.uniform(-0.5, 0.5, size=(n, 3)) * half
    d = _unit(target - o)
    tmax = rs.uniform(0.2, 8.0, n).astype(np.float32)
    return o, d, tmax


def away_rays(fs, seed, n=N_AIMED):
    """rays that pass no box of a listed object, not even one grown by 1/64 on every side: every work list of sweep_wg stays empty"""
    rs = np.random.RandomState(seed)
    boxes = np.float64(fs.obj_aabb)[listed_objects(fs)]
    o = rs.uniform([0.1, 0.1, 0.1], [5.4, 5.3, 5.4], size=(16 * n, 3)).astype(np.float32)
    d = _unit(rs.normal(size=(16 * n, 3)))
    tmax = rs.uniform(0.2, 8.0, 16 * n).astype(np.float32)
    keep = np.flatnonzero(~slab_pass(o, d, boxes, pad=1 / 64).any(axis=1))[:n] if len(boxes) else np.arange(n)
    assert len(keep) == n, len(keep)
    return o[keep], d[keep], tmax[keep]


# the objects `aimed` is pointed at, per scene, as positions in listed_objects(fs) (negative: from the end) - lists_130: the first list,
# the last one that gets a list (the 128th) and the first object past it
AIMED_AT = {"tile_34": (0, 1, 2), "tile_35": (0,), "lists_130": (0, SWEEP_MAX_LISTS - 1, SWEEP_MAX_LISTS), "keys_16": (2, 3), "ties": ()}


def batches(name):
    """-> {batch name: (o, d, tmax)} of a scene: `random`, its prefixes, `away`, `aimed` at each object of AIMED_AT (and, in `ties`,
    which has no listed object, at the first quad of the first three stacks); built once per session, read-only"""
    key = ("batches", name)
    if key not in _scene_cache:
        _, fs = scene(name)
        out = {"random": random_rays(fs, 7)}
        for n in PREFIXES: out[f"random[:{n}]"] = tuple(a[:n] for a in out["random"])
        out["away"] = away_rays(fs, 8)
        listed = listed_objects(fs)
        targets = [int(listed[k]) for k in AIMED_AT[name]] if name != "ties" else [6, 10, 14]
        for k, obj in enumerate(targets): out[f"aimed({obj})"] = aimed_rays(fs, 9 + k, obj)
        for v in out.values():
            for a in v: a.setflags(write=False)
        _scene_cache[key] = out
    return _scene_cache[key]


# ---------------------------------------------------------------- the oracle's answers, once per scene and batch
def oracle_scene(name, **kw):
    from oracle import binding as ob
    from adapt_amd.scene_pack import make_config
    key = ("oracle", name, tuple(sorted(kw.items())))
    if key not in _scene_cache:
        tup, fs = scene(name, **kw)
        _scene_cache[key] = ob.OracleScene(fs, make_config(tup[3]).cam_t)
    return _scene_cache[key]


def oracle_hits(name, batch):
    """-> (obj, prim, t, uv, occluded) of the oracle's brute-force intersector for a batch; computed once, read-only"""
    key = ("hits", name, batch)
    if key not in _scene_cache:
        o, d, tmax = batches(name)[batch]
        sc = oracle_scene(name)
        obj, prim, t, uv, _ = sc.intersect(o, d)
        out = (obj, prim, t, uv, sc.occluded(o, d, tmax))
        for a in out: a.setflags(write=False)
        _scene_cache[key] = out
    return _scene_cache[key]


def per_object_hits(name, o, d):
    """-> (t (rays, objects) float32, prim (rays, objects) int32 in the scene's numbering): each object's own closest hit, from one
    OracleScene per object (no hit: t = inf, prim = -1)"""
    import copy
    from oracle import binding as ob
    from adapt_amd.scene_pack import pack_scene
    (em, arr, objs, prop), fs = scene(name)
    info = np.int32(fs.obj_info).reshape(-1, 3)
    t_all, p_all = np.full((len(o), len(info)), np.inf, np.float32), np.full((len(o), len(info)), -1, np.int32)
    for k, (first, count, kind) in enumerate(info):
        sl = slice(first, first + count)
        one = {key: arr[key][sl] for key in ("primitives", "n_g", "n_s", "uvs")}
        one["indices"] = np.int64([0]) if kind else None
        sc = ob.OracleScene(pack_scene(em, one, [copy.copy(objs[k])], prop))
        _, prim, t, _, _ = sc.intersect(o, d)
        hit = prim >= 0
        t_all[hit, k], p_all[hit, k] = t[hit], prim[hit] + first
    return t_all, p_all
