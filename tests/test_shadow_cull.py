"""Occluder lists of the light samples (csrc/flat_build.cpp flat_occluders, reached through apt_flat_occluders) checked on
the CPU: which records the rule leaves out of an emitter's list on the packed C2 scene, where it refuses to leave any out, and - with a
numpy float32 restatement of flat_any1's arithmetic (traverse.hpp) - that a left-out record never blocks a shadow ray, also from origins
pushed to the wrong side of its plane by as much as the rule allows."""
import ctypes as C

import numpy as np
import pytest

from adapt_amd import _lib
from flat_cases import _fma, flat_records, sections

C2_NAMES = ["floor", "ceiling", "back", "green", "red", "smallbox", "largebox"]


def occluders(prims, obj_info, src_i, src_f, cull=1):
    lib = _lib.load()
    prims = np.ascontiguousarray(prims, np.float32).reshape(-1, 9); obj_info = np.ascontiguousarray(obj_info, np.int32).reshape(-1, 3)
    src_i = np.ascontiguousarray(src_i, np.int32).reshape(-1, 4); src_f = np.ascontiguousarray(src_f, np.float32).reshape(-1, 11)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)); ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    ns, nr, npairs = src_i.shape[0], C.c_int32(0), C.c_int32(0)
    args = (fp(prims), prims.shape[0], ip(obj_info), obj_info.shape[0], ip(src_i), fp(src_f), ns, cull)
    _lib.check(lib.apt_flat_occluders(*args, None, None, 0, None, 0, C.byref(nr), C.byref(npairs)), "apt_flat_occluders", lib)
    table, keep, pairs = np.zeros(ns * 8, np.int32), np.zeros(ns * nr.value, np.int32), np.zeros(npairs.value, np.float32)
    _lib.check(lib.apt_flat_occluders(*args, ip(table), ip(keep), keep.size, fp(pairs), pairs.size, C.byref(nr), C.byref(npairs)), "apt_flat_occluders", lib)
    return table.reshape(ns, 8), keep.reshape(ns, nr.value).astype(bool), pairs


def record_prims(prims, obj_info):
    counts, stream, tab = flat_records(prims, obj_info)
    ids = tab.reshape(-1, 28)[:, 8:10].copy().view(np.int32)
    return counts, stream, ids


def pair_up(stream, counts, keep):
    """flat_pairs() of the kept records, in numpy"""
    out = []
    recs = sections(counts)
    for sec, w in enumerate((12, 18, 12, 4)):
        mine = [stream[at:at + w] for r, (s, at) in enumerate(recs) if s == sec and keep[r]]
        for j in range(0, len(mine), 2):
            a = mine[j]; b = mine[j + 1] if j + 1 < len(mine) else a
            out.append(np.stack([a, b], 1).reshape(-1))
    return np.concatenate(out) if out else np.zeros(1, np.float32)


def test_c2_leaves_out_the_walls_and_the_box_bottoms(flat):
    fs = flat("cbox")
    counts, stream, ids = record_prims(fs.prims, fs.obj_info)
    assert (counts[0] + counts[1], counts[2] + counts[3], counts[4] + counts[5], counts[6]) == (10, 6, 2, 0)
    table, keep, pairs = occluders(fs.prims, fs.obj_info, fs.src_i, fs.src_f)
    obj_of = np.repeat(np.arange(fs.obj_info.shape[0]), fs.obj_info[:, 1])
    culled = sorted((C2_NAMES[obj_of[ids[r, 0]]], int(ids[r, 0])) for r in np.flatnonzero(~keep[0]))
    # the floor, back, green and red walls can never block the light; nor can the bottoms of the two blocks (coplanar with the floor).
    # The ceiling could not either, but 0.99 above the light its bound, 5.6e-5 by the rule's worst-case rounding, is above half the floor.
    assert culled == [("back", 4), ("floor", 0), ("green", 6), ("largebox", 32), ("red", 8), ("red", 9), ("smallbox", 20)], culled
    kept = sorted({C2_NAMES[obj_of[ids[r, 0]]] for r in np.flatnonzero(keep[0])})
    assert kept == ["ceiling", "largebox", "smallbox"]
    assert keep[0].sum() == 11 and table[0, :5].tolist() == [0, 9, 2, 0, 0]
    np.testing.assert_array_equal(pairs, pair_up(stream, counts, keep[0]))
    # APT_SHADOW_CULL=0: the full stream
    table0, keep0, pairs0 = occluders(fs.prims, fs.obj_info, fs.src_i, fs.src_f, cull=0)
    assert keep0.all() and table0[0, :5].tolist() == [0, 10, 6, 2, 0]
    np.testing.assert_array_equal(pairs0, pair_up(stream, counts, keep0[0]))


def _c2_with_light(fs, pos):
    src_f = fs.src_f.copy(); src_f[0, 6:9] = pos
    return src_f


def _kept_objects(fs, src_f):
    _, _, ids = record_prims(fs.prims, fs.obj_info)
    _, keep, _ = occluders(fs.prims, fs.obj_info, fs.src_i, src_f)
    obj_of = np.repeat(np.arange(fs.obj_info.shape[0]), fs.obj_info[:, 1])
    return {C2_NAMES[obj_of[ids[r, 0]]] for r in np.flatnonzero(keep[0])}, {C2_NAMES[obj_of[ids[r, 0]]] for r in np.flatnonzero(~keep[0])}


def test_refuses_a_light_outside_the_room(flat):
    fs = flat("cbox")
    kept, _ = _kept_objects(fs, _c2_with_light(fs, (2.779, 7.0, 3.0)))          # above the ceiling
    assert "ceiling" in kept
    kept, _ = _kept_objects(fs, _c2_with_light(fs, (2.779, 3.0, 7.0)))          # behind the back wall
    assert "back" in kept


@pytest.mark.parametrize("y", [0.0, 1e-6, -1e-6, 2e-5])
def test_refuses_a_light_on_or_next_to_a_plane(flat, y):
    fs = flat("cbox")
    ymin = float(fs.prims.reshape(-1, 3, 3)[fs.obj_info[0, 0]:fs.obj_info[0, 0] + 2, :, 1].min())
    kept, culled = _kept_objects(fs, _c2_with_light(fs, (2.779, ymin + y, 3.0)))
    assert "floor" in kept, culled


def _quad(p0, e1, e2):
    p0, e1, e2 = (np.asarray(x, np.float32) for x in (p0, e1, e2))
    return [np.concatenate([p0, p0 + e1, p0 + e1 + e2]), np.concatenate([p0, p0 + e1 + e2, p0 + e2])]


@pytest.mark.parametrize("poke", [False, True])
def test_refuses_a_plane_with_geometry_on_both_sides(poke):
    """a floor and a triangle beside it: culled while the triangle stays above the floor's plane, kept once it reaches below it"""
    tri = np.float32([6, 0.5, 0, 7, 2, 0, 6.5, 0.5 if not poke else -0.5, 1])
    prims = np.stack(_quad((0, 0, 0), (4, 0, 0), (0, 0, 4)) + [tri])
    obj_info = np.int32([[0, 2, 0], [2, 1, 0]])
    src_i = np.int32([[0, 0, -1, 0]]); src_f = np.float32([[1, 1, 1, 0, 0, 0, 2, 3, 2, 0, 0]])
    _, keep, _ = occluders(prims, obj_info, src_i, src_f)
    counts, _, ids = record_prims(prims, obj_info)
    floor = [r for r in range(ids.shape[0]) if ids[r, 0] in (0, 1)]
    assert keep[0, floor].all() == poke


# ---- no left-out record ever blocks: flat_any1's float32 arithmetic in numpy

def _blocks(rec, sec, o, d, lim):
    """flat_blocks() of flat_any1's test of one record, float32 as the kernel (FMA chains, a reciprocal): -> bool per ray"""
    f = np.float32
    r = rec.astype(np.float32)
    s = (o - r[0:3]).astype(np.float32)
    t_o = _fma(r[9], s[:, 0], _fma(r[10], s[:, 1], r[11] * s[:, 2]))
    t_d = _fma(r[9], d[:, 0], _fma(r[10], d[:, 1], r[11] * d[:, 2]))
    with np.errstate(all="ignore"):
        inv = (f(1) / t_d).astype(np.float32)
        t = (-t_o * inv).astype(np.float32)
        p = [_fma(t, d[:, k], s[:, k]) for k in range(3)]
        u = _fma(r[3], p[0], _fma(r[4], p[1], r[5] * p[2]))
        v = _fma(r[6], p[0], _fma(r[7], p[1], r[8] * p[2]))
        if sec == 0: inside = np.maximum(np.abs(u - f(0.5)), np.abs(v - f(0.5))) <= f(0.5)
        elif sec == 2: inside = np.minimum(np.minimum(u, v), (f(1) - u) - v) >= 0
        else:
            e1 = _fma(r[12], u, _fma(r[13], v, r[14])); e2 = _fma(r[15], u, _fma(r[16], v, r[17]))
            inside = np.minimum(np.minimum(u, v), np.minimum(e1, e2)) >= 0
        return inside & (t > f(1e-4)) & (t < lim)


def _points_on(prims, ids, rs, n):
    """random points on the triangles of every planar record (or on the sphere)"""
    out = []
    for k in ids:
        if k < 0: continue
        a, b, c = prims[k].reshape(3, 3).astype(np.float64)
        x, y = rs.uniform(size=(2, n))
        flip = x + y > 1; x[flip], y[flip] = 1 - x[flip], 1 - y[flip]
        out.append(a + x[:, None] * (b - a) + y[:, None] * (c - a))
    return np.concatenate(out)


def _light_points(fs, e, rs, n):
    t = fs.src_i[e, 0]
    if t in (0, 2): return np.repeat(fs.src_f[e, 6:9][None].astype(np.float64), n, 0)
    first, cnt, _ = fs.obj_info[fs.src_i[e, 2]]
    tri = rs.randint(first, first + cnt, size=n)
    return np.concatenate([_points_on(fs.prims.reshape(-1, 9), [k], rs, 1) for k in tri])


def test_the_capacity_scene_s_occluder_list_reaches_the_upper_half_of_a_strip_word():
    """capacity_mixed under its point light: the rule leaves out the floor, the bottom of the box resting on it and the back wall (the
    other walls are nearer to the light than its worst-case rounding allows, as the Cornell box's ceiling above).  What stays is 39 pairs,
    so the light-strip masks over this list (tests/test_light_strips.py) have bits at 32 and above to set and clear."""
    from flat_cases import capacity
    _, fs = capacity("capacity_mixed")
    counts, stream, ids = record_prims(fs.prims, fs.obj_info)
    table, keep, pairs = occluders(fs.prims, fs.obj_info, fs.src_i, fs.src_f)
    assert fs.src_i.shape[0] == 1 and fs.src_i[0, 0] == 0                            # one point light
    kept = table[0, 1:5]
    n_pairs = int(((kept + 1) // 2).sum())
    assert n_pairs >= 33 and kept.sum() == keep[0].sum(), (kept, n_pairs)
    assert kept.tolist() == [10, 5, 57, 3] and n_pairs == 39                        # (three of its sections end in a lone record)
    obj_of = np.repeat(np.arange(fs.obj_info.shape[0]), fs.obj_info[:, 1])
    assert sorted(int(obj_of[ids[r, 0]]) for r in np.flatnonzero(~keep[0])) == [0, 2, 6]      # floor, back wall, box
    np.testing.assert_array_equal(pairs, pair_up(stream, counts, keep[0]))


@pytest.mark.parametrize("tag", ["cbox", "glass_box", "features_c", "capacity_mixed", "capacity_tris"])
def test_left_out_records_never_block(tag, flat):
    from flat_cases import CAPACITY_SCENES, capacity
    fs = capacity(tag)[1] if tag in CAPACITY_SCENES else flat(tag)
    prims = fs.prims.reshape(-1, 9)
    counts, stream, ids = record_prims(prims, fs.obj_info)
    _, keep, _ = occluders(prims, fs.obj_info, fs.src_i, fs.src_f)
    recs = sections(counts)
    rs = np.random.RandomState(5)
    planar = [r for r in range(len(recs)) if recs[r][0] < 3]
    n_checked = n_sensitive = 0
    for e in range(fs.src_i.shape[0]):
        for R in np.flatnonzero(~keep[e]):
            sec, at = recs[R]; rec = stream[at:at + (12, 18, 12)[sec]]
            T, P = rec[9:12].astype(np.float64), rec[0:3].astype(np.float64)
            o = np.concatenate([_points_on(prims, ids[r], rs, 400) for r in planar])
            L = _light_points(fs, e, rs, o.shape[0])
            sgn = np.sign(((L - P) @ T).mean())
            # the most the rule lets an origin sit on the wrong side (its bound: crossing at t <= 0.5e-4), and 200 times that
            delta = (sgn * ((L - P) @ T)).min(); maxdist = np.linalg.norm(L - o, axis=1).max()
            push_max = 0.5e-4 * delta / maxdist
            for scale, expect_none in ((1.0, True), (200.0, False)):
                h = sgn * ((o - P) @ T)
                near = np.abs(h) < 1e-3                     # origins on R or on a record that meets its plane: pushed below it
                oo = (o - (sgn * T)[None] * (rs.uniform(0, push_max * scale, size=o.shape[0]) * near)[:, None]).astype(np.float32)
                to = (L.astype(np.float32) - oo).astype(np.float32)
                dist = np.sqrt((to.astype(np.float64) ** 2).sum(1)).astype(np.float32)
                d = (to / dist[:, None]).astype(np.float32)
                lim = np.where(dist > 0, dist - np.float32(1e-4), np.float32(1e7)).astype(np.float32)
                b = _blocks(rec, sec, oo, d, lim)
                if expect_none:
                    assert not b.any(), (tag, e, int(R), int(b.sum()))
                    n_checked += o.shape[0]
                else: n_sensitive += int(b.any())
    assert n_checked > 0
    assert n_sensitive > 0          # pushed far enough, the same records do block: the restatement can see a block
