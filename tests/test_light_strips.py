"""Strip masks of the camera vertex's light samples (csrc/flat_build.cpp light_strips, reached through apt_light_strips)
checked on the CPU.  For every bundled scene with flat records and the film shapes of tests/test_camera_cull.py, the camera rays of every
block of 64 local pixels (corners, edge midpoints, jittered rays with the jitter on its bounds) meet the scene in a numpy float32
restatement of flat_closest1's sweep (traverse.hpp), the hit point is made as the kernel makes it, fl(fl(d t) + o), and aimed at the
emitter's points as sample_light does; a float32 restatement of flat_any1's per-record test then runs over the emitter's FULL occluder
list, the reciprocal also moved by one ulp either way.  Every record that accepts a sample has to sit in a set pair of the block's word -
no exceptions - also from origins pushed off their records and outlines by half of what the rule allows an origin (the other half is left
to the restated hit's own rounding).  Sphere records are never left out, and a strip that sees a sphere keeps every pair."""
import ctypes as C

import numpy as np
import pytest

from adapt_amd import _lib
from flat_cases import _fma, flat_records, sections
from test_camera_cull import _EDGE, FILMS, FLAT_MAX_PRIMS, _cfg, camera_dirs, flat_scenes, local_pixels, upper_half
from test_shadow_cull import occluders

STRIP_EMITTERS = 16                     # bvh_build.hpp APT_LIGHT_STRIP_EMITTERS
RAYS_PER_FILM = 100_000                 # jittered rays of a film, spread over its blocks (at least 24, at most 2048 per block), besides the 8 corner / edge-midpoint rays of each
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)
W = (12, 18, 12, 4)


def light_strips(fs, cfg, cull=1):
    lib = _lib.load()
    prims = np.ascontiguousarray(fs.prims, np.float32).reshape(-1, 9); obj_info = np.ascontiguousarray(fs.obj_info, np.int32).reshape(-1, 3)
    src_i = np.ascontiguousarray(fs.src_i, np.int32).reshape(-1, 4); src_f = np.ascontiguousarray(fs.src_f, np.float32).reshape(-1, 11)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)); ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    ns, n_strips, slack = src_i.shape[0], C.c_int32(0), C.c_float(0)
    n_pairs = np.zeros(ns, np.int32)
    args = (fp(prims), prims.shape[0], ip(obj_info), obj_info.shape[0], ip(src_i), fp(src_f), ns, C.byref(cfg), cull)
    _lib.check(lib.apt_light_strips(*args, None, 0, C.byref(n_strips), ip(n_pairs), C.byref(slack)), "apt_light_strips", lib)
    rows = min(ns, STRIP_EMITTERS)
    masks = np.zeros(rows * n_strips.value, np.uint64)
    _lib.check(lib.apt_light_strips(*args, masks.ctypes.data_as(C.POINTER(C.c_uint64)), masks.size, C.byref(n_strips), ip(n_pairs), C.byref(slack)), "apt_light_strips", lib)
    return masks.reshape(rows, n_strips.value), n_pairs, float(slack.value)


def list_pairs(counts, keep):
    """record (stream order) -> its pair in the emitter's occluder list (-1: not in it), and the list's pair count: flat_pairs() of the kept records"""
    n = [counts[0] + counts[1], counts[2] + counts[3], counts[4] + counts[5], counts[6]]
    out, base, r = [], 0, 0
    for cnt in n:
        kept = 0
        for _ in range(cnt):
            out.append(base + kept // 2 if keep[r] else -1); kept += int(keep[r]); r += 1
        base += (kept + 1) // 2
    return np.array(out, np.int64), base


def _solve(rec, sec, o, d, nudge=0):
    """planar_solve() and the inside test of one planar record for rays (o, d), float32 as the kernel: -> t, inside.  nudge: the reciprocal moved by that many ulps"""
    f = np.float32
    r = rec.astype(f)
    s = (o - r[0:3]).astype(f)
    t_o = _fma(r[9], s[:, 0], _fma(r[10], s[:, 1], (r[11] * s[:, 2]).astype(f)))
    t_d = _fma(r[9], d[:, 0], _fma(r[10], d[:, 1], (r[11] * d[:, 2]).astype(f)))
    inv = (f(1) / t_d).astype(f)
    if nudge: inv = np.nextafter(inv, f(np.inf) * f(nudge))
    t = (-t_o * inv).astype(f)
    p = [_fma(t, d[:, k], s[:, k]) for k in range(3)]
    u = _fma(r[3], p[0], _fma(r[4], p[1], (r[5] * p[2]).astype(f)))
    v = _fma(r[6], p[0], _fma(r[7], p[1], (r[8] * p[2]).astype(f)))
    if sec == 0: inside = np.maximum(np.abs((u - f(0.5)).astype(f)), np.abs((v - f(0.5)).astype(f))) <= f(0.5)
    elif sec == 2: inside = np.minimum(np.minimum(u, v), ((f(1) - u).astype(f) - v).astype(f)) >= 0
    else:
        e1 = _fma(r[12], u, _fma(r[13], v, r[14] + np.zeros_like(u))); e2 = _fma(r[15], u, _fma(r[16], v, r[17] + np.zeros_like(u)))
        inside = np.minimum(np.minimum(u, v), np.minimum(e1, e2)) >= 0
    return t, inside


def camera_hits(stream, recs, cam, d):
    """flat_closest1 over the planar records, then the kernel's hit point d * t + o (two roundings): -> hit mask, hit points.  Spheres are
    left out of this sweep: a ray a sphere would stop goes on to the planar record behind it, one more origin inside the strip's pyramid."""
    f = np.float32
    best = np.full(d.shape[0], f(1e7), f)
    o = np.broadcast_to(cam, d.shape)
    for sec, at in recs:
        if sec == 3: continue
        t, inside = _solve(stream[at:at + W[sec]], sec, o, d)
        ok = inside & (t > f(1e-4)) & (t < best)
        best = np.where(ok, t, best)
    hit = best < f(1e7)
    return hit, ((d * best[:, None]).astype(f) + cam[None]).astype(f)


def strip_rays(cfg, i, j, n_jitter, rs):
    """camera rays of every block: its pyramid's corners and edge midpoints, and n_jitter jittered rays: -> block per ray, directions"""
    npix = i.size
    n_blocks = (npix + 63) // 64
    bi, pi, vx, vy = [], [], [], []
    for b in range(n_blocks):
        lp = np.arange(64 * b, min(npix, 64 * b + 64))
        ii, jj = i[lp], j[lp]
        for (ci, cvx) in ((ii.min(), 1.0), (ii.max(), 0.0), (None, 0.5)):
            for (cj, cvy) in ((jj.min(), 1.0), (jj.max(), 0.0), (None, 0.5)):
                if ci is None and cj is None: continue
                bi.append(b); pi.append((ii[len(ii) // 2] if ci is None else ci, jj[len(jj) // 2] if cj is None else cj)); vx.append(cvx); vy.append(cvy)
    pi = np.array(pi, np.int64)
    lp = rs.randint(0, 64, size=(n_blocks, n_jitter)) + 64 * np.arange(n_blocks)[:, None]
    lp = np.minimum(lp, npix - 1).reshape(-1)
    a, c = rs.uniform(size=(2, lp.size)).astype(np.float32)
    pa, pc = rs.randint(0, 3, size=(2, lp.size))                   # a third of the rays: jitter on a bound, in x / in y independently
    a = np.where(pa == 0, _EDGE[rs.randint(0, _EDGE.size, size=lp.size)], a); c = np.where(pc == 0, _EDGE[rs.randint(0, _EDGE.size, size=lp.size)], c)
    blocks = np.concatenate([np.array(bi, np.int64), lp // 64])
    d = camera_dirs(cfg, np.concatenate([pi[:, 0], i[lp]]), np.concatenate([pi[:, 1], j[lp]]), np.concatenate([np.float32(vx), a]), np.concatenate([np.float32(vy), c]))
    return blocks, d


def light_targets(fs, e, n, rs):
    """points a light sample of emitter e can aim at (shading.hpp emitter_sample_hit), one per ray; None: an emitter without points"""
    t = int(fs.src_i[e, 0])
    if t in (0, 2): return np.repeat(fs.src_f[e, 6:9][None].astype(np.float32), n, 0)
    obj = int(fs.src_i[e, 2])
    if t != 1 or obj < 0: return None
    first, cnt, _ = fs.obj_info[obj]
    if fs.obj_info[obj, 2]:                                      # a sphere: points on its surface
        c = fs.prims.reshape(-1, 9)[first].astype(np.float64)
        v = rs.normal(size=(n, 3)); v /= np.linalg.norm(v, axis=1)[:, None]
        return (c[None, 0:3] + abs(c[3]) * v).astype(np.float32)
    tri = fs.prims.reshape(-1, 3, 3)[rs.randint(first, first + cnt, size=n)].astype(np.float64)
    x, y = rs.uniform(size=(2, n))
    flip = x + y > 1; x[flip], y[flip] = 1 - x[flip], 1 - y[flip]
    x[: n // 4] = rs.randint(0, 2, n // 4); y[: n // 4] = (1 - x[: n // 4]) * rs.randint(0, 2, n // 4)      # a quarter at the vertices
    return (tri[:, 0] + x[:, None] * (tri[:, 1] - tri[:, 0]) + y[:, None] * (tri[:, 2] - tri[:, 0])).astype(np.float32)


def shadow_rays(o, l):
    """sample_light's direction, distance and search limit (stages.hpp shadow_limit), float32"""
    f = np.float32
    to = (l - o).astype(f)
    dist = np.sqrt(((to[:, 0] * to[:, 0] + to[:, 1] * to[:, 1]).astype(f) + to[:, 2] * to[:, 2]).astype(f)).astype(f)
    with np.errstate(all="ignore"):
        d = (to / dist[:, None]).astype(f)
    return d, np.where(dist > 0, (dist - f(1e-4)).astype(f), f(1e7)).astype(f)


def check_film(tag, film, fs, cfg, stats):
    prims = fs.prims.reshape(-1, 9)
    counts, stream, _ = flat_records(prims, fs.obj_info)
    recs = sections(counts)
    _, keep, _ = occluders(prims, fs.obj_info, fs.src_i, fs.src_f)
    masks, n_pairs, slack = light_strips(fs, cfg)
    i, j = local_pixels(cfg)
    n_blocks = (i.size + 63) // 64
    n_emit = fs.src_i.shape[0]
    assert masks.shape == (min(n_emit, STRIP_EMITTERS), n_blocks) and slack > 0
    masks0, _, _ = light_strips(fs, cfg, cull=0)
    assert masks0.shape == masks.shape and (masks0 == ALL).all()                # the switch off: every pair of every strip
    rs = np.random.RandomState(23)
    blocks, d = strip_rays(cfg, i, j, int(np.clip(RAYS_PER_FILM // n_blocks, 24, 2048)), rs)
    cam = np.array(list(cfg.cam_t), np.float32)
    with np.errstate(all="ignore"):
        hit, o_all = camera_hits(stream, recs, cam, d)
    blocks, o_hit = blocks[hit], o_all[hit]
    stats["origins"] += int(hit.sum())
    for e in range(masks.shape[0]):
        pair, np_e = list_pairs(counts, keep[e])
        assert np_e == n_pairs[e]
        l = light_targets(fs, e, o_hit.shape[0], rs)
        if l is None or np_e > 64:
            assert (masks[e] == ALL).all(), (tag, film, e)                      # an emitter that sweeps the full stream, a list of more than 64 pairs
            continue
        if np_e < 64: assert not ((masks[e] != ALL) & ((masks[e] >> np.uint64(np_e)) != 0)).any()      # no bit beyond the list's pairs
        for R, (sec, _) in enumerate(recs):                                     # a sphere record of the list is never left out
            if sec == 3 and keep[e][R]: assert ((masks[e] >> np.uint64(pair[R])) & np.uint64(1)).all(), (tag, film, e, R)
        m = masks[e][blocks]
        stats["set"] += int(sum(bin(int(x)).count("1") for x in masks[e] if x != ALL)); stats["of"] += int(np_e) * int((masks[e] != ALL).sum())
        push = rs.normal(size=o_hit.shape); push *= (rs.uniform(0, 0.5 * slack, size=o_hit.shape[0]) / np.linalg.norm(push, axis=1))[:, None]
        for o in (o_hit, (o_hit.astype(np.float64) + push).astype(np.float32)):
            dd, lim = shadow_rays(o, l)
            for R, (sec, at) in enumerate(recs):
                if sec == 3 or not keep[e][R]: continue
                listed = ((m >> np.uint64(pair[R])) & np.uint64(1)).astype(bool)
                for nudge in (0, 1, -1):
                    with np.errstate(all="ignore"):
                        t, inside = _solve(stream[at:at + W[sec]], sec, o, dd, nudge)
                    blocks_ray = inside & (t > np.float32(1e-4)) & (t < lim)
                    stats["blocked"] += int(blocks_ray.sum())
                    bad = blocks_ray & ~listed
                    assert not bad.any(), (tag, film, e, R, int(bad.sum()), int(blocks[np.flatnonzero(bad)[0]]))


@pytest.mark.parametrize("film", list(FILMS))
def test_every_blocker_of_a_strip_is_in_its_mask(film, flat, parsed):
    scenes = list(flat_scenes(flat, parsed, film))
    assert "cbox" in [tag for tag, _, _ in scenes]
    stats = {"origins": 0, "blocked": 0, "set": 0, "of": 0}
    for tag, fs, prop in scenes:
        check_film(tag, film, fs, _cfg(prop, FILMS[film]), stats)
    assert stats["origins"] > 0 and stats["blocked"] > 0                        # the restatement sees hits and blocked samples at all
    assert stats["set"] < stats["of"], stats                                    # ... and the masks leave pairs out
    print(f"{film}: {stats}")


def test_the_cornell_box_masks_are_shorter_than_the_list(flat, parsed):
    """C2 at 512 x 512: the occluder list has 6 pairs; the issue's proxy expected about 2 of them per strip.  Measured: see the printed figure (profiles/NOTES.md)."""
    fs = flat("cbox")
    masks, n_pairs, _ = light_strips(fs, _cfg(parsed("cbox")[3], FILMS["512x512"]))
    lengths = np.array([bin(int(x)).count("1") for x in masks[0]])
    assert masks.shape == (1, 4096) and n_pairs[0] == 6
    assert lengths.mean() < n_pairs[0], lengths.mean()
    print(f"cbox 512x512: {lengths.mean():.2f} of {n_pairs[0]} pairs per strip on average (min {lengths.min()}, max {lengths.max()}, {100.0 * (lengths == 0).mean():.1f} % of the strips keep none)")


def test_the_capacity_scene_sets_and_clears_mask_bits_in_the_upper_half_of_the_word():
    """capacity_mixed under its point light at 64 x 64: the light's occluder list has 39 pairs - 37 planar ones, then the two sphere
    pairs, which a mask never leaves out.  Among the strips that see no sphere (the others keep every pair) some keep a planar pair at
    bit 32 or above and some leave one out."""
    from flat_cases import capacity
    tup, fs = capacity("capacity_mixed")
    masks, n_pairs, _ = light_strips(fs, _cfg(tup[3], FILMS["64x64"]))
    assert masks.shape == (1, 64) and n_pairs[0] == 39
    real = masks[0][masks[0] != ALL]
    assert 0 < real.size < 64                                                       # strips with a sphere in view, and strips without
    assert upper_half(real, 32, n_pairs[0]) == (True, True)
    assert upper_half(real, 32, 37) == (True, True)                                 # the planar pairs of the upper half
    assert upper_half(real, 37, 39) == (True, False)                                # the sphere pairs: always kept


@pytest.mark.parametrize("n", [16, 17])
def test_sixteen_lights_get_mask_rows_and_seventeen_get_none(n):
    """APT_LIGHT_STRIP_EMITTERS: with 16 emitters every one has a row of masks that leave pairs out; one more and no emitter is culled by
    strip (16 rows of all-ones words), while every emitter still gets its list's pair count"""
    from flat_cases import many_lights
    from adapt_amd.scene_pack import pack_scene
    tup = many_lights(n)
    fs = pack_scene(*tup)
    assert fs.src_i.shape[0] == n and fs.prims.shape[0] == FLAT_MAX_PRIMS
    masks, n_pairs, _ = light_strips(fs, _cfg(tup[3], FILMS["64x64"]))
    assert masks.shape == (STRIP_EMITTERS, 64) and n_pairs.shape == (n,) and (n_pairs >= 33).all() and (n_pairs <= 41).all()
    if n == 16:
        assert all((row != ALL).any() for row in masks)
        assert all(upper_half(row[row != ALL], 32, int(np_e) - 2) == (True, True) for row, np_e in zip(masks, n_pairs))
    else:
        assert (masks == ALL).all()
