"""Inputs and an index model for the texture-chain tests (helper module: no tests in here).

  * SETS / scene(): synthetic texture sets, packed scenes made from the `textured` fixture's FlatScene with tex_i, tex_f and the three
    atlases replaced.  Inside the rectangle under test every texel has a distinct finite value per channel; every other atlas texel is
    NaN, so a read outside the rectangle shows in the result even at weight 0.  The atlas handed out is a view between two NaN guard
    rows: a read one atlas row past either end of the image still lands in memory this module owns (CPU oracle; a device scene gets a
    copy of the image alone).
  * strata(): coordinate rows in named strata.  The strata that put the float32 product a = (u * scale) * w somewhere choose u so that
    the product lands there (the search is over the neighbouring floats of the quotient).
  * texel_indices(): the float32 restatement of Texture.query's index arithmetic, one rounding per operation, WITHOUT the clamps of
    adapt_amd/csrc/shade_stage.hpp texture_query - `inside` says where those clamps are the identity.
  * query_model(): the whole lookup in float32 numpy, with or without the clamps.

Used by tests/test_texture_chain.py (CPU: model and oracle) and tests/test_gpu_texture_chain.py (device, both builds).
"""
import dataclasses
import functools

import numpy as np

F32 = np.float32
SCALES = (1.0, 0.37, -2.0, 0.0, 1e6)          # scale_u = scale_v of slot k
# name: atlas side, off_x, off_y, w, h.  2x64 touches the atlas' top and bottom rows, 64x64 fills its atlas (all four borders; its buffer
# is 49 152 bytes, twelve 4 KiB pages exactly), 63x17 and 3x5 sit at non-zero offsets
SETS = {"2x2": (64, 5, 9, 2, 2), "2x64": (64, 31, 0, 2, 64), "3x5": (128, 120, 60, 3, 5), "63x17": (128, 40, 100, 63, 17), "64x64": (64, 0, 0, 64, 64)}
STRATA = ("interior", "seam", "tiny_negative", "zero", "tiles_1e4", "tiles_1e5", "tiles_1e6", "tiles_1e8", "huge", "nonfinite")
STAYS_INSIDE = ("interior", "zero", "tiles_1e4", "tiles_1e5")          # every row, every set, every scale
TILES = {"tiles_1e4": 1e4, "tiles_1e5": 1e5, "tiles_1e6": 1e6, "tiles_1e8": 1e8}
POOL = 100000                                 # candidates searched for the rare rows of a large tile count that leave the rectangle


def atlas(name):
    """(A, A, 3) float32 view: NaN outside the set's rectangle, 1 + channel + (y * w + x) / 4096 inside (exact, distinct)"""
    A, ox, oy, w, h = SETS[name]
    big = np.full((A + 2, A, 3), np.nan, F32)
    y, x = np.mgrid[0:h, 0:w]
    big[1 + oy:1 + oy + h, ox:ox + w] = (F32(1) + np.arange(3, dtype=F32))[None, None, :] + (F32(y * w + x) / F32(4096))[:, :, None]
    img = big[1:A + 1]
    assert img.flags["C_CONTIGUOUS"]
    return img


def slots(fs):
    """[(map, object)] of the five textures of a synthetic scene: slot k carries SCALES[k]"""
    mesh = np.nonzero(np.asarray(fs.obj_info)[:, 2] == 0)[0]
    assert len(mesh) >= 2
    return [(k % 3, int(mesh[k // 3])) for k in range(len(SCALES))]


def scene(fs, name):
    """`fs` (the packed `textured` scene) with the set's rectangle on every slot and the set's atlas as all three maps"""
    A, ox, oy, w, h = SETS[name]
    tex_i = np.zeros((fs.n_objects, 3, 5), np.int32); tex_i[:, :, 0] = -255
    tex_f = np.ones((fs.n_objects, 3, 2), F32)
    for k, (m, o) in enumerate(slots(fs)):
        tex_i[o, m] = (0, ox, oy, w, h)
        tex_f[o, m] = SCALES[k]
    img = atlas(name)
    return dataclasses.replace(fs, tex_i=tex_i, tex_f=tex_f, atlas=[img, img, img])


def product(u, scale, w):
    """a = (u * scale) * w in float32"""
    with np.errstate(all="ignore"):
        return F32(F32(F32(u) * F32(scale)) * F32(w))


def _landing(target, scale, w):
    """float32 u whose product lands on (or next to) `target`: the best of the nine floats around target / (scale * w)"""
    target = np.asarray(target, np.float64)
    with np.errstate(all="ignore"):
        u0 = F32(target / (np.float64(F32(scale)) * w))
    cand = [u0]
    for _ in range(4):
        cand.append(np.nextafter(cand[-1], F32(np.inf)))
    lo = u0
    for _ in range(4):
        lo = np.nextafter(lo, F32(-np.inf)); cand.append(lo)
    cand = np.stack(cand)
    with np.errstate(all="ignore"):
        err = np.abs(np.float64(product(cand, scale, w)) - target[None])
    return cand[np.argmin(err, axis=0), np.arange(target.shape[0])]


def _steps(x, j):
    """x moved by j float32 neighbours (j an int array)"""
    x = F32(x).copy()
    for _ in range(int(np.abs(j).max())):
        up, dn = np.nextafter(x, F32(np.inf)), np.nextafter(x, F32(-np.inf))
        x = np.where(j > 0, up, np.where(j < 0, dn, x)); j = j - np.sign(j)
    return x


def axis_rows(stratum, w, scale, rs, n=64):
    """float32 coordinates of one axis of one stratum for a rectangle extent `w` and a scale.  scale 0 cannot put the product anywhere
    (it is +-0, or NaN for a non-finite coordinate): its rows are those of scale 1."""
    s = 1.0 if scale == 0 else scale
    b = w - 1
    if stratum == "interior":
        return _landing(rs.randint(-3, 4, n) * b + rs.uniform(0.01, b - 0.01, n), s, w)
    if stratum == "seam":                       # within +-8 ulp of k * (w-1), k = -3..4 (around 0: the denormals)
        k, j = [a.ravel() for a in np.meshgrid(np.arange(-3, 5), np.arange(-8, 9))]
        return _landing(np.float64(_steps(F32(k * b), j)), s, w)
    if stratum == "tiny_negative":
        return _landing(-np.ldexp(1.0, -np.arange(2, 61)), s, w)
    if stratum == "zero":
        return F32([0.0, -0.0, 0.0, -0.0])
    if stratum in TILES:                        # tile counts |u * scale| in [T / 2, T], both signs
        def draw(m):
            t = rs.uniform(0.5, 1.0, m) * TILES[stratum] * rs.choice([-1.0, 1.0], m)
            with np.errstate(all="ignore"):
                return F32(t / np.float64(F32(s)))
        u = draw(n)
        if TILES[stratum] >= 1e6 and w >= 63:   # the rows that leave the rectangle are one in 1e4 at 1e6 tiles (w = 64): a quarter of the stratum is taken from them
            pool = draw(POOL)
            out = pool[~axis_indices(pool, s, w)[4]][:n // 4]
            u[:len(out)] = out
        return u
    if stratum == "huge":                       # u * scale = +-1e20, +-1e37; u = +-3e38: the products overflow unless scale * w < 1.13
        with np.errstate(all="ignore"):
            return np.concatenate([F32(np.float64([1e20, -1e20, 1e37, -1e37]) / np.float64(F32(s))), F32([3e38, -3e38, 3.4e38, -3.4e38])])
    assert stratum == "nonfinite"
    return F32([np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf, 0.3, 0.3, 0.3])


@functools.lru_cache(maxsize=None)
def rows(stratum, name, scale, seed=0):
    """(n, 2) float32 (u, v) of one stratum for one set and one scale: both axes drawn from the stratum, independently (non-finite rows:
    each axis alone and both together)"""
    _, _, _, w, h = SETS[name]
    rs = np.random.RandomState([seed, STRATA.index(stratum), w, h, int(abs(scale) * 100) % 9973])
    u, v = axis_rows(stratum, w, scale, rs), axis_rows(stratum, h, scale, rs)
    if stratum == "zero":
        v = v[[0, 1, 1, 0]]
    elif stratum == "nonfinite":
        v = F32([0.3, 0.3, 0.3, np.nan, -np.inf, np.inf, np.nan, np.inf, -np.inf])
    elif stratum in ("seam", "tiny_negative", "huge"):
        v = v[rs.permutation(len(v))][:len(u)] if len(v) >= len(u) else v[rs.randint(len(v), size=len(u))]
    out = np.stack([u, v], 1).astype(F32)
    out.setflags(write=False)
    return out


def all_rows(fs, name, seed=0):
    """every stratum on every slot of one synthetic scene -> (maps, objs, uv, stratum names, slot index), row arrays of equal length"""
    maps, objs, uv, st, sl = [], [], [], [], []
    for k, (m, o) in enumerate(slots(fs)):
        for s in STRATA:
            r = rows(s, name, SCALES[k], seed)
            uv.append(r); maps += [m] * len(r); objs += [o] * len(r); st += [s] * len(r); sl += [k] * len(r)
    return np.int32(maps), np.int32(objs), np.concatenate(uv), np.array(st), np.int32(sl)


def axis_indices(u, scale, w):
    """one axis of Texture.query in float32, one rounding per operation: a = (u * scale) * w; r = a - b * floor(a / b), b = w - 1 (Taichi's
    float `%`); floor(r); ratio = r - floor(r).  -> (a, r, floor, ratio, inside): inside = finite, 0 <= floor and floor + 1 <= w - 1"""
    with np.errstate(all="ignore"):
        a = product(u, scale, w)
        b = F32(w) - F32(1)
        q = np.floor(F32(a / b))
        r = F32(a - F32(b * q))
        fl = np.floor(r)
        ratio = F32(r - fl)
        inside = np.isfinite(r) & (fl >= 0) & (fl + F32(1) <= b)
    return a, r, fl, ratio, inside


def texel_indices(u, v, scale_u, scale_v, w, h):
    """-> fu, fv (floors inside the rectangle, float32, unclamped), ratio_u, ratio_v, inside (both axes)"""
    _, _, fu, ru, iu = axis_indices(u, scale_u, w)
    _, _, fv, rv, iv = axis_indices(v, scale_v, h)
    return fu, fv, ru, rv, iu & iv


def _mix(a, b, t):
    with np.errstate(all="ignore"):
        t = F32(t)[:, None]
        return F32(F32(a * F32(F32(1) - t)) + F32(b * t))


def query_model(img, rect, scale_u, scale_v, uv, clamp):
    """Texture.query in float32 numpy on an (H, W, 3) atlas; rect = (off_x, off_y, w, h).  clamp=False: the reference's text - only rows
    that are `inside` may be asked for (the others come back NaN).  clamp=True: texture_query's contract (floor clamped to [0, w-1], NaN
    to 0, ceil = min(floor + 1, w-1), a NaN ratio counts as 0)."""
    ox, oy, w, h = rect
    fu, fv, ru, rv, inside = texel_indices(uv[:, 0], uv[:, 1], scale_u, scale_v, w, h)
    if clamp:
        fu, fv = np.fmin(np.fmax(fu, F32(0)), F32(w - 1)), np.fmin(np.fmax(fv, F32(0)), F32(h - 1))
        cu, cv = np.fmin(fu + F32(1), F32(w - 1)), np.fmin(fv + F32(1), F32(h - 1))
        ru, rv = np.fmax(ru, F32(0)), np.fmax(rv, F32(0))
        ok = np.ones(len(fu), bool)
    else:
        ok = inside
        fu, fv = np.where(ok, fu, 0), np.where(ok, fv, 0)
        cu, cv = fu + 1, fv + 1
    x0, x1, y0, y1 = fu.astype(np.int64) + ox, cu.astype(np.int64) + ox, fv.astype(np.int64) + oy, cv.astype(np.int64) + oy
    out = _mix(_mix(img[y0, x0], img[y0, x1], ru), _mix(img[y1, x0], img[y1, x1], ru), rv)
    out[~ok] = np.nan
    return out


def contained(out, name):
    """per row: finite and, per channel, within the rectangle's min..max widened by 1 ulp of the larger bound (a convex combination
    evaluated in float32: x * (1 - t) + y * t, each product rounded, then the sum)"""
    A, ox, oy, w, h = SETS[name]
    t = atlas(name)[oy:oy + h, ox:ox + w].reshape(-1, 3)
    lo, hi = t.min(axis=0), t.max(axis=0)
    ulp = np.spacing(hi)
    with np.errstate(invalid="ignore"):
        return np.all(np.isfinite(out) & (out >= lo - ulp) & (out <= hi + ulp), axis=1)
