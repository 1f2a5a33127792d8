"""Texture.query at its wrap seams, on the CPU: the float32 index model (tests/texture_cases.py), why texture_query clamps, and the
oracle's texture_query (oracle/pt_oracle.c - the same text as adapt_amd/csrc/shade_stage.hpp) against the model and its contract.

The lookup wraps with Taichi's float remainder r = a - b * floor(a / b), a = (u * scale) * w, b = w - 1, and reads texels floor(r),
floor(r) + 1.  In float32 r is not always in [0, b):
  * a tiny negative a gives a / b = -tiny, floor = -1, r = a + b, which rounds to b once |a| is at most half the gap below b: the ceil
    texel is then one past the rectangle (weight 0, but a NaN or inf there still poisons the result, and under a rectangle that
    touches the atlas' last row it is one row past the buffer);
  * at a = k * b +- a few ulp the rounded quotient can sit on the other side of the integer: r < 0 or r = b;
  * at tile counts of 1e6 and more b * floor(a / b) is rounded by more than a texel: r leaves [0, b) by whole texels, at 1e20 by 1e14;
  * an overflowing product or a non-finite coordinate gives NaN.
The reference reads an unchecked field there; texture_query's contract (its header comment) is the reference's arithmetic bit for bit
wherever the indices stay inside the rectangle, and a convex combination of the rectangle's own texels everywhere else.
"""
import numpy as np
import pytest

import texture_cases as TC

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _axes(name, scale, stratum):
    """the stratum's rows of one set and scale through the index model, per axis: [(a, r, floor, ratio, inside, extent)] for u and v"""
    _, _, _, w, h = TC.SETS[name]
    r = TC.rows(stratum, name, scale)
    return [TC.axis_indices(r[:, 0], scale, w) + (w,), TC.axis_indices(r[:, 1], scale, h) + (h,)]


@pytest.mark.parametrize("name", list(TC.SETS))
def test_strata_sizes_and_landing(name):
    """Each stratum has its rows on every scale, and the strata that aim the product put it where they say."""
    _, _, _, w, h = TC.SETS[name]
    for scale in TC.SCALES:
        n = {s: len(TC.rows(s, name, scale)) for s in TC.STRATA}
        assert n["seam"] == 8 * 17 and n["tiny_negative"] == 59 and n["zero"] == 4 and n["nonfinite"] == 9 and n["huge"] == 8
        assert all(n[s] == 64 for s in ("interior",) + tuple(TC.TILES))
        if scale == 0:
            continue
        for a, _, _, _, _, ext in _axes(name, scale, "seam"):                       # within 8 ulp (and the landing's own rounding: 2 more) of a multiple of w-1
            k = np.rint(np.float64(a) / (ext - 1))
            assert set(k) == set(range(-3, 5))
            assert np.all(np.abs(np.float64(a) - k * (ext - 1)) <= 10 * np.spacing(F32(np.abs(k) * (ext - 1))) + ext * 1.5e-45)          # (around 0 the products are denormals: u * scale is rounded to their grid, then multiplied by w)
        for a, *_ in _axes(name, scale, "tiny_negative"):
            assert np.all((a < 0) & (a >= F32(-0.26)) & (a <= F32(-8e-19)))
        for s, t in TC.TILES.items():
            r = TC.rows(s, name, scale)
            tiles = np.abs(np.float64(r) * np.float64(F32(scale)))
            assert np.all((tiles >= 0.49 * t) & (tiles <= 1.01 * t)), s


def test_rows_per_stratum():
    """a few hundred to a few thousand rows per stratum over the five sets and five scales"""
    for s in TC.STRATA:
        n = sum(len(TC.rows(s, name, scale)) for name in TC.SETS for scale in TC.SCALES)
        assert 100 <= n <= 4000, (s, n)


@pytest.mark.parametrize("name", list(TC.SETS))
def test_unclamped_model_leaves_the_rectangle(name):
    """Where the reference's index arithmetic, restated in float32, leaves the rectangle - the record of why texture_query clamps."""
    _, _, _, w, h = TC.SETS[name]
    left = {s: 0 for s in TC.STRATA}
    for scale in TC.SCALES:
        for s in TC.STAYS_INSIDE:                                                     # interior, +-0, tile counts up to 1e5: every row inside
            assert all(ax[4].all() for ax in _axes(name, scale, s)), (scale, s)
        for s in TC.STRATA:
            left[s] += sum(int((~ax[4]).sum()) for ax in _axes(name, scale, s))
        for a, r, fl, ratio, inside, ext in _axes(name, scale, "nonfinite"):
            assert not inside[~np.isfinite(a)].any()
        if scale == 0:                                                                # the product is +-0 for every finite coordinate
            for s in ("seam", "tiny_negative", "tiles_1e6", "tiles_1e8", "huge"):
                assert all(ax[4].all() for ax in _axes(name, scale, s)), s
            continue
        for a, r, fl, ratio, inside, ext in _axes(name, scale, "seam"):
            b = F32(ext - 1)
            assert np.array_equal(~inside, (r == b) | (r < 0))                        # nothing else goes wrong within 8 ulp of a seam
        for a, r, fl, ratio, inside, ext in _axes(name, scale, "tiny_negative"):
            # q = -1, r = a + b: it rounds to b when |a| is at most half the gap below b (ties go to b: its significand is even for every extent used)
            b = F32(ext - 1)
            gap = np.float64(b) - np.float64(np.nextafter(b, F32(0)))
            assert np.all(r[-np.float64(a) <= gap / 4] == b) and not inside[-np.float64(a) <= gap / 4].any()
            assert inside[-np.float64(a) >= gap].all()
            assert (-np.float64(a) <= gap / 4).sum() >= 30
        for a, r, fl, ratio, inside, ext in _axes(name, scale, "tiles_1e8"):
            assert inside.all() if ext < 63 else not inside.all(), (scale, ext)
        for a, r, fl, ratio, inside, ext in _axes(name, scale, "tiles_1e6"):
            # (at an extent of 63 no coordinate of 400 000 drawn at this tile count left the rectangle; at 64 about one in 1e4 does)
            assert inside.all() if ext < 64 else not inside.all(), (scale, ext)
    assert left["tiny_negative"] > 0 and left["huge"] > 0 and left["nonfinite"] == 2 * 6 * len(TC.SCALES)
    if max(w, h) >= 63:
        assert left["tiles_1e6"] + left["tiles_1e8"] > 0
    if min(w, h) <= 5:
        assert left["seam"] > 0                                                       # b = 1, 2, 4: a quotient next to an integer rounds onto it


@pytest.fixture(scope="module")
def lookups(flat):
    """per set: the rows of every stratum and slot, what the oracle returns for them, the model's `inside` and the scale of each row"""
    from oracle import binding as ob
    fs = flat("textured")
    out = {}
    for name in TC.SETS:
        sc = TC.scene(fs, name)
        maps, objs, uv, stratum, slot = TC.all_rows(fs, name)
        got = ob.OracleScene(sc).texture_query(maps, objs, uv)
        out[name] = (sc, maps, objs, uv, stratum, slot, got)
    return out


@pytest.mark.parametrize("name", list(TC.SETS))
def test_oracle_equals_the_model_bit_for_bit_inside(name, lookups):
    sc, maps, objs, uv, stratum, slot, got = lookups[name]
    rect = TC.SETS[name][1:]
    n_inside = 0
    for k, scale in enumerate(TC.SCALES):
        m = slot == k
        want = TC.query_model(sc.atlas[0], rect, scale, scale, uv[m], clamp=False)
        inside = TC.texel_indices(uv[m, 0], uv[m, 1], scale, scale, rect[2], rect[3])[4]
        assert np.isfinite(want[inside]).all()
        assert np.array_equal(_bits(got[m][inside]), _bits(want[inside])), (scale, np.nonzero((_bits(got[m]) != _bits(want)).any(axis=1) & inside)[0][:8])
        n_inside += int(inside.sum())
        for s in TC.STAYS_INSIDE:
            assert inside[stratum[m] == s].all()
    assert n_inside >= 0.5 * len(uv)


@pytest.mark.parametrize("name", list(TC.SETS))
def test_oracle_keeps_every_lookup_inside_the_rectangle(name, lookups):
    """The contract on the rows that are not inside.  Every atlas texel outside the rectangle is NaN, and so are the guard rows in front
    of and behind the atlas: a finite result has read nothing outside the rectangle."""
    sc, maps, objs, uv, stratum, slot, got = lookups[name]
    A, ox, oy, w, h = TC.SETS[name]
    finite = np.isfinite(uv).all(axis=1)
    ok = TC.contained(got, name)
    assert ok[finite].all(), (stratum[finite & ~ok][:8], uv[finite & ~ok][:8])      # finite coordinate: finite, within the rectangle's min..max
    assert (~finite).sum() == 9 * len(TC.SCALES) and ok[~finite].all()                # (non-finite ones may give NaN; with a NaN ratio counted as 0 they do not)
    last = 0
    for k, scale in enumerate(TC.SCALES):
        m = slot == k
        clamped = TC.query_model(sc.atlas[0], (ox, oy, w, h), scale, scale, uv[m], clamp=True)
        assert np.array_equal(_bits(got[m]), _bits(clamped)), scale                   # the contract restated in numpy, every row
        # remainder == w-1 on both axes: the last texel itself; on one axis: that column (row) of the rectangle, interpolated along the other
        _, ru, fu, _, iu = TC.axis_indices(uv[m, 0], scale, w)
        _, rv, fv, _, iv = TC.axis_indices(uv[m, 1], scale, h)
        img = sc.atlas[0]
        both = (ru == w - 1) & (rv == h - 1)
        assert np.array_equal(got[m][both], np.broadcast_to(img[oy + h - 1, ox + w - 1], (int(both.sum()), 3)))
        edge_u = (ru == w - 1) & iv
        lo, hi = img[oy + fv[edge_u].astype(int), ox + w - 1], img[oy + fv[edge_u].astype(int) + 1, ox + w - 1]
        assert np.all((got[m][edge_u] >= lo) & (got[m][edge_u] <= hi))
        last += int(both.sum()) + int(edge_u.sum())
    assert last > 0


def test_oracle_surface_maps_are_its_lookups_at_the_restated_coordinates(flat):
    """orc_surface_maps (what the device's apt_surface_maps_probe is held to): the colour is texture_query at get_uv_item's interpolation
    restated in float32 numpy, the flags follow the object's maps and the first-hit flag, and with the flag off the shading normal is
    the interpolated vertex normal.  Barycentric sums next to 1 (w0 = -+2^-24) are among the rows."""
    from oracle import binding as ob
    fs = flat("textured")
    osc = ob.OracleScene(fs)
    tex_i = np.asarray(fs.tex_i).reshape(fs.n_objects, 3, 5)
    obj_of = np.repeat(np.arange(fs.n_objects), fs.obj_info[:, 1])
    prims = np.nonzero((tex_i[obj_of, :, 0] > -255).any(axis=1))[0]
    rs = np.random.RandomState(5)
    t = F32(rs.randint(1, 1024, len(prims)) / 1024.0)
    bary = np.concatenate([rs.dirichlet([1, 1, 1], len(prims))[:, :2], np.stack([t, np.nextafter(F32(1) - t, F32(2))], 1), np.stack([t, np.nextafter(F32(1) - t, F32(0))], 1)]).astype(F32)
    prims = np.int32(np.tile(prims, 3))
    obj = obj_of[prims]
    uv = F32(fs.uvs).reshape(-1, 3, 2)[prims]
    bu, bv = bary[:, 0:1], bary[:, 1:2]
    w0 = F32(F32(F32(1) - bu) - bv)
    assert (w0 < 0).any() and (np.abs(w0[len(w0) // 3:]) <= F32(2.0 ** -23)).all()
    guv = F32(F32(F32(uv[:, 1] * bu) + F32(uv[:, 2] * bv)) + F32(uv[:, 0] * w0))
    for first in (1, 0):
        kd, ns, ap = osc.surface_maps(prims, bary, first)
        want = (tex_i[obj, 0, 0] > -255) * 1 + first * ((tex_i[obj, 1, 0] > -255) * 2 + (tex_i[obj, 2, 0] > -255) * 4)
        assert np.array_equal(ap, want)
        m = (want & 1) != 0
        assert np.array_equal(_bits(kd[m]), _bits(osc.texture_query(np.zeros(m.sum(), np.int32), obj[m], guv[m])))
        assert np.array_equal(_bits(kd[~m]), _bits(F32(fs.bxdf_f)[obj[~m], 0:3]))
        if not first:
            vn = F32(fs.v_normals).reshape(-1, 3, 3)[prims]
            assert np.array_equal(_bits(ns), _bits(F32(F32(F32(vn[:, 0] * w0) + F32(vn[:, 1] * bu)) + F32(vn[:, 2] * bv))))
    with pytest.raises(ValueError):
        osc.surface_maps([fs.n_prims], [[0.2, 0.2]])
