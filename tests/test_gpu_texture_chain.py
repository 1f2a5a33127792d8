"""The texture chain on the device, both builds: texture_query at its wrap seams (apt_texture_probe on the synthetic sets and strata of
tests/texture_cases.py), the maps of a vertex (apt_surface_maps_probe: uv interpolation from barycentrics, normal map, bump map, albedo)
and a small `textured` render against the image the commit before the clamp rendered.

texture_query.  The chain is (u * scale) * w, Taichi's remainder a - b * floor(a / b) with a plain `/`, floorf, fmaxf / fminf, and
mix3 = x * (1 - t) + y * t.  None of it is an operation the product build substitutes (vec.hpp sdiv / srcp / ssqrt / srsqrt, the OCML
calls) and both builds compile with -ffp-contract=off, so: product == exact bit for bit, and device == oracle bit for bit, on every row
(the oracle is pinned to the float32 numpy model by tests/test_texture_chain.py).  On top of that the contract itself: every finite
coordinate gives a finite value within the rectangle's min..max - every atlas texel outside the rectangle is NaN, so a read outside it,
even at weight 0, would show.

surface_maps.  k_d and the flags are bit-equal to the oracle (lookups only).  n_s goes through rotation_between, whose fnormalize is
axis * v_rsq in the product build: tests/test_gpu_product_functions.py's rule, |f - r| <= K max(|o - r|, u S) against
f64_models.surface_maps_ns, K = 9 per frame built (derived at FAMILIES maps_one_frame = 9: a normal map or a bump map; maps_two_frames =
18: a bump map on a normal-mapped vertex), and that module's aggregate (the product build's p50 and p99.9 of |f - r| / (u S) at most
AGG times the oracle's) where the rows are a population of frames - `textured`, `seams`.  The `parallel` scene has six geometric normals,
hence six frames and four v_rsq arguments in all: its 1092 values are those four roundings over and over, and only the per-element rule
applies to it.  The exact build's n_s equals the oracle's bit for bit.  Measured on an MI355X (profiles/texture_chain_metrics.log), the
largest |f - r| / max(|o - r|, u S) of the product build: 1.98 on `textured` (one frame at right angles to Y: the derivation gives 4),
2.73 on `seams` (two frames), 5.0 on `parallel` (a target 7e-3 from -Y: 8 from the v_rsq alone); the exact build 0.49, 1.0, 1.0.  A float32 numpy restatement
of the chain with a correctly rounded reciprocal square root moved down by one ulp reproduces the 5.0 to the last digit.
"""
import dataclasses
import os

import numpy as np
import pytest

import f64_models as M
import texture_cases as TC
from conftest import GOLDEN, record_metric
from product_function_cases import AGG, FAMILIES, _ratio

pytestmark = pytest.mark.gpu
F32 = np.float32
BUILDS = ("fast", "exact")


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same_bits(a, b):
    """bit for bit, any NaN equal to any NaN"""
    a, b = F32(a), F32(b)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(_bits(a)[~nan], _bits(b)[~nan])


class _Device:
    """a DeviceScene in the named build"""
    def __init__(self, variant, fs):
        from adapt_amd import _lib
        from adapt_amd.renderer import DeviceScene
        self.variant, self.fs, self._lib, self._cls = variant, fs, _lib, DeviceScene

    def __enter__(self):
        lib = self._lib.load(self.variant)
        assert self._lib.arithmetic(lib) == self.variant
        self.sc = self._cls(self.fs, lib=lib)
        return self.sc

    def __exit__(self, *exc):
        self.sc.close()


# ---------------------------------------------------------------------------------------------- texture_query
@pytest.fixture(scope="module")
def lookups(flat):
    """per set: the rows (every stratum, every slot), the oracle's values and both builds'"""
    from oracle import binding as ob
    fs = flat("textured")
    out = {}
    for name in TC.SETS:
        sc = TC.scene(fs, name)
        maps, objs, uv, stratum, slot = TC.all_rows(fs, name)
        got = {"oracle": ob.OracleScene(sc).texture_query(maps, objs, uv)}
        for build in BUILDS:
            with _Device(build, sc) as dev:
                got[build] = dev.texture_query(maps, objs, uv)
        _, _, _, w, h = TC.SETS[name]
        inside = np.zeros(len(uv), bool)
        for k, scale in enumerate(TC.SCALES):
            inside[slot == k] = TC.texel_indices(uv[slot == k, 0], uv[slot == k, 1], scale, scale, w, h)[4]
        out[name] = (uv, stratum, slot, inside, got)
    return out


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", list(TC.SETS))
def test_texture_query_equals_the_oracle(name, build, lookups):
    uv, stratum, slot, inside, got = lookups[name]
    d, o = got[build], got["oracle"]
    differs = (_bits(d) != _bits(o)).any(axis=1) & ~(np.isnan(d) & np.isnan(o)).all(axis=1)
    record_metric(f"texture_chain.query[{name},{build}]", {"rows": len(uv), "inside": float(inside.mean()), "differ_inside": int((differs & inside).sum()),
                                                          "differ": int(differs.sum()), **{f"rows_{s}": int((stratum == s).sum()) for s in TC.STRATA},
                                                          **{f"inside_{s}": float(inside[stratum == s].mean()) for s in TC.STRATA}})
    assert np.array_equal(_bits(d[inside]), _bits(o[inside])), (stratum[differs & inside][:8], uv[differs & inside][:8])      # the reference's arithmetic
    assert _same_bits(d, o), (stratum[differs][:8], uv[differs][:8])                                                          # and the same clamps outside it
    for s in TC.STAYS_INSIDE:
        assert inside[stratum == s].all()


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", list(TC.SETS))
def test_texture_query_never_leaves_the_rectangle(name, build, lookups):
    """finite coordinate: finite (the sentinel: no NaN texel was read, at any weight) and within the rectangle's min..max"""
    uv, stratum, slot, inside, got = lookups[name]
    d = got[build]
    finite = np.isfinite(uv).all(axis=1)
    ok = TC.contained(d, name)
    record_metric(f"texture_chain.contained[{name},{build}]", {"finite_rows": int(finite.sum()), "nan_on_finite_rows": int(np.isnan(d[finite]).any(axis=1).sum()),
                                                               "outside_min_max": int((~ok & finite).sum()), "nan_rows": int(np.isnan(d).any(axis=1).sum())})
    assert not np.isnan(d[finite]).any(), (stratum[finite][np.isnan(d[finite]).any(axis=1)][:8])
    assert ok[finite].all(), (stratum[finite & ~ok][:8], uv[finite & ~ok][:8], d[finite & ~ok][:8])
    assert (~inside & finite).sum() >= 100                                           # the rows the clamp exists for were asked for


@pytest.mark.parametrize("name", list(TC.SETS))
def test_texture_query_product_build_equals_exact_build(name, lookups):
    uv, stratum, slot, inside, got = lookups[name]
    assert _same_bits(got["fast"], got["exact"]), name
    record_metric(f"texture_chain.builds_bit_equal[{name}]", {"rows": len(uv), "different": 0})


# ---------------------------------------------------------------------------------------------- the maps of a vertex
def _barycentrics(rs):
    """(n, 2): interior, on each edge, at each vertex, and sums of 1 +- one float32 step (w0 = 1 - bu - bv = -+tiny)"""
    inner = rs.dirichlet([1, 1, 1], 8)[:, :2]
    t = F32(rs.randint(1, 1024, 3) / 1024.0)
    on_bu0 = np.stack([np.zeros(3), t], 1); on_bv0 = np.stack([t, np.zeros(3)], 1); on_w0 = np.stack([t, F32(1) - t], 1)      # (exact: t is a multiple of 2^-10)
    corners = [[0, 0], [1, 0], [0, 1]]
    t = F32(rs.randint(1, 1024, 3) / 1024.0)
    over = np.stack([t, np.nextafter(F32(1) - t, F32(2))], 1); under = np.stack([t, np.nextafter(F32(1) - t, F32(0))], 1)
    return np.concatenate([inner, on_bu0, on_bv0, on_w0, corners, over, under]).astype(F32)


def _with_two_frames(fs):
    """the `textured` scene with a bump map on its normal-mapped object too (and a normal map on its bump-mapped one): both frames on a vertex"""
    tex_i, tex_f = np.array(fs.tex_i, copy=True).reshape(fs.n_objects, 3, 5), np.array(fs.tex_f, copy=True).reshape(fs.n_objects, 3, 2)
    has = tex_i[:, :, 0] > -255
    n_obj, b_obj = int(np.nonzero(has[:, 1])[0][0]), int(np.nonzero(has[:, 2])[0][0])
    tex_i[n_obj, 2], tex_f[n_obj, 2] = tex_i[b_obj, 2], (1.0, 1.0)
    tex_i[b_obj, 1], tex_f[b_obj, 1] = tex_i[n_obj, 1], (1.0, -1.0)
    return dataclasses.replace(fs, tex_i=tex_i, tex_f=tex_f)


def _map_scenes(fs):
    """name -> packed scene: `textured` itself; `seams`, its uvs moved onto 0, 1, integer tile seams and a quarter (so that the tiny w0 of
    a barycentric sum next to 1 becomes a tiny coordinate), both frames on a vertex; `parallel`, a normal map that is (0, 1, 0) everywhere
    under geometric normals of +-Y, next to +-Y inside rotation_between's 1e-5 and just outside it"""
    seams = np.array(fs.uvs, copy=True).reshape(-1, 3, 2)
    patterns = F32([[[0, 0], [1, 0], [0, 1]], [[1, 1], [0, 0], [0, 0]], [[0.25, 0.125], [0, 0], [0, 0]], [[2, 3], [3, 3], [2, 4]],
                    [[-1, -2], [0, -2], [-1, -1]], [[0, 0], [0, 0], [0, 0]], [[-0.25, -0.5], [1, 0], [0, 1]]])
    for p in range(seams.shape[0]):
        seams[p] = patterns[p % len(patterns)]
    two = _with_two_frames(fs)
    normals = np.array(fs.normals, copy=True)
    yish = F32([[0, 1, 0], [0, -1, 0], [1e-3, 1, 0], [0, -1, 2e-3], [6e-3, 1, 0], [0, -1, -7e-3]])
    yish = F32(yish / np.linalg.norm(np.float64(yish), axis=1, keepdims=True))
    mapped = np.nonzero(np.repeat(two.tex_i[:, 1, 0] > -255, fs.obj_info[:, 1]))[0]
    for j, p in enumerate(mapped):
        normals[p] = yish[j % len(yish)]
    flat_up = np.zeros_like(fs.atlas[1]); flat_up[..., 1] = 1
    return {"textured": fs, "seams": dataclasses.replace(two, uvs=seams),
            "parallel": dataclasses.replace(two, normals=normals, atlas=[fs.atlas[0], flat_up, fs.atlas[2]])}


def _restated_uv(fs, prims, bary):
    """get_uv_item's interpolation in float32, one rounding per operation: w0 = (1 - bu) - bv; g = (uv1 * bu + uv2 * bv) + uv0 * w0"""
    uv = F32(fs.uvs).reshape(-1, 3, 2)[prims]
    bu, bv = bary[:, 0:1], bary[:, 1:2]
    w0 = F32(F32(F32(1) - bu) - bv)
    return F32(F32(F32(uv[:, 1] * bu) + F32(uv[:, 2] * bv)) + F32(uv[:, 0] * w0))


@pytest.fixture(scope="module")
def map_runs(flat):
    """per scene: the rows, the oracle's and both builds' (k_d, n_s, applied), first-hit rows first"""
    from oracle import binding as ob
    fs0 = flat("textured")
    out = {}
    for name, fs in _map_scenes(fs0).items():
        rs = np.random.RandomState(11)
        textured = np.nonzero(np.repeat((np.asarray(fs.tex_i).reshape(fs.n_objects, 3, 5)[:, :, 0] > -255).any(axis=1), fs.obj_info[:, 1]))[0]
        plain = np.nonzero(np.repeat(fs.obj_info[:, 2] == 0, fs.obj_info[:, 1]))[0][:2]          # and two mesh primitives (object 0: no map at all)
        prims, bary = [], []
        for p in list(textured) + list(plain):
            b = _barycentrics(rs)
            prims += [p] * len(b); bary.append(b)
        prims, bary = np.int32(prims), np.concatenate(bary)
        first = np.concatenate([np.ones(len(prims), np.int32), np.zeros(len(prims), np.int32)])
        prims, bary = np.concatenate([prims, prims]), np.concatenate([bary, bary])
        got = {"oracle": ob.OracleScene(fs).surface_maps(prims, bary, first)}
        for build in BUILDS:
            with _Device(build, fs) as dev:
                got[build] = dev.surface_maps(prims, bary, first)
        out[name] = (fs, prims, bary, first, got, ob.OracleScene(fs))
    return out


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", ["textured", "seams", "parallel"])
def test_surface_maps_colour_and_flags_equal_the_oracle(name, build, map_runs):
    fs, prims, bary, first, got, osc = map_runs[name]
    (kd, ns, ap), (okd, ons, oap) = got[build], got["oracle"]
    tex_i = np.asarray(fs.tex_i).reshape(fs.n_objects, 3, 5)
    obj = np.repeat(np.arange(fs.n_objects), fs.obj_info[:, 1])[prims]
    want = (tex_i[obj, 0, 0] > -255) * 1 + (first != 0) * ((tex_i[obj, 1, 0] > -255) * 2 + (tex_i[obj, 2, 0] > -255) * 4)
    assert np.array_equal(ap, want) and np.array_equal(oap, want)
    assert set(np.unique(want)) == ({0, 1, 3, 5} if name == "textured" else {0, 1, 7})           # no map, albedo alone, + normal map, + bump map | + both
    assert _same_bits(kd, okd), np.nonzero((_bits(kd) != _bits(okd)).any(axis=1))[0][:8]
    # the coordinates restated in float32, through the lookup alone: the same colour, bit for bit
    guv = _restated_uv(fs, prims, bary)
    m = (want & 1) != 0
    assert _same_bits(kd[m], osc.texture_query(np.zeros(m.sum(), np.int32), obj[m], guv[m]))
    assert np.array_equal(_bits(kd[~m]), _bits(F32(fs.bxdf_f)[obj[~m], 0:3]))                     # no albedo map: the material's colour
    inside = np.ones(len(prims), bool)
    for mp in range(3):
        for o in np.unique(obj):
            s = (obj == o) & (tex_i[obj, mp, 0] > -255)
            if s.any():
                su, sv = F32(fs.tex_f).reshape(-1, 3, 2)[o, mp]
                inside[s] &= TC.texel_indices(guv[s, 0], guv[s, 1], su, sv, tex_i[o, mp, 3], tex_i[o, mp, 4])[4]
    record_metric(f"texture_chain.maps_colour[{name},{build}]", {"rows": len(prims), "lookups_inside": float(inside.mean()), "rows_not_inside": int((~inside).sum())})
    if name == "seams":
        assert (~inside).sum() >= 10                                                             # barycentric sums next to 1 did put coordinates on the seams
    # first-hit flag off: the shading normal is the one the vertex arrived with (the interpolated vertex normal), the albedo still applies
    off = first == 0
    assert _same_bits(ns[off], ons[off]) and (want[off] <= 1).all() and (want[off] == 1).any()
    vn = F32(fs.v_normals).reshape(-1, 3, 3)[prims[off]]
    bu, bv = bary[off, 0:1], bary[off, 1:2]
    n0 = F32(F32(F32(vn[:, 0] * F32(F32(F32(1) - bu) - bv)) + F32(vn[:, 1] * bu)) + F32(vn[:, 2] * bv)) if fs.has_vertex_normal else F32(fs.normals)[prims[off]]
    assert _same_bits(ns[off], n0)


def _check_normals(name, fam, f, o, r, S, keep, aggregate):
    """test_gpu_product_functions._check: the per-element rule, and the aggregate where the rows are a population (module docstring)"""
    K = FAMILIES[fam]
    qf, qo = _ratio(f, r, S)[keep], _ratio(o, r, S)[keep]
    per = np.where(qf == 0, 0.0, qf / np.maximum(qo, 1.0))
    worst = float(per.max())
    p50f, p999f, p50o, p999o = np.percentile(qf, 50), np.percentile(qf, 99.9), np.percentile(qo, 50), np.percentile(qo, 99.9)
    m = {"family": fam, "K": K, "max_ratio": worst, "p50_f": p50f, "p50_o": p50o, "p999_f": p999f, "p999_o": p999o, "rows": int(keep.sum())}
    record_metric(name, m)
    assert worst <= K, m
    if aggregate:
        assert p50f <= AGG * max(p50o, 1.0) and p999f <= AGG * max(p999o, 1.0), m
    return worst


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", ["textured", "seams", "parallel"])
def test_surface_maps_shading_normal_against_the_f64_model(name, build, map_runs):
    fs, prims, bary, first, got, osc = map_runs[name]
    (kd, ns, ap), (okd, ons, oap) = got[build], got["oracle"]
    on = (first != 0) & ((ap & 6) != 0)
    prims, bary, ap, ns, ons = prims[on], bary[on], ap[on], ns[on], ons[on]
    obj = np.repeat(np.arange(fs.n_objects), fs.obj_info[:, 1])[prims]
    guv = _restated_uv(fs, prims, bary)
    t = {}
    for mp, bit in ((1, 2), (2, 4)):
        t[mp] = np.zeros((len(prims), 3), F32)
        m = (ap & bit) != 0
        t[mp][m] = osc.texture_query(np.full(m.sum(), mp, np.int32), obj[m], guv[m])
    n0 = osc.surface_maps(prims, bary, 0)[1]                                                      # the normal the vertex arrives with (float32, no map applied)
    r, S, margin = M.reference(M.surface_maps_ns, (ap, F32(fs.normals)[prims], n0, t[1], t[2]), (1, 2, 3, 4))
    if build == "exact":
        assert _same_bits(ns, ons), np.nonzero((_bits(ns) != _bits(ons)).any(axis=1))[0][:8]
    keep = (margin > M.KNIFE) & np.isfinite(r).all(axis=1)
    assert (~keep).sum() <= 0.01 * len(keep)                                                    # (`parallel`'s normals sit 9e-6 and 8e-6 from rotation_between's 1e-5 edge: outside the knife edge)
    worst = 0.0
    for fam, sel in (("maps_one_frame", (ap & 6) != 6), ("maps_two_frames", (ap & 6) == 6)):
        if sel.any():
            k = np.repeat((keep & sel)[:, None], 3, axis=1)
            worst = max(worst, _check_normals(f"texture_chain.maps_normal[{name},{build},{fam}]", fam, ns, ons, r, S, k, aggregate=name != "parallel"))
    if name == "parallel":
        # n_g = +-Y under a normal-map texel of (0, 1, 0): rotation_between's parallel branch, +-identity, gives n_s = +-Y, and the bump
        # map's frame around that is +-identity again: the shading normal is +-the bump texel itself, in both builds
        ng = F32(fs.normals)[prims]
        par = (np.abs(ng[:, 1]) == 1) & (ap == 7)
        assert par.sum() >= 20 and np.array_equal(ns[par], ng[par, 1:2] * t[2][par]) and np.isfinite(ns[par]).all()
    record_metric(f"texture_chain.maps_normal[{name},{build}]", {"rows": int(len(prims)), "kept": int(keep.sum()), "max_ratio": worst})


# ---------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("build", BUILDS)
def test_small_textured_render_is_the_image_from_before_the_clamp(build, parsed):
    """16 x 12, 2 spp of scenes/test/textured.xml, bit for bit the image the commit before texture_query's clamps rendered on an MI355X
    (tests/golden/texture_chain_textured_16x12x2.npz, both builds): inside the rectangle the clamps are the identity, end to end."""
    from adapt_amd.renderer import Renderer
    g = np.load(os.path.join(GOLDEN, "texture_chain_textured_16x12x2.npz"))
    r = Renderer(*parsed("textured"), width=16, height=12, exact=(build == "exact"))
    try:
        assert r.info()["arithmetic"] == build
        r.render(n_spp=2)
        img = r.color.to_numpy()
    finally:
        r.close()
    assert img.shape == g[build].shape == (16, 12, 3) and np.isfinite(g[build]).all() and g[build].max() > 0
    assert np.array_equal(_bits(img), _bits(g[build])), int((_bits(img) != _bits(g[build])).any(axis=2).sum())
