"""Inputs and shared checks of the emitter light-sample tests (tests/test_emitter_samples_host.py on the CPU,
tests/test_gpu_emitter_samples.py on the device).  Not collected by pytest (no `test_` prefix); nothing here needs a device.

Scenes: `features_a` (all five emitter types), `cbox` (one point light) and a synthetic emitter scene built here as arrays.  Rows: the strata
of f64_models.emitter_sample_sweep, 64 rows each, the Philox stream of row k keyed (k, SEED) as apt_emitter_probe keys it.

The tolerance rule is the one of tests/test_gpu_product_functions.py: r = f64_models.emitter_sample_hit, S = its scale with the hit
point perturbed relatively (float_cols) and the direction a sphere light constructs perturbed absolutely (dir_cols), per element
|f - r| <= K max(|o - r|, u S).  Rows within a knife edge (margin <= f64_models.KNIFE) are left out and counted; rows placed ON an edge
are never left out: they must match, under the same rule, the model forced onto ONE of the branches adjacent to the edge."""
import itertools
import math

import numpy as np

import f64_models as M
from conftest import _Obj, _Packed, _World

SEED = 1109
SCENE_TAGS = ("features_a", "cbox", "synthetic")

# float32 roundings along the oracle's longest chain to an output, each at most u relative to a term the scale S accounts for (the
# model's |r|, amplified where hit - pos cancels; the roundings that construct a sphere light's direction are the dir_cols' 4 u):
#   point       hit - pos, |x|^2 (3 products, 2 sums), 1 / x, the product with the intensity                                   8
#   spot        hit - pos, |x|^2 (5), sqrt, depth^2, the division                                                            10
#   collimated  hit - pos, the dot product (5), dir * proj, hit - that (the intensity is passed on or zeroed)                  8
#   mesh        the point (2 products, a sum, the fold's 2, + v0), hit - pos, |diff|^2 (5), sqrt, 1 / norm, the scaling, the dot
#               product (5), |diff|^2 / dl, x inv_area, intensity / pdf                                                       24
#   sphere      centre + n r (2), p / r^2 (2), then as a mesh light from hit - pos on (18); the direction n itself: dir_cols    24
ORACLE_ROUNDINGS = {"point": 8, "spot": 10, "collimated": 8, "mesh": 24, "sphere": 24}

# the decisions an on-edge row of each kind sits on (f64_models.emitter_sample_hit `force`)
EDGE_DECISIONS = {"mesh": ("dl",), "sphere": ("dl",), "spot": ("cone",), "collimated": ("proj", "rim"), "point": ()}


# ------------------------------------------------------------------ the synthetic emitter scene
def _tri_normals(P):
    n = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    return n / np.where(ln > 0, ln, 1.0), 0.5 * ln[:, 0]


def _src(t, intensity, direc=(0, 0, 1), pos=(0, 0, 0), inv_area=1.0, r=0.0):
    bits = {0: 0x11, 1: 0x14, 2: 0x11, 4: 0x12 + int(r == 0)}[t]
    d = np.float64(direc); d = d / np.linalg.norm(d)
    return _Packed([t, bits, -1, 0], np.concatenate([intensity, d, pos, [inv_area, r]]))


def synthetic_scene():
    """-> the 4-tuple `scene_parsing` returns.  Emitters, in order:
      0  mesh light, 7 coplanar triangles of unequal area in a tilted plane, triangle 3 of zero area (v2 == v0)
      1  mesh light, a 16 x 16 quad of 2 equal triangles in the plane y = 1024, around (1008, 1024, -1002)
      2, 3, 4  sphere lights of radius 1e-3, 0.3 and 50
      5  point, 6 spot, 7 collimated (r = 0.25), all three with directions off every axis;  8  collimated with r = 0
    and one Lambertian floor quad that emits nothing."""
    from adapt_amd.parsers.obj_desc import get_aabb
    lam = lambda: _Packed(*M.mat_row(1, (0.5, 0.5, 0.5)))
    emitters, objs, prims, normals = [], [], [], []

    def mesh(P, emit_id, normal=None):
        P = np.float32(P)
        n, area = _tri_normals(P.astype(np.float64))
        if normal is not None:
            n = np.where(area[:, None] > 0, n, np.float64(normal)[None])
        prims.append(P); normals.append(np.float32(n))
        objs.append(_Obj(len(P), 0, get_aabb(P.copy(), 0), emit_id, lam()))
        return float(area.sum())

    def sphere(c, r, emit_id):
        P = np.float32([[c, (r, r, r), (0, 0, 0)]])
        prims.append(P); normals.append(np.float32([[0, 1, 0]]))
        objs.append(_Obj(1, 1, get_aabb(P[:, :2].copy(), 1), emit_id, lam()))

    # 0: a fan about o in the plane spanned by a, b: wedge k spans the angles ang[k] .. ang[k + 1], radii rad[k], rad[k + 1]
    o = np.float64([1.5, 2.0, -1.0])
    nn = np.float64([0.3, -0.9, 0.2]); nn /= np.linalg.norm(nn)
    a, b = M._frame(nn[None]); a, b = a[0], b[0]
    ang = np.radians([0, 15, 70, 100, 100, 190, 260, 360]); rad = np.float64([0.4, 0.9, 0.2, 0.7, 0.7, 0.5, 1.0, 0.4])
    rim = o + rad[:, None] * (np.cos(ang)[:, None] * a + np.sin(ang)[:, None] * b)
    fan = np.array([[o, rim[k], rim[k + 1]] for k in range(7)])
    fan[3, 2] = fan[3, 0]                                         # zero area: v2 == v0
    fan = np.float32(fan)
    nfan = _tri_normals(fan.astype(np.float64))[0][0]             # the plane's normal as the float32 vertices give it
    area0 = mesh(fan, 0, normal=nfan)
    emitters.append(_src(1, (10.0, 8.0, 6.0), inv_area=1.0 / area0))
    # 1: coordinates around 1e3, in a plane float32 holds exactly
    q = np.float32([[1000, 1024, -1010], [1016, 1024, -1010], [1016, 1024, -994], [1000, 1024, -994]])
    area1 = mesh([[q[0], q[2], q[1]], [q[0], q[3], q[2]]], 1)      # normal (0, 1, 0): it lights what lies above it
    emitters.append(_src(1, (40.0, 40.0, 30.0), inv_area=1.0 / area1))
    for k, (c, r) in enumerate((((0.5, 0.25, -0.75), 1e-3), ((-2.0, 1.0, 0.5), 0.3), ((30.0, -80.0, 20.0), 50.0))):
        sphere(c, r, 2 + k)
        emitters.append(_src(1, (5.0, 6.0, 7.0), inv_area=1.0 / (4.0 * math.pi * float(np.float32(r)) ** 2)))
    emitters.append(_src(0, (3.0, 2.0, 1.0), pos=(0.7, 1.9, -0.4)))
    emitters.append(_src(2, (4.0, 4.0, 2.0), direc=(0.3, -0.8, 0.52), pos=(-1.2, 2.5, 0.8), r=math.cos(math.radians(25.0))))
    emitters.append(_src(4, (2.0, 3.0, 4.0), direc=(-0.4, -0.6, 0.7), pos=(2.2, 3.1, -1.7), r=0.25))
    emitters.append(_src(4, (1.0, 1.0, 1.0), direc=(0.5, 0.5, -0.7), pos=(-0.3, 0.6, 1.1), r=0.0))
    mesh([[(-4, -1, -4), (4, -1, -4), (4, -1, 4)], [(-4, -1, -4), (4, -1, 4), (-4, -1, 4)]], -1)
    P = np.concatenate(prims)
    arr = {"primitives": P, "n_g": np.concatenate(normals), "n_s": np.zeros((len(P), 3, 3), np.float32),
           "uvs": np.zeros((len(P), 3, 2), np.float32), "indices": None}
    world = _World(); world.medium = type("M", (), {"ior": 1.0})()
    prop = {"film": {"width": 16, "height": 16}, "fov": 40.0, "max_bounce": 4, "num_shadow_ray": 1, "use_rr": False, "use_mis": True,
            "anti_alias": True, "stratified_sampling": False, "brdf_two_sides": False, "accelerator": "none", "rr_bounce_th": 4,
            "rr_threshold": 0.1, "transform": (np.float32([0, 0, 1]), np.float32([0, 1, -8]), None), "world": world,
            "has_vertex_normal": False, "packed_textures": None, "volume": []}
    return emitters, arr, objs, prop


# ------------------------------------------------------------------ one scene's rows, model and oracle
class Case:
    """rows of one scene: X (m,4), stratum, edge, kind (m,), words (m,4), r / S (m,8), mg (m,), keep = off every edge and outside KNIFE"""
    def __init__(self, tag, parsed_tuple):
        from adapt_amd.scene_pack import make_config, pack_scene
        from oracle import binding as ob
        self.tag, self.parsed = tag, parsed_tuple
        self.fs = fs = pack_scene(*parsed_tuple)
        self.X, self.stratum, self.edge = M.emitter_sample_sweep(fs, seed=7)
        m = len(self.X)
        self.src = self.X[:, 0].astype(int)
        self.types = np.array([int(fs.src_i[k][0]) for k in self.src])
        self.geoms = {k: M.emitter_geom(fs, k) for k in range(len(fs.src_i))}
        self.kind = np.array([M.emitter_kind(t, self.geoms[k]) for t, k in zip(self.types, self.src)])
        self.words = np.array([ob.rng_stream(k, SEED, 1, 4) for k in range(m)])
        self.r, self.S, self.mg = M.reference(M.emitter_sample_hit, self.cols(), (3,), dir_cols=(5,))
        self.keep = ~self.edge & (self.mg > M.KNIFE)
        self._oracle = ob.OracleScene(fs, make_config(parsed_tuple[3]).cam_t)
        self._o = None
        self._forced = None

    def cols(self, rows=slice(None), X=None, words=None):
        X = self.X if X is None else X
        src = X[:, 0].astype(int)[rows]
        return ([int(self.fs.src_i[k][0]) for k in src], [self.fs.src_f[k] for k in src], [self.geoms[k] for k in src], X[rows, 1:4],
                (self.words if words is None else words)[rows], np.zeros((len(src), 3)))

    @property
    def o(self):
        """the oracle on the same stream: (m,8) = pos, intensity, pdf, draws"""
        if self._o is None:
            self._o = self.oracle_rows(self.X)
        return self._o

    def oracle_rows(self, X):
        o = np.zeros((len(X), 8))
        for k in range(len(X)):
            pos, inten, pdf, nd = self._oracle.src_sample_hit(int(X[k, 0]), X[k, 1:4], key=k, seed=SEED)
            o[k] = [*pos, *inten, pdf, nd]
        return o

    @property
    def forced(self):
        """the on-edge rows under every combination of their adjacent branches: [(rows index array, r, S)], the free evaluation first"""
        if self._forced is None:
            out = []
            for kind, names in EDGE_DECISIONS.items():
                rows = np.where(self.edge & (self.kind == kind))[0]
                if not len(rows):
                    continue
                for combo in itertools.product((None, True, False), repeat=len(names)):
                    force = {n: c for n, c in zip(names, combo) if c is not None}
                    if force.get("dl") is False:
                        force["pdf"] = True         # the lit branch with the model's own dl, whatever its sign: float32's dl is some
                                                    # value within its error of 0, and S carries the pdf's response to that
                    fn = lambda *a, force=force: M.emitter_sample_hit(*a, force=force)
                    r, S, _ = M.reference(fn, self.cols(rows), (3,), dir_cols=(5,))
                    out.append((rows, r, S))
            self._forced = out
        return self._forced


_cases = {}


def case(tag, parsed):
    """`parsed`: conftest's fixture (tag -> the parsed 4-tuple); the synthetic scene is built here"""
    if tag not in _cases:
        _cases[tag] = Case(tag, synthetic_scene() if tag == "synthetic" else parsed(tag))
    return _cases[tag]


# ------------------------------------------------------------------ the rule
def allowance(o, r, S, K):
    """K max(|o - r|, u S) per element (o = None: K u S)"""
    with np.errstate(invalid="ignore"):
        a = M.U * S if o is None else np.maximum(np.nan_to_num(np.abs(o - r), nan=0.0, posinf=np.inf), M.U * S)
    return K * np.nan_to_num(a, nan=0.0, posinf=np.inf)


def within(x, o, r, S, K):
    """per element: x == r, both NaN, a NaN the oracle has too, or |x - r| inside the allowance"""
    x, r = np.asarray(x, np.float64), np.asarray(r, np.float64)
    with np.errstate(invalid="ignore"):
        ok = (x == r) | (np.isnan(x) & np.isnan(r)) | (np.abs(x - r) <= allowance(o, r, S, K))
    if o is not None:
        ok |= np.isnan(x) & np.isnan(o)
    return ok


def two_branch_failures(c, x, o, K_of_kind):
    """on-edge rows of case c whose outputs x match the model on NONE of the adjacent branches -> list of (row, stratum).  The oracle's
    own error widens the allowance only on the branch the oracle itself took (the one it matches within its rounding count): against
    another branch |o - r| is the whole value, not an error, and the allowance there is K u S."""
    good = np.zeros(len(c.X), bool)
    for rows, r, S in c.forced:
        K = np.array([K_of_kind[k] for k in c.kind[rows]])[:, None]
        xr, r7, S7 = np.asarray(x[rows, :7], np.float64), r[:, :7], S[:, :7]
        allow = allowance(None, r7, S7, K)
        ok = within(xr, None, r7, S7, K)
        if o is not None:
            orow = o[rows, :7]
            Ko = np.array([ORACLE_ROUNDINGS[k] for k in c.kind[rows]])[:, None]
            took = np.all(within(orow, None, r7, S7, Ko), axis=1) & (o[rows, 7] == r[:, 7])
            with np.errstate(invalid="ignore"):
                ok |= took[:, None] & (np.abs(xr - r7) <= allowance(orow, r7, S7, K))
            ok |= np.isnan(xr) & np.isnan(orow)
        good[rows] |= np.all(ok, axis=1) & (x[rows, 7] == r[:, 7])
    bad = np.where(c.edge & ~good)[0]
    return [(int(k), c.stratum[k]) for k in bad]


def ratios(x, r, S):
    """|x - r| / (u S) per element, 0 where equal or both NaN, inf where only one is NaN"""
    from product_function_cases import _ratio
    return _ratio(x, r, S)


# ------------------------------------------------------------------ properties that need no oracle
def property_failures(c, x, tol):
    """(a) a mesh light's point lies in the triangle the model picks, (b) a sphere light's point lies on the sphere, (c) the pdf of
    every lit area sample is the solid-angle pdf MIS computes (f64_models.emitter_solid_angle_pdf) at the sampled point.  x (m,8): the
    outputs under test; tol (m,7): the absolute allowance per element.  Rows: off every edge and outside KNIFE.  -> list of failures"""
    bad = []
    for k in np.where(c.keep & (c.types == 1))[0]:
        g = c.geoms[c.src[k]]
        hit, pos = np.float64(c.X[k, 1:4]), np.float64(x[k, 0:3])
        tp = float(tol[k, 0:3].sum())
        if g[0] == "mesh":
            tri = int(np.int32(np.uint32(c.words[k, 0]))) % len(g[1])
            A = np.float64([g[1][tri], g[2][tri]]).T
            bc, *_ = np.linalg.lstsq(A, pos - np.float64(g[3][tri]), rcond=None)
            off = np.linalg.norm(A @ bc + np.float64(g[3][tri]) - pos)
            tb = tp / max(np.linalg.norm(A, axis=0).max(), 1e-30)
            if not (off <= tp and bc.min() >= -tb and bc.max() <= 1 + tb and bc.sum() <= 1 + 2 * tb):
                bad.append((int(k), c.stratum[k], "a", bc.tolist(), off))
            n = np.float64(g[4][tri])
        else:
            cen, rad = np.float64(g[1]), g[2]
            if not abs(np.linalg.norm(pos - cen) - abs(rad)) <= tp:
                bad.append((int(k), c.stratum[k], "b", float(np.linalg.norm(pos - cen)), rad))
            n = (pos - cen) / rad
        if np.any(x[k, 3:6] != 0):
            sap = _sap_at(c, k, g, hit, pos, n)
            # the packed inverse area is a float32 of its own (one more u), and the pdf moves with the point it is read back at: the
            # position's own allowance, through the formula, is part of the pdf's
            # - for a sphere light, whose normal is recovered from pos = c + n r and loses u |c| / r with it; a mesh light's normal is
            # the triangle's, and its pdf is held at the device's own point with nothing added
            moved = 0.0
            if g[0] == "sphere":
                moved = max(abs(_sap_at(c, k, g, hit, pos + np.float64(sg) * tol[k, 0:3], n) - sap) for sg in itertools.product((-1, 1), repeat=3))
            if not abs(x[k, 6] - sap) <= tol[k, 6] + 2 * M.U * abs(sap) + moved:
                bad.append((int(k), c.stratum[k], "c", float(x[k, 6]), float(sap)))
    return bad


def _sap_at(c, k, g, hit, pos, n):
    """the solid-angle pdf MIS computes for emitter row k at the point pos (a sphere light's normal follows the point)"""
    if g[0] == "sphere":
        n = (pos - np.float64(g[1])) / g[2]
    diff = hit - pos
    dist = np.linalg.norm(diff)
    return M.emitter_solid_angle_pdf(1, c.fs.src_f[c.src[k]][9], diff / dist, n, dist)[0][0]


def containment_failures(c, x):
    """every sampled position inside what flat_build.cpp emitter_points hands the occluder and strip culls: the box of a mesh light's
    vertices, widened by 4 ulp of its largest coordinate; for a sphere light the box c +- (|r| (1 + 1e-3) + 1e-6 (1 + sum |c|))"""
    bad = []
    for k in np.where(c.types == 1)[0]:
        g = c.geoms[c.src[k]]
        pos = np.float64(x[k, 0:3])
        if np.isnan(pos).any():
            continue
        if g[0] == "mesh":
            first, count, _ = (int(a) for a in c.fs.obj_info[int(c.fs.src_i[c.src[k]][2])])
            V = np.float64(c.fs.prims).reshape(-1, 3, 3)[first:first + count].reshape(-1, 3)      # the vertices emitter_points reads
            pad = 4.0 * float(np.spacing(np.float32(np.abs(V).max())))
            lo, hi = V.min(0) - pad, V.max(0) + pad
        else:
            cen = np.float64(g[1])
            pad = abs(g[2]) * (1.0 + 1e-3) + 1e-6 * (1.0 + np.abs(cen).sum())
            lo, hi = cen - pad, cen + pad
        if not (np.all(pos >= lo) and np.all(pos <= hi)):
            bad.append((int(k), c.stratum[k], pos.tolist(), lo.tolist(), hi.tolist()))
    return bad


# ------------------------------------------------------------------ (d) the solid angle an emitter subtends
N_SOLID = 16384


def solid_angle_sphere(cen, rad, p):
    d = np.linalg.norm(np.float64(p) - np.float64(cen))
    return 2.0 * math.pi * (1.0 - math.sqrt(1.0 - (rad / d) ** 2))


def solid_angle_mesh(tris, p):
    """Van Oosterom - Strackee, summed over the triangles"""
    tot = 0.0
    for T in np.float64(tris):
        a, b, c_ = (T[i] - np.float64(p) for i in range(3))
        la, lb, lc = (np.linalg.norm(q) for q in (a, b, c_))
        num = np.dot(a, np.cross(b, c_))
        den = la * lb * lc + np.dot(a, b) * lc + np.dot(a, c_) * lb + np.dot(b, c_) * la
        tot += abs(2.0 * math.atan2(num, den))
    return tot


def solid_angle_points(c, k):
    """three hit points in front of emitter k of case c and the solid angle it subtends from each"""
    g = c.geoms[k]
    if g[0] == "sphere":
        cen, rad = np.float64(g[1]), g[2]
        pts = [cen + rad * np.float64(d) for d in ((0.0, 2.0, 0.0), (1.5, -0.4, 0.9), (-3.0, 2.0, 4.0))]
        return [(np.float32(p), solid_angle_sphere(cen, rad, np.float32(p))) for p in pts]
    tris = np.stack([g[3], g[3] + g[1], g[3] + g[2]], axis=1).astype(np.float64)
    V = tris.reshape(-1, 3)
    cen, ext, n = 0.5 * (V.min(0) + V.max(0)), (V.max(0) - V.min(0)).max(), np.float64(g[4][0])
    ta, tb = M._frame(n[None])
    pts = [cen + ext * (h * n + u * ta[0] + w * tb[0]) for h, u, w in ((0.5, 0.0, 0.0), (1.0, 0.6, -0.3), (0.25, -0.9, 0.8))]
    return [(np.float32(p), solid_angle_mesh(tris, np.float32(p))) for p in pts]


_solid_words = {}


def solid_angle_model(c, k, p):
    """intensity / Le of the model over N_SOLID streams (row keys 0 .. N_SOLID - 1, as one probe launch keys them) -> (n,) float64"""
    from oracle import binding as ob
    if "w" not in _solid_words:
        _solid_words["w"] = np.array([ob.rng_stream(j, SEED, 1, 4) for j in range(N_SOLID)])
    W = _solid_words["w"]
    sf, g, t = c.fs.src_f[k], c.geoms[k], int(c.fs.src_i[k][0])
    le = float(sf[0])
    return np.array([M.emitter_sample_hit(t, sf, g, p, W[j])[0][3] for j in range(N_SOLID)]) / le
