"""A numpy model of the direct-light viewer (upstream's renderer/direct_render.py), in float32 and upstream's operation
order, on the oracle binding's pix2ray / intersect / occluded - and the same in float64 with a brute-force intersector of its own.  What
the viewer's tests share (tests/test_direct_host.py on the CPU, tests/test_gpu_direct.py on the device).  Not collected by pytest.

The float32 model is held to the fixtures the reference produced (tests/golden/direct_*.npz).  The float64 model says where the reference
itself is on an edge: a pixel whose hit object or shadow flag differs between the two precisions is one a correct implementation within
the product build's stated accuracy may decide either way."""
import ctypes
import ctypes.util
import os
import xml.etree.ElementTree as xet

import numpy as np

from adapt_amd.scene_pack import make_config, pack_scene

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# fixture (tests/golden/direct_<name>.npz, written by tests/golden/gen/gen_direct.py) -> the scene tag of conftest's parsed()
FIXTURES = {"cbox": "cbox", "cbox_50x30": "cbox", "balls_mono": "balls_mono", "textured": "textured", "features_a": "features_a",
            "features_a_kg0": "features_a", "cbox_crop": "cbox", "cbox_aa": "cbox"}
SAME_AS_CBOX = ("cbox_crop", "cbox_aa")       # the loop has no crop test, TracerBase fixes anti_alias = False: these equal the plain case
EDGE_CAP = 0.0025                             # share of pixels on which float32 and float64 may disagree (hit object or shadow flag), per case

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.powf.restype = ctypes.c_float
_libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]


def powf(x, y):
    """glibc's powf, element by element: the entry point the fixtures' generator calls (numpy's own float32 power may be a vector routine)"""
    x, y = np.broadcast_arrays(np.asarray(x, F), np.asarray(y, F))
    return np.array([_libm.powf(float(a), float(b)) for a, b in zip(x.reshape(-1), y.reshape(-1))], F).reshape(x.shape)


def load_fixture(name):
    with np.load(os.path.join(GOLDEN, f"direct_{name}.npz")) as z:
        fx = {k: z[k] for k in z.files}
    s = [int(v) for v in fx["settings"]]
    fx.update(width=s[0], height=s[1], has_vertex_normal=s[2], anti_alias=s[3], stratified=s[4], crop=s[5:9], cnt=s[9])
    return fx


def point_emitter(intensity, pos=(0.0, 0.0, 0.0)):
    """a point source with the given rgb intensity, as the parser makes one"""
    from adapt_amd.emitters import PointSource
    r, g, b = (float(v) for v in intensity)
    x, y, z = (float(v) for v in pos)
    e = PointSource(xet.fromstring(f'<emitter type="point" id="viewer"><rgb name="emission" value="1.0"/><point name="center" x="{x!r}" y="{y!r}" z="{z!r}"/></emitter>'))
    e.intensity = F([r, g, b])
    e.pos = F([x, y, z])
    return e


def scene_for(fx, scene):
    """the parsed scene with the settings the fixture was made with: (emitter, array_info, objects, prop) for BlinnPhongTracer / DirectModel"""
    import copy
    em, arr, objs, prop = scene
    prop = dict(prop)
    prop["anti_alias"], prop["stratified_sampling"] = bool(fx["anti_alias"]), bool(fx["stratified"])
    film = {k: v for k, v in prop["film"].items() if not k.startswith("crop_")}
    film["width"], film["height"] = int(fx["width"]), int(fx["height"])
    if fx["crop"][2] > 0:
        film.update(dict(zip(("crop_x", "crop_y", "crop_rx", "crop_ry"), (int(v) for v in fx["crop"]))))
    prop["film"] = film
    if len(fx["kg"]):
        objs = list(objs)
        for row in fx["kg"]:
            k = int(row[0])
            objs[k] = copy.copy(objs[k]); objs[k].bsdf = copy.copy(objs[k].bsdf); objs[k].bsdf.k_g = F(row[1:4])
    return point_emitter(fx["intensity"]), arr, objs, prop


def dot3(a, b):
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2])


def shade(T, ray, t, n_s, k_d, k_g, cam_t, e, occluded, intensity, pow_fn):
    """direct_render.py:73-84 for the hit pixels (rows), in dtype T and upstream's operation order"""
    ray, n_s, k_d, k_g = (np.asarray(a, T) for a in (ray, n_s, k_d, k_g))
    with np.errstate(all="ignore"):
        hit = (ray * np.asarray(t, T)[:, None] + np.asarray(cam_t, T)).astype(T)
        to = (np.asarray(e, T) - hit).astype(T)
        dist = np.sqrt(dot3(to, to).astype(T)).astype(T)
        light_dir = (to / dist[:, None]).astype(T)
        half = (T(0.5) * (light_dir - ray)).astype(T)
        inv_len = (T(1.0) / np.sqrt(dot3(half, half).astype(T)).astype(T)).astype(T)
        half_way = (inv_len[:, None] * half).astype(T)
        base = np.fmax(dot3(half_way, n_s).astype(T), T(0))
        spec = pow_fn(base[:, None], k_g).astype(T)
        atten = np.fmin((T(1.0) / (T(1e-5) + dist * dist).astype(T)).astype(T), T(1e5))
        spec = (spec * atten[:, None]).astype(T)
        spec = np.where(np.asarray(occluded, bool)[:, None], (spec * T(0.1)).astype(T), spec)
        return ((spec * np.asarray(intensity, T)).astype(T) * k_d).astype(T), hit, light_dir, dist


def brute_closest(T, prims, obj_info, o, d, limit):
    """closest hit in dtype T, every primitive, upstream's tests (tracer_base.py:183-214) without the slab cull: (object, t); -1 for none"""
    n = o.shape[0]
    best_t, best_obj = np.array(limit, T).copy() if np.ndim(limit) else np.full(n, limit, T), np.full(n, -1, np.int64)
    with np.errstate(all="ignore"):
        for k, (first, count, is_sphere) in enumerate(obj_info):
            if is_sphere:
                c, r2 = prims[first, 0].astype(T), T(prims[first, 1, 0]) ** 2
                s2c = c - o
                cn2, proj = dot3(s2c, s2c), dot3(d, s2c)
                c2r = cn2 - proj * proj
                cut = np.sqrt(np.maximum(r2 - c2r, 0))
                tt = proj + np.where(cn2 > r2 + T(1e-4), -cut, cut)
                ok = (c2r < r2) & (tt > T(1e-4)) & (tt < best_t)
                best_t, best_obj = np.where(ok, tt, best_t), np.where(ok, k, best_obj)
                continue
            for m in range(first, first + count):
                p1, v1, v2 = prims[m, 0].astype(T), (prims[m, 1] - prims[m, 0]).astype(T), (prims[m, 2] - prims[m, 0]).astype(T)
                M = np.empty((n, 3, 3), T)
                M[:, :, 0], M[:, :, 1], M[:, :, 2] = v1, v2, -d
                det = np.linalg.det(M)
                good = np.abs(det) > 0
                M[~good] = np.eye(3, dtype=T)
                uvt = np.linalg.solve(M, (o - p1)[..., None])[..., 0]
                u, v, tt = uvt[:, 0], uvt[:, 1], uvt[:, 2]
                ok = good & (u >= 0) & (v >= 0) & (u + v <= 1) & (tt > T(1e-4)) & (tt < best_t)
                best_t, best_obj = np.where(ok, tt, best_t), np.where(ok, k, best_obj)
    return best_obj, best_t


class DirectModel:
    """BlinnPhongTracer on the oracle (float32) and by brute force (float64)"""

    def __init__(self, emitter, array_info, objects, prop):
        from oracle import binding as ob
        prop = dict(prop)
        prop["anti_alias"] = prop["stratified_sampling"] = False              # tracer_base.py:60-61
        prop["film"] = {k: v for k, v in prop["film"].items() if not k.startswith("crop_")}      # direct_render.py:64: no crop test
        self.rc = make_config(prop)
        from adapt_amd.renderer import unlit_objects
        self.fs = pack_scene([emitter], array_info, unlit_objects(objects), prop)
        self.osc = ob.OracleScene(self.fs, self.rc.cam_t)
        self.w, self.h = self.rc.width, self.rc.height
        self.cam_t = np.asarray(self.rc.cam_t, F)
        self.intensity = F(emitter.intensity)
        self.k_d = np.stack([F(o.bsdf.k_d) for o in objects])
        self.k_g = np.stack([F(o.bsdf.k_g) for o in objects])
        self.pix = [(i, j) for i in range(self.w) for j in range(self.h)]
        self.rays = np.stack([self.osc.pix2ray(self.rc, i, j, 0, [0.5, 0.5]) for i, j in self.pix]).astype(F)
        o = np.tile(self.cam_t, (len(self.pix), 1))
        self.obj, prim, t, _, ns = self.osc.intersect(o, self.rays)
        self.hit = prim >= 0
        self.t, self.n_s = np.where(self.hit, t, F(0)).astype(F), np.where(self.hit[:, None], ns, F(0)).astype(F)

    def _image(self, rows, tail=()):
        return np.asarray(rows).reshape((self.w, self.h) + tuple(tail))

    @property
    def depth_map(self): return self._image(self.t)
    @property
    def norm_map(self): return self._image(self.n_s, (3,))
    @property
    def obj_map(self): return self._image(np.where(self.hit, self.obj, -1))

    def render_parts(self, emit_pos):
        """(pixels (w, h, 3) float32, occluded (w, h) bool - False where nothing was hit -, lit (w, h, 3): the frame had no shadow ray hit)"""
        idx = np.flatnonzero(self.hit)
        e = F(emit_pos)
        ob = self.obj[idx]
        unshadowed, hit, light_dir, dist = shade(F, self.rays[idx], self.t[idx], self.n_s[idx], self.k_d[ob], self.k_g[ob], self.cam_t, e, np.zeros(len(idx), bool), self.intensity, powf)
        occ = self.osc.occluded(hit, light_dir, dist).astype(bool)
        px, *_ = shade(F, self.rays[idx], self.t[idx], self.n_s[idx], self.k_d[ob], self.k_g[ob], self.cam_t, e, occ, self.intensity, powf)
        pixels, occluded, lit = np.zeros((len(self.pix), 3), F), np.zeros(len(self.pix), bool), np.zeros((len(self.pix), 3), F)
        pixels[idx], occluded[idx], lit[idx] = px, occ, unshadowed
        return self._image(pixels, (3,)), self._image(occluded), self._image(lit, (3,))

    def render(self, emit_pos):
        """(pixels, occluded) of render_parts"""
        return self.render_parts(emit_pos)[:2]

    def edges(self, emit_pos):
        """The same frame in float64 - rays from the float64 pinhole, brute-force hits, brute-force shadow rays: (pixels on which the hit
        object differs from float32's, pixels hit alike whose shadow flag differs), both (w, h) bool"""
        D = np.float64
        rc = self.rc
        R = np.asarray(rc.cam_r, D).reshape(3, 3)
        ij = np.asarray(self.pix, D)
        cd = np.stack([(D(rc.half_w) + 0.5 - ij[:, 0]) * D(rc.inv_focal), (ij[:, 1] - D(rc.half_h) - 0.5) * D(rc.inv_focal), np.ones(len(ij))], -1)
        rays = cd @ R.T
        rays /= np.linalg.norm(rays, axis=-1, keepdims=True)
        prims, info = np.asarray(self.fs.prims, D), [tuple(int(v) for v in row) for row in self.fs.obj_info]
        cam = np.tile(np.asarray(self.cam_t, D), (len(ij), 1))
        obj64, t64 = brute_closest(D, prims, info, cam, rays, 1e7)
        obj32 = np.where(self.hit, self.obj, -1)
        hit_differs = obj64 != obj32
        both = np.flatnonzero((obj64 >= 0) & ~hit_differs)
        hp = rays[both] * t64[both, None] + cam[both]
        to = np.asarray(emit_pos, D) - hp
        dist = np.linalg.norm(to, axis=-1)
        blocker, _ = brute_closest(D, prims, info, hp, to / dist[:, None], np.where(dist > 0, dist - 1e-4, 1e7))
        _, occ32 = self.render(emit_pos)
        shadow_differs = np.zeros(len(ij), bool)
        shadow_differs[both] = (blocker >= 0) != occ32.reshape(-1)[both]
        return self._image(hit_differs), self._image(shadow_differs)


def occluded_in(frame, lit):
    """Which pixels of a device frame were shaded as occluded, read off the frame itself: an occluded pixel is 0.1 x what it would be lit.
    -> (occluded (w, h) bool, decidable (w, h) bool: pixels whose lit value is not zero - a zero pixel says nothing about its shadow ray)"""
    top = lit.max(-1)
    ch = lit.argmax(-1)
    val = np.take_along_axis(frame, ch[..., None], -1)[..., 0]
    return val < F(0.55) * top, top > 0
