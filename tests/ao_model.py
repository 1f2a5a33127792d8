"""A numpy model of the ambient-occlusion renderer (upstream's renderer/ssao.py), in float32 and upstream's operation order,
built on the oracle binding's primitives: the Philox stream (rng_stream), pix2ray, the closest-hit query and rotation_between.  What the
AO tests share (tests/test_ao_host.py on the CPU, tests/test_gpu_ao.py on the device).  Not collected by pytest (no `test_` prefix).

The model returns, per call of render and pixel, the value the call adds to channel 0 and - the point of it - which hemisphere samples are
FRAGILE: samples one of whose discrete decisions (the two gates of splat_camera, the film cell int() truncates to, the crop test, the
`depth >= queried` compare) changes when the sample is recomputed with its inputs perturbed by the build's stated accuracy.  A fragile sample
may differ between two correct implementations by a whole term (at most 1), every other sample only by rounding.

  product build: the intersectors answer within 1e-5 relative in t: the camera hit's distance and the depth map are scaled by
                 1 +- 1e-5, all four sign pairs.
  exact build:   the device evaluates cos / sin in double and rounds once, the fixtures come from glibc's cosf / sinf: 1 ulp apart at most
                 (measured on the fixtures' arguments: tests/test_ao_host.py, profiles/ao_metrics.log).  The two horizontal components of the
                 local direction are moved by +-1 ulp, all four sign pairs."""
import ctypes
import ctypes.util

import numpy as np

from adapt_amd.scene_pack import make_config, pack_scene

F = np.float32
AO_DEFAULTS = {"smp_hemisphere": 32, "depth_samples": 64, "sample_extent": 0.1}
TWO_PI = F(2.0 * 3.14159265358979323846)
PERTURB = {
    "fast": [{"t": a, "map": b} for a in (-1e-5, 1e-5) for b in (-1e-5, 1e-5)],
    "exact": [{"ulp_x": a, "ulp_z": b} for a in (-1, 1) for b in (-1, 1)],
}

# fixture (tests/golden/ao_<name>.npz, written by tests/golden/gen/gen_ao.py) -> the scene tag of conftest's parsed()
FIXTURES = {"cbox": "cbox", "cbox_defaults": "cbox", "balls_mono": "balls_mono", "features_a": "features_a", "textured": "textured",
            "cbox_crop": "cbox", "cbox_smp1": "cbox", "cbox_smp33": "cbox", "cbox_depth1": "cbox", "cbox_extent2": "cbox",
            "cbox_no_aa": "cbox", "cbox_no_strat": "cbox"}


# the GPU cases (tests/test_gpu_ao.py): every fixture, and the BVH walk on synth.three_bunnies(levels=1), which has no fixture - the model stands in
# name -> (scene: a tag of conftest's parsed() or "bunnies1", spp, the settings)
MODEL_CASES = {
    "bunnies1": ("bunnies1", 2, {"width": 24, "height": 24, "seed": 0, "smp_hemisphere": 8, "depth_samples": 8, "sample_extent": 0.1}),
    "cbox_50x30": ("cbox", 2, {"width": 50, "height": 30, "seed": 3, "smp_hemisphere": 8, "depth_samples": 8, "sample_extent": 0.1}),      # a pixel count that is no multiple of 64
}
GPU_CASES = list(FIXTURES) + list(MODEL_CASES)
FRAGILE_CAP = 0.02      # fragile pixel-samples' share of all hemisphere samples, per case and build, that the GPU test's bound relies on


def case_scene(name, parsed):
    """(scene, settings for AoModel / AORenderer, spp, fixture or None) of a GPU case"""
    if name in FIXTURES:
        fx = load_fixture(name)
        scene, kw = scene_for(fx, parsed(FIXTURES[name]))
        return scene, kw, int(fx["spp"]), fx
    tag, spp, kw = MODEL_CASES[name]
    if tag == "bunnies1":
        from adapt_amd.synth import three_bunnies
        return three_bunnies(levels=1), dict(kw), spp, None
    return parsed(tag), dict(kw), spp, None


def load_fixture(name):
    import os
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"ao_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def scene_for(fx, scene):
    """the parsed scene with the sensor and film settings the fixture was made with; -> (scene, keyword settings for AoModel / AORenderer)"""
    em, arr, objs, prop = scene
    prop = dict(prop)
    prop["anti_alias"], prop["stratified_sampling"] = bool(fx["anti_alias"]), bool(fx["stratified"])
    film = dict(prop["film"])
    for k in ("crop_x", "crop_y", "crop_rx", "crop_ry"):
        film.pop(k, None)
    if int(fx["do_crop"]):
        sx, ex, sy, ey = (int(v) for v in fx["window"])
        film.update(crop_x=(sx + ex) // 2, crop_rx=(ex - sx) // 2, crop_y=(sy + ey) // 2, crop_ry=(ey - sy) // 2)
    prop["film"] = film
    kw = {"width": int(fx["width"]), "height": int(fx["height"]), "seed": int(fx["seed"]), "smp_hemisphere": int(fx["smp_hemisphere"]),
          "depth_samples": int(fx["depth_samples"]), "sample_extent": float(fx["sample_extent"])}
    return (em, arr, objs, prop), kw


_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.cosf.restype = _libm.sinf.restype = ctypes.c_float
_libm.cosf.argtypes = _libm.sinf.argtypes = [ctypes.c_float]


def cosf(x):
    """glibc's cosf, element by element: the entry point the fixtures' generator and the C oracle call"""
    x = np.asarray(x, F)
    return np.array([_libm.cosf(float(v)) for v in x.reshape(-1)], F).reshape(x.shape)


def sinf(x):
    x = np.asarray(x, F)
    return np.array([_libm.sinf(float(v)) for v in x.reshape(-1)], F).reshape(x.shape)


def unit(u32):
    """a draw as ti.random(float): the top 24 bits"""
    return (np.asarray(u32, np.uint32) >> np.uint32(8)).astype(F) * F(1.0 / 16777216.0)


def smooth_step(x):
    """ssao.py:21-24 with edge0 = 0, edge1 = 1 (clamp as fmin(fmax(x, 0), 1): a NaN clamps to 0)"""
    with np.errstate(invalid="ignore"):
        t = np.fmin(np.fmax(np.asarray(x, F), F(0)), F(1))
        return ((t * t) * (F(3) - F(2) * t)).astype(F)


def dot3(a, b):
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]).astype(F)


def matvec(M, v):
    """M @ v, rows accumulated left to right; M (..., 3, 3) or (3, 3), v (..., 3)"""
    return np.stack([((M[..., r, 0] * v[..., 0] + M[..., r, 1] * v[..., 1]) + M[..., r, 2] * v[..., 2]).astype(F) for r in range(3)], -1)


def inverse3(m):
    """Taichi's 3x3 inverse: adjugate x (1 / det), in float32"""
    m = np.asarray(m, F)
    det = F(F(m[0, 0] * F(F(m[1, 1] * m[2, 2]) - F(m[2, 1] * m[1, 2]))) - F(m[1, 0] * F(F(m[0, 1] * m[2, 2]) - F(m[2, 1] * m[0, 2])))) + F(m[2, 0] * F(F(m[0, 1] * m[1, 2]) - F(m[1, 1] * m[0, 2])))
    inv_det = F(1.0) / F(det)
    E = lambda x, y: m[x % 3, y % 3]
    out = np.zeros((3, 3), F)
    for r in range(3):
        for c in range(3):
            out[c, r] = F(inv_det * F(F(E(r + 1, c + 1) * E(r + 2, c + 2)) - F(E(r + 2, c + 1) * E(r + 1, c + 2))))
    return out


def rasterize(half_w, half_h, inv_focal, window, lx, ly):
    """rasterize_pinhole (ssao.py:65-76): (pi, pj, valid) - int() truncates toward zero; window = (start_x, end_x, start_y, end_y)"""
    lx, ly = np.asarray(lx, F), np.asarray(ly, F)
    with np.errstate(invalid="ignore", over="ignore"):
        fx = (F(half_w + 1.0) - lx / F(inv_focal)).astype(F)
        fy = (F(half_h + 1.0) + ly / F(inv_focal)).astype(F)
        big = ~(np.isfinite(fx) & np.isfinite(fy)) | (np.abs(fx) > 2e9) | (np.abs(fy) > 2e9)
        pi = np.trunc(np.where(big, -1e9, fx)).astype(np.int64)
        pj = np.trunc(np.where(big, -1e9, fy)).astype(np.int64)
    valid = (pi >= window[0]) & (pj >= window[2]) & (pi < window[1]) & (pj < window[3])
    return pi, pj, valid


def splat_camera(ray_d, cam_normal, inv_cam_r, half_w, half_h, inv_focal, window, depth_map):
    """splat_camera (ssao.py:78-91) for unit directions ray_d (..., 3): (test_depth, (gate 1, gate 2, cell)) - test_depth is the depth map
    at the cell the direction projects to, 0 where dot(ray_d, cam_normal) <= 0, z <= 0 or the cell lies outside the window; cell = -1 there"""
    ray_d = np.asarray(ray_d, F)
    g1 = dot3(ray_d, np.asarray(cam_normal, F)) > 0
    loc = matvec(np.asarray(inv_cam_r, F), ray_d)
    z = loc[..., 2]
    g2 = g1 & (z > 0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        pi, pj, valid = rasterize(half_w, half_h, inv_focal, window, (loc[..., 0] / z).astype(F), (loc[..., 1] / z).astype(F))
    valid &= g2
    w, h = depth_map.shape
    test = np.where(valid, depth_map[np.clip(pi, 0, w - 1), np.clip(pj, 0, h - 1)], F(0)).astype(F)
    return test, (g1, g2, np.where(valid, pi * h + pj, -1))


def occlusion_term(depth, test_depth, extent):
    """(term, behind) of ssao.py:107-109: queried = test_depth + 1e-3; (depth >= queried) * smooth_step(0, 1, extent / |queried - depth|)"""
    depth = np.asarray(depth, F)
    queried = (np.asarray(test_depth, F) + F(1e-3)).astype(F)
    behind = depth >= queried
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        term = (np.where(behind, F(1), F(0)) * smooth_step(F(extent) / np.abs(queried - depth).astype(F))).astype(F)
    return term, behind


class AoModel:
    def __init__(self, scene, width=None, height=None, seed=0, **settings):
        from oracle import binding as ob
        self.ob = ob
        prop = scene[3]
        self.rc = make_config(prop, width=width, height=height, seed=seed)
        self.fs = pack_scene(*scene)
        self.osc = ob.OracleScene(self.fs, self.rc.cam_t)
        s = {k: type(d)(settings[k] if settings.get(k) is not None else prop.get(k, d)) for k, d in AO_DEFAULTS.items()}
        self.smp, self.depth_samples, self.extent = s["smp_hemisphere"], s["depth_samples"], F(s["sample_extent"])
        rc = self.rc
        self.w, self.h = rc.width, rc.height
        self.cam_t = np.asarray(rc.cam_t, F)
        self.cam_r = np.asarray(rc.cam_r, F).reshape(3, 3)
        self.inv_cam_r = inverse3(self.cam_r)
        n = self.cam_r[:, 2].copy()
        self.cam_normal = (F(1.0) / F(np.sqrt(F(F(n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]))) * n).astype(F)
        self.window = (rc.start_x, rc.end_x, rc.start_y, rc.end_y) if rc.do_crop else (0, self.w, 0, self.h)
        self.pixels_in = [(i, j) for i in range(self.w) for j in range(self.h)
                          if not rc.do_crop or (rc.start_x <= i < rc.end_x and rc.start_y <= j < rc.end_y)]
        self.n_jitter = 2 if rc.anti_alias else 0

    # ------------------------------------------------------------------ camera rays
    def _rays(self, cnt, first_draw_of):
        """camera rays of every pixel in the window at sample counter cnt; first_draw_of(pixel index) -> the jitter's first draw"""
        d = np.zeros((len(self.pixels_in), 3), F)
        for n, (i, j) in enumerate(self.pixels_in):
            script = [0.5, 0.5]
            if self.n_jitter:
                first = first_draw_of(n)
                u = unit(self.ob.rng_stream(i * self.h + j, self.rc.seed, cnt, first + 2)[first:])
                script = [float(u[0]), float(u[1])]
            d[n] = self.osc.pix2ray(self.rc, i, j, cnt, script)
        return d

    def _trace(self, d):
        o = np.tile(self.cam_t, (d.shape[0], 1))
        obj, prim, t, uv, ns = self.osc.intersect(o, d)
        return prim >= 0, t.astype(F), ns.astype(F)

    # ------------------------------------------------------------------ depth map (ssao.py:46-63)
    def depth_map(self):
        """(depth (w, h) float32, hit counts (w, h), draws (w, h)): sample counter 0, draws 2k, 2k + 1 for the k-th sample"""
        total = np.zeros(len(self.pixels_in), F)
        hits = np.zeros(len(self.pixels_in), np.int32)
        for k in range(self.depth_samples):
            hit, t, _ = self._trace(self._rays(0, lambda n: self.n_jitter * k))
            total = np.where(hit, (total + t).astype(F), total)
            hits += hit
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = np.where(hits > 0, (total / hits.astype(F)).astype(F), total)
        depth, nh, draws = np.zeros((self.w, self.h), F), np.zeros((self.w, self.h), np.int32), np.zeros((self.w, self.h), np.int32)
        for n, (i, j) in enumerate(self.pixels_in):
            depth[i, j], nh[i, j], draws[i, j] = mean[n], hits[n], self.n_jitter * self.depth_samples
        return depth, nh, draws

    # ------------------------------------------------------------------ one call of render (ssao.py:93-130)
    def _terms(self, pos_t, d, R, cos_t, sin_t, cp, sp, depth_map, perturb):
        """per (hit pixel, hemisphere sample): (term, decisions) under one perturbation (None: nominal)"""
        perturb = perturb or {}
        t = (pos_t * F(1.0 + perturb.get("t", 0.0))).astype(F)
        dm = (depth_map * F(1.0 + perturb.get("map", 0.0))).astype(F)
        lx, lz = (cp * sin_t).astype(F), (sp * sin_t).astype(F)
        for key, arr in (("ulp_x", lx), ("ulp_z", lz)):
            if perturb.get(key):
                arr[...] = np.nextafter(arr, F(np.inf if perturb[key] > 0 else -np.inf))
        local = np.stack([lx, cos_t, lz], -1)
        pos = (self.cam_t + d * t[:, None]).astype(F)
        sample = matvec(R[:, None], local)
        position = (pos[:, None, :] + sample * self.extent).astype(F)
        rel = (position - self.cam_t).astype(F)
        depth = np.sqrt(dot3(rel, rel)).astype(F)
        ray_d = (rel / depth[..., None]).astype(F)
        test, (g1, g2, cell) = splat_camera(ray_d, self.cam_normal, self.inv_cam_r, self.rc.half_w, self.rc.half_h, self.rc.inv_focal, self.window, dm)
        term, behind = occlusion_term(depth, test, self.extent)
        return term, (g1, g2, cell, behind)

    def render_call(self, cnt, depth_map, build=None):
        """One call of render at sample counter cnt: value (w, h) - what the call adds to channel 0 -, hit (w, h), draws (w, h) and, with
        build = "fast" | "exact", fragile (w, h): the number of the pixel's hemisphere samples that are fragile for that build"""
        w, h = self.w, self.h
        value, hit_img, draws, fragile = np.zeros((w, h), F), np.zeros((w, h), bool), np.zeros((w, h), np.int32), np.zeros((w, h), np.int32)
        d_all = self._rays(cnt, lambda n: 0)
        hit, t, ns = self._trace(d_all)
        idx = np.flatnonzero(hit)
        for n, (i, j) in enumerate(self.pixels_in):
            draws[i, j] = self.n_jitter + (2 * self.smp if hit[n] else 0)
            hit_img[i, j] = hit[n]
        if len(idx) == 0:
            return {"value": value, "hit": hit_img, "draws": draws, "fragile": fragile}
        u = np.stack([unit(self.ob.rng_stream(self.pixels_in[n][0] * h + self.pixels_in[n][1], self.rc.seed, cnt, self.n_jitter + 2 * self.smp)[self.n_jitter:]) for n in idx])
        cos_t, u_phi = u[:, 0::2].astype(F), u[:, 1::2].astype(F)
        sin_t = np.sqrt((F(1) - cos_t * cos_t).astype(F)).astype(F)
        phi = (TWO_PI * u_phi).astype(F)
        cp, sp = cosf(phi), sinf(phi)
        up = np.array([0, 1, 0], F)
        R = np.stack([self.ob.rotation_between(up, ns[n]) for n in idx]).astype(F)
        term, dec = self._terms(t[idx], d_all[idx], R, cos_t, sin_t, cp, sp, depth_map, None)
        occ = np.zeros(len(idx), F)
        for k in range(self.smp):
            occ = (occ + term[:, k]).astype(F)
        val = (F(1) - occ / F(self.smp)).astype(F)
        frag = np.zeros(term.shape, bool)
        for pert in (PERTURB[build] if build else []):
            _, dec2 = self._terms(t[idx], d_all[idx], R, cos_t, sin_t, cp, sp, depth_map, pert)
            for a, b in zip(dec, dec2):
                frag |= a != b
        for m, n in enumerate(idx):
            i, j = self.pixels_in[n]
            value[i, j], fragile[i, j] = val[m], frag[m].sum()
        return {"value": value, "hit": hit_img, "draws": draws, "fragile": fragile, "phi": phi}

    def run(self, spp, build=None, depth_map=None):
        """spp calls of render after the depth pass: accum (spp, w, h, 3) - the accumulation after every call -, pixels (w, h, 3) after the
        last, draws (spp, w, h), fragile (spp, w, h), depth / depth_hits / depth_draws (w, h)"""
        depth, nh, ddraws = self.depth_map()
        use = depth if depth_map is None else np.asarray(depth_map, F)
        accum = np.zeros((spp, self.w, self.h, 3), F)
        draws, fragile = np.zeros((spp, self.w, self.h), np.int32), np.zeros((spp, self.w, self.h), np.int32)
        cur = np.zeros((self.w, self.h, 3), F)
        cur[..., 2] = use
        last = None
        for s in range(spp):
            last = self.render_call(s + 1, use, build)
            cur[..., 0] = np.where(last["hit"], (cur[..., 0] + last["value"]).astype(F), cur[..., 0])
            accum[s], draws[s], fragile[s] = cur, last["draws"], last["fragile"]
        pixels = np.zeros((self.w, self.h, 3), F)
        if last is not None:
            pixels[...] = np.where(last["hit"], (cur[..., 0] / F(spp)).astype(F), F(0))[..., None]
        return {"accum": accum, "pixels": pixels, "draws": draws, "fragile": fragile, "depth": depth, "depth_hits": nh, "depth_draws": ddraws}
