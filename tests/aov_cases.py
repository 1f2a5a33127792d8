"""What the feature-buffer tests share (tests/test_aov_host.py on the CPU, tests/test_gpu_aov.py on the device): the scenes, the camera
rays as the oracle makes them, the oracle's answer per ray and the near-tie count.  Not collected by pytest (no `test_` prefix)."""
import numpy as np

from adapt_amd.scene_pack import make_config, pack_scene

FILMS = [(64, 48), (50, 30)]                # (50 x 30: a pixel count that is no multiple of 64)
# case -> (scene: a tag of the parsed() fixture or "bunnies1" = synth.three_bunnies(levels=1), the APT_TRAVERSAL to force or None)
CASES = {
    "cbox": ("cbox", None),
    "balls_mono": ("balls_mono", None),
    "textured": ("textured", None),
    "cbox/bvh": ("cbox", "bvh"),
    "cbox/tile": ("cbox", "tile"),
    "bunnies1": ("bunnies1", None),
}
TIE_REL = 1e-5                              # candidates closer than this (relative) may be told apart differently by the product build
TIE_CAP = 1e-3                              # ... on at most this share of the rays


def scene_of(name, parsed, anti_alias):
    """(emitters, array_info, objects, prop) with the sensor's anti_alias flag set as asked"""
    if name == "bunnies1":
        from adapt_amd.synth import three_bunnies
        em, arr, objs, prop = three_bunnies(levels=1)
    else:
        em, arr, objs, prop = parsed(name)
    prop = dict(prop)
    prop["anti_alias"] = bool(anti_alias)
    return em, arr, objs, prop


def oracle_of(scene, w, h):
    from oracle import binding as ob
    rc = make_config(scene[3], width=w, height=h)
    fs = pack_scene(*scene)
    return ob.OracleScene(fs, rc.cam_t), rc, fs


def jitter(rc, i, j, s):
    """the two numbers pix2ray draws for sample s of pixel (i, j): the first two of the pixel-sample's Philox stream"""
    from oracle import binding as ob
    u = ob.rng_stream(i * rc.height + j, rc.seed, s, 2)
    return [float(np.float32(x >> 8) * np.float32(1.0 / 16777216.0)) for x in u]


def centre_rays(osc, rc):
    """(w*h, 3) float32 directions through the pixel centres in [x][y] order, as the oracle's pix2ray makes them (anti-aliasing off)"""
    assert not rc.anti_alias
    d = np.zeros((rc.width, rc.height, 3), np.float32)
    for i in range(rc.width):
        for j in range(rc.height):
            d[i, j] = osc.pix2ray(rc, i, j, 1, [0.5, 0.5])
    return d.reshape(-1, 3)


def oracle_aov(osc, fs, rc, d):
    """per ray of `d` from the camera: (hit, prim, t, albedo, normal) as the shade stage opens the vertex - the material's k_d or the
    albedo map, the shading normal after the normal / bump maps"""
    o = np.tile(np.float32(rc.cam_t), (d.shape[0], 1))
    obj, prim, t, uv, ns = osc.intersect(o, d)
    hit = prim >= 0
    kd = np.zeros((d.shape[0], 3), np.float32)
    kd[hit] = np.float32(fs.bxdf_f).reshape(-1, 13)[obj[hit], 0:3]
    ns = np.where(hit[:, None], ns, np.float32(0))
    if getattr(fs, "tex_i", None) is not None and hit.any():
        mesh = hit & (np.int32(fs.obj_info).reshape(-1, 3)[np.maximum(obj, 0), 2] == 0)
        k_t, n_t, _ = osc.surface_maps(prim[mesh], uv[mesh], True)
        kd[mesh], ns[mesh] = k_t, n_t
    return hit, prim, np.where(hit, t, np.float32(0)), kd, ns


def candidate_distances(fs, o, d):
    """(rays, prims) float64: every primitive's own hit distance along each ray (inf: none), from the packed triangles / spheres -
    Moeller-Trumbore and the quadratic, independent of both intersectors"""
    P = np.float64(fs.prims).reshape(-1, 9)
    sphere = np.zeros(P.shape[0], bool)
    for first, count, kind in np.int32(fs.obj_info).reshape(-1, 3):
        sphere[first:first + count] = kind != 0
    o, d = np.float64(o)[:, None, :], np.float64(d)[:, None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        v0, e1, e2 = P[None, :, 0:3], P[None, :, 3:6] - P[None, :, 0:3], P[None, :, 6:9] - P[None, :, 0:3]
        pv = np.cross(d, e2)
        det = (e1 * pv).sum(-1)
        tv = o - v0
        u = (tv * pv).sum(-1) / det
        qv = np.cross(tv, e1)
        v = (d * qv).sum(-1) / det
        t_tri = (e2 * qv).sum(-1) / det
        t_tri = np.where((np.abs(det) > 1e-12) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t_tri > 1e-4), t_tri, np.inf)
        oc = o - P[None, :, 0:3]
        b = (oc * d).sum(-1); c = (oc * oc).sum(-1) - P[None, :, 3] ** 2
        disc = b * b - c
        root = np.sqrt(np.maximum(disc, 0))
        t_sph = np.where(-b - root > 1e-4, -b - root, -b + root)
        t_sph = np.where((disc >= 0) & (t_sph > 1e-4), t_sph, np.inf)
    return np.where(sphere[None, :], t_sph, t_tri)


def near_ties(fs, o, d):
    """bool per ray: its two closest candidates lie within TIE_REL (relative) of each other"""
    out = np.zeros(len(d), bool)
    chunk = max(1, (1 << 21) // max(1, int(fs.n_prims)))          # ~2 Mi ray-primitive pairs at a time
    for a in range(0, len(d), chunk):
        t = np.partition(candidate_distances(fs, o[a:a + chunk], d[a:a + chunk]), 1, axis=1)[:, :2] if fs.n_prims >= 2 else None
        if t is not None:
            with np.errstate(invalid="ignore"):
                out[a:a + chunk] = np.isfinite(t[:, 1]) & (t[:, 1] - t[:, 0] <= TIE_REL * t[:, 0])
    return out
