"""Pane-stack scenes for the null-surface walks, the float64 model of the transmittance walk and what the CPU and GPU tests of them
share (tests/test_null_stack.py: the oracle; tests/test_gpu_null_stack.py: the device, both builds, every walk).  Not collected by
pytest (no `test_` prefix).

Every other scene of the suite has ONE null-surface object, so no light sample there walks more than three segments and no camera path
crosses more than two null surfaces in a row.  These scenes stack k thin null-surface boxes ("panes") holding a medium:

  side_stack(k, sheet_after)   one Lambertian quad facing the camera, a point light far to its side, k panes (perpendicular to x) between
                               light and quad, outside the camera's frustum; optionally an opaque sheet behind pane `sheet_after`; always
                               an opaque backstop just behind the light, which only a walk that overshoots the light can meet.  One
                               bounce, one light sample, clear world, absorbing panes: pixel(k) / pixel(0) IS the walk's transmittance.
  front_stack(k, variant)      the Cornell room with k panes perpendicular to the view axis and the light at the front: camera paths cross
                               up to 2k null surfaces per stretch, light samples from the back need up to 2k + 1 segments.

track_ray (vpt.py:99-138) walks at most SEVEN closest-hit segments; a sample still walking after the seventh counts as arrived.  With
the quad-to-pane gap as segment 1, pane j is segment 2j and the gap behind it segment 2j + 1: only the first three panes attenuate, a
sheet behind pane 1, 2 or 3 is met in segment 3, 5 or 7 and blocks, a sheet behind pane 4 is never seen.
"""
import xml.etree.ElementTree as xet

import numpy as np

from adapt_amd.scene_pack import make_config, pack_scene

F32 = np.float32
U = 2.0 ** -24
MAX_SEGMENTS = 7                            # vpt.py:113

# ------------------------------------------------------------------ geometry
SIDE_W, SIDE_H = 32, 24
SIDE_KS = (0, 1, 2, 3, 4, 6)
SIDE_SHEETS = (1, 2, 3, 4, 5)               # of five panes: the sheet stands behind pane j
SIDE_CAM = (0.0, 0.0, -6.0)
SIDE_FOV = 20.0                             # over the film's 24 rows: the view is 2.12 x 1.59 wide at the quad, the quad 2.6
SIDE_QUAD_Z, SIDE_QUAD_HALF = 3.0, 2.6
SIDE_LIGHT = (40.0, 0.0, -10.0)
SIDE_X0, SIDE_PITCH, SIDE_DX = 3.0, 1.0, 0.5            # pane j (1-based) spans x in [X0 + (j - 1) PITCH, ... + DX]
SIDE_SPAN = 20.0                                        # |y|, |z| extent of panes and sheet: a light sample crosses them within |y|, |z| < 3.1
SIDE_U_A = (0.1, 0.3, 0.6)
SIDE_BACKSTOP = 0.5                                     # the opaque sheet behind the light stands this far behind it (pane 1 alone is further from the quad)
FRONT_W, FRONT_H = 48, 36
FRONT_CASES = ("k1", "k3", "k6", "scatter", "world", "nested")


def box(lo, hi):
    """twelve triangles of the axis-aligned box, wound so that the geometric normal cross(b - a, c - b) points outwards: in_free_space
    is the sign of n_g . d (vpt.py:119)"""
    lo, hi = np.float64(lo), np.float64(hi)
    tris = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for side, x in ((-1.0, lo[a]), (1.0, hi[a])):
            p = np.zeros((4, 3))
            p[:, a] = x
            p[:, b] = (lo[b], hi[b], hi[b], lo[b])
            p[:, c] = (lo[c], lo[c], hi[c], hi[c])           # counter-clockwise about +a
            if side < 0:
                p = p[::-1]
            tris += [[p[0], p[1], p[2]], [p[0], p[2], p[3]]]
    tris = F32(tris)
    n = np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 1])
    out = tris.mean(axis=1) - (lo + hi) / 2
    assert np.all((n * out).sum(axis=1) > 0)
    return tris


def _null(u_a, u_s=(0.0, 0.0, 0.0), g=0.0, ident="pane"):
    from adapt_amd.synth import _mat
    rgb = lambda name, v: f'<rgb name="{name}" r="{v[0]}" g="{v[1]}" b="{v[2]}"/>'
    return _mat(f'<bsdf type="null" id="{ident}"><medium type="hg">{rgb("u_a", u_a)}{rgb("u_s", u_s)}<rgb name="par" value="{g}"/>'
                f'<float name="ior" value="1.0"/></medium></bsdf>')


def _point(pos, emission):
    from adapt_amd.emitters import SOURCE_MAP
    return SOURCE_MAP["point"](xet.fromstring(f'<emitter type="point" id="pt"><rgb name="emission" value="{emission}"/>'
                                              f'<point name="center" x="{pos[0]}" y="{pos[1]}" z="{pos[2]}"/></emitter>'))


def _sensor(w, h, fov, bounce, use_rr, extra=""):
    return (f'<sensor><float name="fov" value="{fov}"/><integer name="max_bounce" value="{bounce}"/><integer name="num_shadow_ray" value="1"/>'
            f'<boolean name="use_rr" value="{"true" if use_rr else "false"}"/><boolean name="anti_alias" value="true"/>'
            f'<boolean name="stratified_sampling" value="true"/><boolean name="use_mis" value="true"/><string name="accelerator" value="bvh"/>'
            f'{extra}<integer name="width" value="{w}"/><integer name="height" value="{h}"/></sensor>')


def side_pane_x(j):
    """(entry, exit) x of pane j = 1 .. k"""
    x = SIDE_X0 + (j - 1) * SIDE_PITCH
    return x, x + SIDE_DX


def side_sheet_x(j):
    """the opaque sheet behind pane j: halfway to where pane j + 1 begins"""
    return side_pane_x(j)[1] + (SIDE_PITCH - SIDE_DX) / 2


def side_stack(k, sheet_after=None):
    """-> the 4-tuple scene_parsing returns"""
    from adapt_amd.synth import _Builder, _brdf
    b = _Builder()
    s, z = SIDE_QUAD_HALF, SIDE_QUAD_Z
    b.mesh(F32([[[-s, -s, z], [-s, s, z], [s, s, z]], [[-s, -s, z], [s, s, z], [s, -s, z]]]), _brdf("lambertian", "#CCCCCC"))      # normal -z: towards the camera
    pane = _null(SIDE_U_A)
    for j in range(1, k + 1):
        x0, x1 = side_pane_x(j)
        b.mesh(box((x0, -SIDE_SPAN, -SIDE_SPAN), (x1, SIDE_SPAN, SIDE_SPAN)), pane)
    black = _brdf("lambertian", "#000000")
    sheet = lambda x, e=SIDE_SPAN: F32([[[x, -e, -e], [x, e, -e], [x, e, e]], [[x, -e, -e], [x, e, e], [x, -e, e]]])
    if sheet_after is not None:
        b.mesh(sheet(side_sheet_x(sheet_after)), black)
    # an opaque backstop half a unit BEHIND the light, in every variant: a walker whose remaining distance was not shortened by what
    # it has walked searches past the light and is blocked there; a correct one never sees it
    b.mesh(sheet(SIDE_LIGHT[0] + SIDE_BACKSTOP), black)
    emitters, arr, objs, cfg = b.finish([_point(SIDE_LIGHT, "4000.0, 4000.0, 4000.0")], _sensor(SIDE_W, SIDE_H, SIDE_FOV, 1, False))
    cfg["transform"] = (F32([0, 0, 1]), F32(SIDE_CAM), None)
    return emitters, arr, objs, cfg


def front_stack(case):
    """one of FRONT_CASES -> the 4-tuple scene_parsing returns.  Roulette from the first bounce on (rr_bounce_th 1, threshold 0.8): it
    draws on pass-through iterations too (vpt.py:164-172 runs before the intersection)."""
    from adapt_amd.parsers.world import World_np
    from adapt_amd.synth import _Builder, _brdf, _room
    b = _Builder()
    _room(b, _brdf("lambertian", "#BDBDBD"), _brdf("lambertian", "#DD2525"), _brdf("lambertian", "#25DD25"))
    thin = _null((0.05, 0.1, 0.2))
    if case == "nested":                                       # a null box inside a null box: two media, four surfaces on a line through both
        b.mesh(box((0.6, 0.4, 1.0), (4.9, 4.6, 4.0)), thin)
        b.mesh(box((1.5, 1.2, 2.0), (4.0, 3.8, 3.0)), _null((0.3, 0.15, 0.05), (0.2, 0.2, 0.2), 0.3, "core"))
    else:
        k = {"k1": 1, "k3": 3, "k6": 6, "scatter": 3, "world": 3}[case]
        mat = _null((0.05, 0.1, 0.2), (0.5, 0.4, 0.3), 0.4) if case == "scatter" else thin
        for j in range(k):                                     # the room is 5.56 x 5.49 x 5.59: the panes leave a margin to every wall
            z0 = 0.7 + 0.75 * j
            b.mesh(box((0.5, 0.4, z0), (5.0, 4.9, z0 + 0.4)), mat)
    extra = '<integer name="rr_bounce_th" value="1"/><float name="rr_threshold" value="0.8"/>'
    emitters, arr, objs, cfg = b.finish([_point((2.78, 2.7, 0.2), "40.0, 40.0, 40.0")], _sensor(FRONT_W, FRONT_H, 39.3077, 4, True, extra))
    if case == "world":
        cfg["world"] = World_np(xet.fromstring('<world name="w"><medium type="hg"><rgb name="u_a" value="0.01"/><rgb name="u_s" r="0.04" g="0.05" b="0.06"/>'
                                               '<rgb name="par" value="0.5"/><float name="ior" value="1.0"/></medium></world>'))
    return emitters, arr, objs, cfg


# ------------------------------------------------------------------ the float64 model of the walk (side stack)
def walk_model(point, k, sheet_after=None, light=SIDE_LIGHT, u_e=SIDE_U_A):
    """track_ray for one light sample of the side stack, in float64: from `point` on the quad towards the light, closest-hit segment by
    segment over the pane faces and the sheet.  -> (segments walked, transmittance (3,), optical depth (3,)).

    A segment ends at the next surface in front of the walker.  Nothing in front: the sample arrives.  The sheet: blocked, transmittance
    0.  A pane's far face: the segment lay inside the pane and attenuates by exp(-u_e length); its near face: the segment lay in the
    clear world.  After the seventh segment the walk stops wherever it is and the sample counts as arrived."""
    p, l = np.float64(point), np.float64(light)
    dist = float(np.linalg.norm(l - p))
    d = (l - p) / dist
    surfaces = []                                              # (distance along the ray, kind)
    for j in range(1, k + 1):
        x_in, x_out = side_pane_x(j)
        surfaces += [((x_in - p[0]) / d[0], "near face"), ((x_out - p[0]) / d[0], "far face")]
    if sheet_after is not None:
        surfaces.append(((side_sheet_x(sheet_after) - p[0]) / d[0], "sheet"))
    u_e = np.float64(u_e)
    tau, t, segments = np.zeros(3), 0.0, 0
    while segments < MAX_SEGMENTS:
        segments += 1
        ahead = [s for s in surfaces if t < s[0] < dist]
        if not ahead:
            break                                              # the way to the light is free
        t_hit, kind = min(ahead)
        if kind == "sheet":
            return segments, np.zeros(3), np.full(3, np.inf)
        if kind == "far face":
            tau += u_e * (t_hit - t)
        t = t_hit
    return segments, np.exp(-tau), tau


# K_RATIO 2^-24 (1 + tau) bounds |pixel(k) / pixel(0) - T| / T for correctly rounded float32 code, tau the optical depth of the channel:
#   constant part, 20 roundings of 2^-24 each: up to three expf of at most one ulp (2 each), the three products that fold them into the
#   sample (3), the product with the light's intensity (1), and the five operations between there and the pixel (brdf, MIS weight, the
#   division by the emitter pdf as a reciprocal and a product, the light-sample average) in EACH of the two images (10);
#   part proportional to tau, 14 roundings: an in-pane length is the hit distance from a walker that was moved onto the near face by
#   o + d t - its x, below 8, is rounded to 2^-22, against a length of at least DX = 0.5: 8 - the distance arithmetic itself (3), the
#   normalised direction (2), the product u_e * length (1).
# 20 + 14 tau <= 24 (1 + tau).
K_RATIO = 24.0
DEVICE_MARGIN = 4.0        # the device's bound: the oracle's measured maximum x 4 (the product build's exp and flat-sweep distances are good to 1e-5 relative)


def side_points(osc, rc):
    """(w, h, 3) float64: where the one sample of each pixel meets the quad - the camera ray is the oracle's pix2ray on the two numbers
    the sample's Philox stream opens with (as tests/aov_cases.py takes them), the intersection is float64"""
    from aov_cases import jitter
    pts = np.zeros((rc.width, rc.height, 3))
    o = np.float64(rc.cam_t)
    for i in range(rc.width):
        for j in range(rc.height):
            d = np.float64(osc.pix2ray(rc, i, j, 1, jitter(rc, i, j, 1)))
            pts[i, j] = o + d * ((SIDE_QUAD_Z - o[2]) / d[2])
    assert np.abs(pts[..., :2]).max() < SIDE_QUAD_HALF
    return pts


_side = {}


def side_reference():
    """computed once, left unchanged: the render configuration, the sample points, per k the model's transmittance (w, h, 3), optical
    depth and segments (w, h), and the oracle's 1 spp images and statistics of every stack and sheet variant"""
    if not _side:
        from oracle import binding as ob
        tup0 = side_stack(0)
        rc = make_config(tup0[3], width=SIDE_W, height=SIDE_H, volumetric=True)
        pts = side_points(ob.OracleScene(pack_scene(*tup0), rc.cam_t), rc)
        model = {}
        for k in SIDE_KS:
            rows = [walk_model(p, k) for p in pts.reshape(-1, 3)]
            model[k] = (np.array([r[1] for r in rows]).reshape(SIDE_W, SIDE_H, 3), np.array([r[2] for r in rows]).reshape(SIDE_W, SIDE_H, 3),
                        np.array([r[0] for r in rows]).reshape(SIDE_W, SIDE_H))
        sheet_model = {j: np.array([walk_model(p, 5, j)[1] for p in pts.reshape(-1, 3)]).reshape(SIDE_W, SIDE_H, 3) for j in SIDE_SHEETS}
        oracle = {}
        for key in [(k, None) for k in SIDE_KS] + [(5, j) for j in SIDE_SHEETS]:
            tup = side_stack(*key)
            img, _, st = ob.OracleScene(pack_scene(*tup), rc.cam_t).render(make_config(tup[3], width=SIDE_W, height=SIDE_H, volumetric=True), 1)
            oracle[key] = (img, st)
        _side.update(rc=rc, points=pts, model=model, sheet_model=sheet_model, oracle=oracle)
    return _side


def ratio_error(image_k, image_0, k):
    """max over the pixels that image_0 lights and the channels of |image_k / image_0 - T| / (2^-24 (1 + tau) T), T and tau the model's.
    No lit pixel is left out: one that image_k leaves dark counts with a ratio of 0.  -> (the maximum, lit pixels)"""
    ref = side_reference()
    T, tau, _ = ref["model"][k]
    lit = (np.float64(image_0) > 0).all(axis=2)
    ratio = np.float64(image_k)[lit] / np.float64(image_0)[lit]
    err = np.abs(ratio - T[lit]) / (U * (1 + tau[lit]) * T[lit])
    return float(err.max()), int(lit.sum())


def oracle_max_error():
    """the oracle's largest ratio_error over SIDE_KS: what the device's bound is a multiple of"""
    ref = side_reference()
    return max(ratio_error(ref["oracle"][(k, None)][0], ref["oracle"][(0, None)][0], k)[0] for k in SIDE_KS)


def check_sheets(images, image_0):
    """images: {j: the five-pane image with the sheet behind pane j}.  A sheet behind pane 1, 2 or 3 blocks every sample: zero everywhere.
    Behind pane 4 or 5 it is never seen - the walk ends in segment 7, the gap behind pane 3: the two images are the same bit for bit, and
    lit wherever the stack-free image is."""
    ref = side_reference()
    for j in (1, 2, 3):
        assert not ref["sheet_model"][j].any()
        assert not np.asarray(images[j]).any(), j
    assert np.array_equal(ref["sheet_model"][4], ref["model"][3][0]) and np.array_equal(ref["sheet_model"][5], ref["model"][3][0])
    a, b = np.asarray(images[4], F32), np.asarray(images[5], F32)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal((a > 0).all(axis=2), (np.asarray(image_0) > 0).all(axis=2)) and (a > 0).any()


def min_segments(k):
    """n_track / light samples walked is at least this for a stack of k panes without a sheet"""
    return min(2 * k + 1, MAX_SEGMENTS) - 0.05


# ------------------------------------------------------------------ the front stack against the oracle on the same stream
FRONT_SPP = 16
_front = {}


def front_reference(case):
    """(scene tuple, render configuration, the oracle's FRONT_SPP image, its statistics), computed once per case"""
    if case not in _front:
        from oracle import binding as ob
        tup = front_stack(case)
        rc = make_config(tup[3], width=FRONT_W, height=FRONT_H, volumetric=True)
        img, _, st = ob.OracleScene(pack_scene(*tup), rc.cam_t).render(rc, FRONT_SPP)
        _front[case] = (tup, rc, img, st)
    return _front[case]


# ------------------------------------------------------------------ builds and walks
# (build, walk, environment switches, info()["traversal"], shadow launches per iteration in a scene with null surfaces)
# The flat walk takes three launches per iteration (the third walks segments 2 .. 6 itself), every other walk one per segment: that
# tells the product build's flat walk from the one APT_VSHADOW_FLAT=0 puts in its place, which info() does not name (the tiled
# sweep here: a pane has twelve primitives, api.hip small_scene_sweep).
WALKS = {
    "fast/flat": ("fast", {}, "flat", 3),
    "fast/tile": ("fast", {"APT_VSHADOW_FLAT": "0"}, "flat", 7),
    "fast/sweep": ("fast", {"APT_TRAVERSAL": "sweep"}, "sweep", 7),
    "fast/bvh": ("fast", {"APT_TRAVERSAL": "bvh"}, "bvh", 7),
    "exact/tile": ("exact", {"APT_TRAVERSAL": "tile"}, "tile", 7),
    "exact/sweep": ("exact", {"APT_TRAVERSAL": "sweep"}, "sweep", 7),
    "exact/bvh": ("exact", {"APT_TRAVERSAL": "bvh"}, "bvh", 7),
}


def assert_walk(r, walk, null_surfaces=True):
    """the renderer runs the build and the walk the row names: arithmetic and traversal of info(), and - the walk's kernel is not named
    there - the launches it takes per iteration"""
    build, _, traversal, per_iter = WALKS[walk]
    info = r.info()
    assert info["arithmetic"] == build and info["traversal"] == traversal, (walk, info)
    assert info["shade_variant"].startswith("volumetric"), info
    n = r.stats()["launches"]
    assert n["extend"] > 0 and n["shadow"] == n["extend"] * (per_iter if null_surfaces else 1), (walk, n)
