"""`Renderer` — drop-in for AdaPT's `pt` renderer class, backed by the HIP library.

Mirrors the contract `render.py` drives in the reference (reference
`renderer/vanilla_renderer.py:23-124`, `tracer/path_tracer.py:181-211`,
`tracer/tracer_base.py:36-102`):

    rdr = Renderer(emitters, array_info, objects, prop)      # same four values scene_parsing returns
    rdr.render(t_start, t_end, s_start, s_end, max_bnc, max_depth)   # +1 spp; the six ints are ignored, as upstream
    rdr.pixels.to_numpy()          # (w, h, 3) float32, index [x, y], linear radiance = color / cnt
    rdr.cnt[None], rdr.color.to_numpy(), rdr.w, rdr.h, rdr.do_crop, rdr.start_x ... rdr.end_y
    rdr.get_check_point() / rdr.load_check_point(d), rdr.reset(), rdr.summary()

Transient (time-resolved) output, `pt` only (DESIGN.md "Transient rendering"): `Renderer(..., transient=True)` bins every path
contribution by its optical length, camera to emitter, as AdaPT's BDPT does in TRANSIENT_CAM mode (bdpt.py:164-165):

    rdr.transient()                # (n_bins, w, h, 3) float32 [t, x, y]: summed radiance of bin t / cnt
    rdr.transient_counts()         # (n_bins, w, h) float32: contributions per bin (upstream's time_cnts)

Path-length images, `pt` only: `Renderer(..., path_lengths=True)` also keeps the render split by path length - the number
of segments, camera to emitter - and by how the emitter was reached (part 0: by a sampled ray, part 1: by a light sample):

    rdr.path_lengths()             # (max_bounce + 1, 2, w, h, 3) float32 [length - 1, part, x, y]; .sum((0, 1)) is `pixels`
    rdr.path_length_counts()       # (max_bounce + 1, 2, w, h) float32: contributions per cell
    rdr.emission(), rdr.direct(), rdr.indirect()      # (w, h, 3): length 1, length 2, lengths 3 and more

Light groups, `pt` only: `Renderer(..., light_groups=True)` also keeps the render split by the emitter the light came
from - in the order of the `emitters` list, named by `rdr.emitter_ids` - and by how it was reached (part 0: by a sampled ray, part 1: by a
light sample), and relights it on the device:

    rdr.light_groups()             # (n_emitters, 2, w, h, 3) float32 [emitter, part, x, y]; .sum((0, 1)) is `pixels`
    rdr.light_group_counts()       # (n_emitters, 2, w, h) float32: contributions per cell
    rdr.relit({"spot": 0.0, "pt": (2.0, 1.5, 1.0)})      # (w, h, 3): the image with those emitters' intensities scaled; the others keep gain 1

Adaptive sampling, `pt` and `vpt`: `Renderer(..., adaptive={"threshold": 0.02, "min_spp": 64, "step": 32})` retires a pixel
once the relative standard error of its mean is at most `threshold`; decisions fall on global sample numbers that are multiples of `step`
and >= `min_spp`.  `render(n)` still advances `cnt` by n (the most samples any pixel has); `pixels` divides by each pixel's own count:

    rdr.sample_counts()            # (w, h) int32: n_p
    rdr.std_error()                # (w, h, 3) float64: standard error of each pixel's mean
    rdr.relative_error()           # (w, h) float64: e_p, the quantity the threshold is held against
    rdr.active_fraction()          # share of this rank's sampled pixels that still sample

Feature buffers and denoiser, `pt` on one rank: `Renderer(..., aov_spp=32)`.  The camera ray of a pixel-sample is a pure
function of (pixel, sample number, seed), so a pass of its own restates the rays of samples 1..min(cnt, aov_spp) and records what they hit:

    rdr.aov()                      # {"albedo": (w,h,3), "normal": (w,h,3), "depth": (w,h), "hit_fraction": (w,h)} float32, means over the hits
    rdr.denoised(**cfg)            # (w, h, 3): `pixels` through the firefly filter (firefly_threshold > 0) and the a-trous filter guided by aov()
    rdr.firefly_filtered(0.4)      # (w, h, 3): the firefly filter alone (upstream's post_processing.py)

Extensions (keyword-only, all optional): `n_spp=` on render() to queue many samples per
call (the wavefront batches them), `device/rank/world_size/band_width` for image-tile
sharding across GPUs, `seed`, `spp_per_batch`, `profile`, and film/bounce overrides so the
BASELINE configs can be run from one scene file.
"""
from __future__ import annotations

import ctypes as C
import time
from collections import namedtuple
from typing import List, Optional

import numpy as np

from . import _lib
from .scene_pack import FlatScene, RenderConfig, make_config, pack_scene
from .tiles import TilePlan

__all__ = ["Renderer", "VolumeRenderer", "AORenderer", "SSAORenderer", "BlinnPhongTracer", "DeviceScene", "bxdf_probe", "medium_probe", "volume_probe", "rng_stream", "adaptive_config", "adaptive_segments", "relative_error", "DENOISE_DEFAULTS"]

ADAPTIVE_DEFAULTS = {"min_spp": 64, "step": 32}
# apt_denoise_cfg's defaults (include/adapt_mi.h; DESIGN.md §4.7 says how they were chosen)
DENOISE_DEFAULTS = {"firefly_threshold": 0.0, "iterations": 3, "sigma_n": 128.0, "sigma_z": 0.1, "sigma_a": 0.1, "sigma_c": 1.0, "demodulate": True}
# apt_renderer_info's trace_mode -> name: TRACE_BVH, TRACE_SWEEP, TRACE_TILE, TRACE_FLAT (csrc/stages.hpp), the words of csrc/api.hip kTraversalName in its order
TRAVERSAL_NAMES = dict(enumerate(("bvh", "sweep", "tile", "flat")))
BVH_BUILDER_NAMES = dict(enumerate(("sah", "lbvh", "ploc")))      # apt_scene_bvh_builder: what built the scene's tree, after any fallback
# The split renders, by the Renderer option that switches one on.  n: the attribute with the number of leading planes
# (0: the mode is off); inner: the plane shape between it and (n_cols, h, 4); read / set: the library's entry points; key: the planes'
# checkpoint key; missing: what a renderer created without the option says.
_Split = namedtuple("_Split", "n inner read set key missing")
SPLIT_MODES = {
    "transient": _Split("n_bins", (), "apt_read_transient", "apt_set_transient", "transient_bins",
                        "this renderer was created without transient=...: there are no time bins"),
    "path_lengths": _Split("n_lengths", (2,), "apt_read_path_lengths", "apt_set_path_lengths", "path_length_planes",
                           "this renderer was created without path_lengths=True: there are no path-length planes"),
    "light_groups": _Split("n_groups", (2,), "apt_read_light_groups", "apt_set_light_groups", "light_group_planes",
                           "this renderer was created without light_groups=True: there are no light-group planes"),
}


def adaptive_config(adaptive) -> Optional[dict]:
    """None / False -> None (uniform sampling); a dict with "threshold" (> 0) and optionally "min_spp" and "step" (> 0) -> the full dict."""
    if adaptive is None or adaptive is False:
        return None
    if not isinstance(adaptive, dict):
        raise TypeError("adaptive must be None or a dict {'threshold': t, 'min_spp': 64, 'step': 32}")
    unknown = set(adaptive) - {"threshold", "min_spp", "step"}
    if unknown:
        raise ValueError(f"adaptive: unknown key(s) {sorted(unknown)}")
    cfg = {"threshold": float(adaptive["threshold"]), **{k: int(adaptive.get(k, v)) for k, v in ADAPTIVE_DEFAULTS.items()}}
    if not (np.isfinite(cfg["threshold"]) and cfg["threshold"] > 0):
        raise ValueError("adaptive: threshold must be a finite number > 0")
    if cfg["min_spp"] <= 0 or cfg["step"] <= 0:
        raise ValueError("adaptive: min_spp and step must be > 0")
    return cfg


def _moments(s1, s2, n):
    """(mean, standard error) per channel in float64; NaN where n < 2"""
    s1 = np.asarray(s1, np.float64); s2 = np.asarray(s2, np.float64)
    nd = np.asarray(n, np.float64)[..., None]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        mean = s1 / nd
        v = s2 / nd - mean * mean
        v = np.where(v < 0.0, 0.0, v)
        se = np.sqrt(v * (nd / (nd - 1.0)) / nd)
    return mean, np.where(nd >= 2, se, np.nan)


def relative_error(s1, s2, n) -> np.ndarray:
    """e_p = max over channels of se / (mean + 1e-3); +inf where that is not finite (n < 2, an inf sample).  The device's k_adaptive_retire
    evaluates the same expressions in the same order."""
    mean, se = _moments(s1, s2, n)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ratio = se / (mean + 1e-3)
    fin = np.all(np.isfinite(ratio), axis=-1)
    return np.where(fin, np.where(fin[..., None], ratio, 0.0).max(axis=-1), np.inf)


def _fp(a):
    return a.ctypes.data_as(_lib.f32p)


def _ip(a):
    return a.ctypes.data_as(_lib.i32p)


def bxdf_probe(bxdf_i, bxdf_f, dirs12, world_ior: float = 1.0, sample: bool = False, seed: int = 0, device: int = 0) -> np.ndarray:
    """Run the device surface models on explicit inputs (apt_bxdf_probe): eval+pdf -> (n,4), sample -> (n,9)."""
    lib = _lib.load()
    bi = np.ascontiguousarray(bxdf_i, np.int32).reshape(-1, 4)
    bf = np.ascontiguousarray(bxdf_f, np.float32).reshape(-1, 13)
    dd = np.ascontiguousarray(dirs12, np.float32).reshape(-1, 12)
    n = bi.shape[0]
    out = np.zeros((n, 9 if sample else 4), np.float32)
    _lib.check(lib.apt_bxdf_probe(int(device), n, _ip(bi), _fp(bf), _fp(dd), float(world_ior), int(bool(sample)), int(seed) & 0xffffffff, _fp(out)),
               "apt_bxdf_probe")
    return out


def medium_probe(med_i, med_f, mode: int, in7, seed: int = 0, device: int = 0) -> np.ndarray:
    """apt_medium_probe: per test a medium row (type, 16 floats) and 7 inputs -> (n, 8); mode 0 sample_mfp, 1 sample_new_rays, 2 eval + transmittance"""
    lib = _lib.load()
    mi = np.ascontiguousarray(med_i, np.int32).reshape(-1); mf = np.ascontiguousarray(med_f, np.float32).reshape(-1, 16)
    x = np.ascontiguousarray(in7, np.float32).reshape(-1, 7)
    out = np.zeros((x.shape[0], 8), np.float32)
    _lib.check(lib.apt_medium_probe(int(device), x.shape[0], _ip(mi), _fp(mf), int(mode), _fp(x), int(seed) & 0xffffffff, _fp(out)), "apt_medium_probe")
    return out


def volume_probe(vol_i, vol_f, vol_grid, mode: int, in10, seed: int = 0, device: int = 0) -> np.ndarray:
    """apt_volume_probe: one packed grid volume (FlatScene.vol_i / vol_f / vol_grid) and 10 inputs per test -> (n, 8); mode 0 intersect,
    1 density lookup, 2 sample_mfp (delta tracking), 3 transmittance (ratio tracking)"""
    lib = _lib.load()
    vi = np.ascontiguousarray(vol_i, np.int32).reshape(-1); vf = np.ascontiguousarray(vol_f, np.float32).reshape(-1)
    vg = np.ascontiguousarray(vol_grid, np.float32).reshape(-1)
    if vi.shape[0] != 5 or vf.shape[0] != 33 or vg.shape[0] != 3 * max(int(vi[1]), 0) * max(int(vi[2]), 0) * max(int(vi[3]), 0):
        raise ValueError("volume_probe: vol_i (5,), vol_f (33,) and a vol_grid of zres * yres * xres * 3 values")
    x = np.ascontiguousarray(in10, np.float32).reshape(-1, 10)
    out = np.zeros((x.shape[0], 8), np.float32)
    _lib.check(lib.apt_volume_probe(int(device), x.shape[0], _ip(vi), _fp(vf), _fp(vg), int(mode), _fp(x), int(seed) & 0xffffffff, _fp(out)), "apt_volume_probe")
    return out


def rng_stream(pixel: int, seed: int, sample: int, n: int, device: int = 0) -> np.ndarray:
    lib = _lib.load()
    out = np.zeros(n, np.uint32)
    _lib.check(lib.apt_rng_stream(int(device), pixel & 0xffffffff, seed & 0xffffffff, sample & 0xffffffff, int(n),
                                  out.ctypes.data_as(_lib.u32p)), "apt_rng_stream")
    return out


def adaptive_segments(cnt: int, n_spp: int, min_spp: int, step: int) -> list:
    """How one render call of an adaptive renderer at sample count `cnt` is split (api.hip render_adaptive does the same): a list of
    (first sample, last sample, decides) per round piece - a piece ends at the next decision point (a multiple of `step` that is
    >= `min_spp`), where the retirement rule runs, or where the call ends, and the next call continues the round."""
    out, left = [], int(n_spp)
    while left > 0:
        first = max(int(min_spp), cnt + 1)
        decide = -(-first // int(step)) * int(step)
        seg = min(left, decide - cnt)
        out.append((cnt + 1, cnt + seg, cnt + seg == decide))
        cnt += seg
        left -= seg
    return out


class DeviceScene:
    """Scene arrays resident in HBM (apt_scene handle); shareable by several renderers on one device."""

    def __init__(self, fs: FlatScene, device: int = 0, lib=None):
        lib = lib or _lib.load()
        self.lib = lib                          # the build this scene lives in (adapt_amd/_lib.py: "fast" or "exact"); handles never cross builds
        self.fs, self.device = fs, device
        keep = [np.ascontiguousarray(a) for a in (fs.prims, fs.normals, fs.v_normals, fs.obj_info, fs.obj_aabb, fs.emitter_id,
                                                  fs.bxdf_i, fs.bxdf_f, fs.src_i, fs.src_f)]
        p, n, vn, oi, ab, ei, bi, bf, si, sf = keep
        desc = _lib.SceneDesc(fs.n_prims, fs.n_objects, fs.n_sources, int(fs.has_vertex_normal), _fp(p), _fp(n), _fp(vn), _ip(oi),
                              _fp(ab), _ip(ei), _ip(bi), _fp(bf), _ip(si), _fp(sf), float(fs.world_ior))
        if fs.has_textures:                     # image textures: uv coordinates, per-object records, one atlas per map
            tex = [np.ascontiguousarray(fs.uvs, np.float32), np.ascontiguousarray(fs.tex_i, np.int32), np.ascontiguousarray(fs.tex_f, np.float32)]
            keep += tex
            desc.uvs, desc.tex_i, desc.tex_f = _fp(tex[0]), _ip(tex[1]), _fp(tex[2])
            for m, img in enumerate(fs.atlas):
                if img is not None:
                    img = np.ascontiguousarray(img, np.float32); keep.append(img)
                    desc.atlas[m] = _fp(img); desc.atlas_h[m], desc.atlas_w[m] = int(img.shape[0]), int(img.shape[1])
        if fs.med_i is not None:                # participating media (read by the volumetric tracer only)
            med = [np.ascontiguousarray(fs.med_i, np.int32), np.ascontiguousarray(fs.med_f, np.float32)]
            keep += med
            desc.med_i, desc.med_f = _ip(med[0]), _fp(med[1])
        if fs.vol_i is not None:                # grid volume (read by the volumetric tracer only)
            vol = [np.ascontiguousarray(fs.vol_i, np.int32), np.ascontiguousarray(fs.vol_f, np.float32), np.ascontiguousarray(fs.vol_grid, np.float32)]
            keep += vol
            desc.vol_i, desc.vol_f, desc.vol_grid = _ip(vol[0]), _fp(vol[1]), _fp(vol[2])
        h = C.c_void_p()
        _lib.check(lib.apt_scene_create(C.byref(desc), int(device), C.byref(h)), "apt_scene_create", lib)
        self.handle = h

    def texture_query(self, maps, objs, uv):
        """Texture.query on the device (parity probe): maps 0 albedo / 1 normal / 2 bump, (n,2) coordinates -> (n,3)"""
        mo = np.ascontiguousarray(np.stack([np.int32(maps), np.int32(objs)], 1), np.int32)
        uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        out = np.zeros((uv.shape[0], 3), np.float32)
        _lib.check(self.lib.apt_texture_probe(self.handle, uv.shape[0], _ip(mo), _fp(uv), _fp(out)), "apt_texture_probe", self.lib)
        return out

    def surface_maps(self, prims, bary, first_hit=True):
        """The normal, bump and albedo maps of a vertex on the device (parity probe of shade_stage.hpp surface_maps): primitives, (n,2)
        barycentrics, first-hit flag(s) -> k_d (n,3), n_s (n,3), the maps that applied (n,) as 1 albedo | 2 normal | 4 bump"""
        bary = np.ascontiguousarray(bary, np.float32).reshape(-1, 2)
        pf = np.ascontiguousarray(np.stack(np.broadcast_arrays(np.int32(prims), np.int32(first_hit)), -1).reshape(-1, 2), np.int32)
        if pf.shape[0] != bary.shape[0]:
            raise ValueError("surface_maps: one primitive per row of barycentrics")
        out = np.zeros((bary.shape[0], 7), np.float32)
        _lib.check(self.lib.apt_surface_maps_probe(self.handle, bary.shape[0], _ip(pf), _fp(bary), _fp(out)), "apt_surface_maps_probe", self.lib)
        return out[:, 0:3].copy(), out[:, 3:6].copy(), out[:, 6].astype(np.int32)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.apt_scene_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Counter:
    """`rdr.cnt[None]` (tracer_base.py:102)."""

    def __init__(self, owner): self._o = owner
    def __getitem__(self, _): return self._o._cnt
    def __setitem__(self, _, v): self._o._set_cnt(int(v))


class _FieldView:
    """`rdr.pixels` / `rdr.color`: objects with .to_numpy() -> (w, h, 3) float32 [x][y]."""

    def __init__(self, owner, normalised: bool): self._o, self._n = owner, normalised
    def to_numpy(self): return self._o._image(self._n)
    def from_numpy(self, arr): self._o._steady_only("color.from_numpy"); self._o._set_accum(np.asarray(arr, np.float32), self._o._cnt)
    @property
    def shape(self): return (self._o.w, self._o.h)


class Renderer:
    VOLUMETRIC = False          # subclass switch: VolumeRenderer renders with the reference's vpt semantics

    def __init__(self, emitters: List, array_info: dict, objects: List, prop: dict, *,
                 device: int = 0, rank: int = 0, world_size: int = 1, band_width: int = 4,
                 seed: int = 0, spp_per_batch: int = 0, profile: bool = False,
                 width: Optional[int] = None, height: Optional[int] = None,
                 max_bounce: Optional[int] = None, num_shadow_ray: Optional[int] = None, volumetric: Optional[bool] = None,
                 exact: Optional[bool] = None, transient=None, adaptive=None, aov_spp: int = 32, path_lengths: bool = False,
                 light_groups: bool = False):
        # transient = None / False: steady state; True: time bins from the sensor's sample_count / min_time / interval; a dict overrides them
        # (scene_pack.transient_config).  Surface renderer, at most 4 light samples per vertex, one rank: apt_renderer_create refuses the rest.
        # path_lengths = True: also keep one image per path length and part; the same limits as transient, and not with it
        # or with adaptive: apt_renderer_create refuses the rest.
        # light_groups = True: also keep one image per emitter and part; the same limits again, and not with path_lengths.
        # exact = True: the bit-parity build (the reference's float32 arithmetic operation for operation; debugging and the exact
        # parity tests), False: the fast build, None: whatever adapt_amd._lib currently hands out (fast unless APT_EXACT=1)
        # adaptive = None: every pixel takes every sample; a dict {"threshold", "min_spp", "step"}: adaptive sampling (adaptive_config)
        self.adaptive = adaptive_config(adaptive)
        self.lib = _lib.load(None if exact is None else ("exact" if exact else "fast"))
        self.arithmetic = _lib.arithmetic(self.lib)
        if volumetric is None:
            volumetric = self.VOLUMETRIC
        self.flat: FlatScene = pack_scene(emitters, array_info, objects, prop)
        self.rc: RenderConfig = make_config(prop, width=width, height=height, max_bounce=max_bounce,
                                            num_shadow_ray=num_shadow_ray, seed=seed, volumetric=bool(volumetric), transient=transient,
                                            path_lengths=bool(path_lengths), light_groups=bool(light_groups))
        self.volumetric = bool(volumetric)
        rc = self.rc
        # attributes the reference's callers read (watermark.py:23-30, render.py:129, path_tracer.py:181-193)
        self.w, self.h = rc.width, rc.height
        self.do_crop = rc.do_crop
        self.start_x, self.end_x, self.start_y, self.end_y = rc.start_x, rc.end_x, rc.start_y, rc.end_y
        self.crop_x, self.crop_y, self.crop_rx, self.crop_ry = rc.crop_x, rc.crop_y, rc.crop_rx, rc.crop_ry
        self.max_bounce, self.num_shadow_ray = rc.max_bounce, rc.num_shadow_ray
        self.use_rr, self.use_mis, self.anti_alias, self.stratified_sample = rc.use_rr, rc.use_mis, rc.anti_alias, rc.stratified
        self.focal, self.inv_focal = rc.focal, rc.inv_focal
        self.num_objects, self.num_prims, self.src_num = self.flat.n_objects, self.flat.n_prims, self.flat.n_sources
        self.cam_orient, self.cam_t, self.cam_r = rc.cam_orient, rc.cam_t, rc.cam_r
        self.device, self.rank, self.world_size = int(device), int(rank), int(world_size)
        self.plan = TilePlan(self.w, self.h, band_width if world_size > 1 else self.w, world_size)
        self._cnt = 0
        self._t0 = time.time()
        # feature buffers: the camera rays of samples 1..min(cnt, aov_spp) are restated on demand (aov()); _aov_n = how many are in
        self.aov_spp, self._aov_n = int(aov_spp), 0
        if self.aov_spp < 0:
            raise ValueError("aov_spp must be >= 0")

        self.scene = DeviceScene(self.flat, self.device, self.lib)
        cfg = _lib.RenderCfg()
        for name in ("width", "height", "start_x", "end_x", "start_y", "end_y", "max_bounce", "num_shadow_ray", "rr_bounce_th"):
            setattr(cfg, name, int(getattr(rc, name)))
        for name in ("do_crop", "use_rr", "use_mis", "anti_alias", "stratified", "brdf_two_sides"):
            setattr(cfg, name, int(bool(getattr(rc, name))))
        cfg.rr_threshold = float(rc.rr_threshold)
        cfg.cam_r = (C.c_float * 9)(*np.float32(rc.cam_r).reshape(-1).tolist())
        cfg.cam_t = (C.c_float * 3)(*np.float32(rc.cam_t).tolist())
        cfg.inv_focal, cfg.half_w, cfg.half_h = float(rc.inv_focal), float(rc.half_w), float(rc.half_h)
        cfg.seed = int(rc.seed) & 0xffffffff
        cfg.band_width, cfg.rank, cfg.world_size = self.plan.band_width, self.rank, self.world_size
        cfg.spp_per_batch, cfg.device, cfg.profile = int(spp_per_batch), self.device, int(bool(profile))
        cfg.volumetric = int(self.volumetric)
        cfg.transient_bins, cfg.transient_min_time, cfg.transient_interval = int(rc.transient_bins), float(rc.transient_min_time), float(rc.transient_interval)
        self.n_bins, self.min_time, self.interval = rc.transient_bins, rc.transient_min_time, rc.transient_interval
        cfg.path_lengths = int(bool(rc.path_lengths))
        self.n_lengths = rc.max_bounce + 1 if rc.path_lengths else 0          # planes kept: lengths 1 .. max_bounce + 1
        cfg.light_groups = int(bool(rc.light_groups))
        self.n_groups = self.flat.n_sources if rc.light_groups else 0           # planes kept: one pair per emitter
        self.emitter_ids = [getattr(e, "id", None) for e in emitters]           # the emitters' XML ids, in plane order
        if self.adaptive:
            cfg.adaptive_threshold = self.adaptive["threshold"]
            cfg.adaptive_min_spp, cfg.adaptive_step = self.adaptive["min_spp"], self.adaptive["step"]
        self._configure(cfg, prop)
        h = C.c_void_p()
        _lib.check(self.lib.apt_renderer_create(self.scene.handle, C.byref(cfg), C.byref(h)), "apt_renderer_create", self.lib)
        self.handle = h
        nc, hh = C.c_int32(0), C.c_int32(0)
        _lib.check(self.lib.apt_tile_shape(self.handle, C.byref(nc), C.byref(hh)), "apt_tile_shape", self.lib)
        self.n_cols = int(nc.value)
        assert self.n_cols == len(self.plan.columns(self.rank))
        self.cnt = _Counter(self)
        self.pixels = _FieldView(self, True)
        self.color = _FieldView(self, False)

    def _configure(self, cfg, prop: dict):
        """what a subclass adds to the apt_render_cfg before the handle is made (AORenderer: the ao block)"""

    # ------------------------------------------------------------ rendering
    def render(self, _t_start: int = 0, _t_end: int = 0, _s_start: int = 0, _s_end: int = 0, _a: int = 0, _b: int = 0,
               *, n_spp: int = 1):
        """Accumulate `n_spp` more samples for every owned pixel (asynchronous; reads synchronise)."""
        _lib.check(self.lib.apt_render(self.handle, int(n_spp)), "apt_render", self.lib)
        self._cnt += int(n_spp)

    def synchronize(self):
        _lib.check(self.lib.apt_synchronize(self.handle), "apt_synchronize", self.lib)

    def reset(self):
        """Leaves the render alone, exactly like the reference (`TracerBase.reset` is an empty kernel, tracer_base.py:284-286); the
        feature buffers, which can be restated at any time, start over."""
        self._clear_aov()

    def clear(self):
        """Zero the accumulation, the sample counter, the statistics, the transient bins, the path-length and light-group planes and the feature buffers."""
        _lib.check(self.lib.apt_reset(self.handle), "apt_reset", self.lib)
        self._cnt = 0
        self._aov_n = 0

    # ------------------------------------------------- feature buffers and denoiser
    def _clear_aov(self):
        if getattr(self, "handle", None) and self._aov_n:
            _lib.check(self.lib.apt_clear_aov(self.handle), "apt_clear_aov", self.lib)
        self._aov_n = 0

    def _update_aov(self):
        """Bring the feature buffers to the camera rays of samples 1..min(cnt, aov_spp): a top-up after more rendering, a fresh start where
        the sample counter went back."""
        want = min(self._cnt, self.aov_spp)
        if want < self._aov_n:
            self._clear_aov()
        _lib.check(self.lib.apt_render_aov(self.handle, self._aov_n, want - self._aov_n), "apt_render_aov", self.lib)      # (refuses vpt and ranks even with nothing to add)
        self._aov_n = want

    def tile_aov(self) -> np.ndarray:
        """The raw sums, (w, h, 8) float32: albedo rgb, depth, normal xyz, hit count - over the camera rays of samples 1..min(cnt, aov_spp)."""
        self._update_aov()
        out = np.empty((self.n_cols, self.h, 8), np.float32)
        _lib.check(self.lib.apt_read_aov(self.handle, _fp(out)), "apt_read_aov", self.lib)
        return out

    def aov(self) -> dict:
        """What the camera rays hit first: albedo (w,h,3) - the diffuse colour the shade stage reads, record or texture -, normal (w,h,3) -
        the shading normal after the maps, world space, renormalised mean -, depth (w,h) and hit_fraction (w,h).  Means over the rays that
        hit, 0 where none did; hit_fraction = hits / samples covered (0 outside a crop window)."""
        raw = self.tile_aov()
        n = raw[..., 7]
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = np.where(n[..., None] > 0, raw[..., :7] / n[..., None], np.float32(0)).astype(np.float32)
            normal = mean[..., 4:7]
            length = np.sqrt((normal[..., 0] * normal[..., 0] + normal[..., 1] * normal[..., 1]) + normal[..., 2] * normal[..., 2])
            normal = np.where(length[..., None] > 0, normal / length[..., None], normal).astype(np.float32)
        return {"albedo": np.ascontiguousarray(mean[..., 0:3]), "normal": np.ascontiguousarray(normal), "depth": np.ascontiguousarray(mean[..., 3]),
                "hit_fraction": (n / np.float32(max(1, self._aov_n))).astype(np.float32)}

    def _denoise(self, cfg: dict, colour) -> np.ndarray:
        unknown = set(cfg) - set(DENOISE_DEFAULTS) - {"firefly_only"}
        if unknown:
            raise ValueError(f"denoise: unknown setting(s) {sorted(unknown)}")
        c = {**DENOISE_DEFAULTS, "firefly_only": False, **cfg}
        dc = _lib.DenoiseCfg(float(c["firefly_threshold"]), int(bool(c["firefly_only"])), int(c["iterations"]), float(c["sigma_n"]), float(c["sigma_z"]),
                             float(c["sigma_a"]), float(c["sigma_c"]), int(bool(c["demodulate"])))
        if not c["firefly_only"]:
            self._update_aov()                    # the guides: up to date before the filter reads them
        src = None
        if colour is not None:
            src = np.ascontiguousarray(colour, np.float32)
            if src.shape != (self.w, self.h, 3):
                raise ValueError(f"denoise: colour must be ({self.w},{self.h},3), got {src.shape}")
        out = np.empty((self.w, self.h, 3), np.float32)
        _lib.check(self.lib.apt_denoise(self.handle, C.byref(dc), _fp(src) if src is not None else None, _fp(out)), "apt_denoise", self.lib)
        return out

    def denoised(self, colour=None, **cfg) -> np.ndarray:
        """(w, h, 3) float32: `pixels` (or `colour`, a (w,h,3) image of this film) through the firefly filter (firefly_threshold > 0) and K
        iterations of the a-trous filter guided by aov().  Settings: DENOISE_DEFAULTS."""
        return self._denoise(cfg, colour)

    def firefly_filtered(self, threshold: float = 0.4, colour=None) -> np.ndarray:
        """(w, h, 3) float32: upstream's firefly filter alone (post_processing.py; its THRESHOLD is 0.4)."""
        return self._denoise({"firefly_threshold": threshold, "firefly_only": True}, colour)

    # ------------------------------------------------------------- readback
    def tile_accum(self) -> np.ndarray:
        """This rank's accumulation tile, (n_cols, h, 3) float32."""
        out = np.empty((self.n_cols, self.h, 3), np.float32)
        c = C.c_int32(0)
        _lib.check(self.lib.apt_get_accum(self.handle, _fp(out), C.byref(c)), "apt_get_accum", self.lib)
        return out

    def tile_pixels(self) -> np.ndarray:
        out = np.empty((self.n_cols, self.h, 3), np.float32)
        _lib.check(self.lib.apt_read_pixels(self.handle, _fp(out)), "apt_read_pixels", self.lib)
        return out

    def _image(self, normalised: bool) -> np.ndarray:
        tile = self.tile_pixels() if normalised else self.tile_accum()
        if self.world_size == 1:
            return tile
        from .tiles import gather_image
        return gather_image(self, normalised)          # (adaptive: divided by the gathered per-pixel counts)

    # ----------------------------------------------------------- split renders (SPLIT_MODES)
    def _need_split(self, mode: str):
        if not getattr(self, SPLIT_MODES[mode].n):
            raise RuntimeError(SPLIT_MODES[mode].missing)

    def _split_shape(self, mode: str) -> tuple:
        m = SPLIT_MODES[mode]
        return (getattr(self, m.n), *m.inner, self.n_cols, self.h, 4)

    def _read_split(self, mode: str) -> np.ndarray:
        """this rank's raw cells: summed r, g, b and the number of contributions"""
        self._need_split(mode)
        out = np.empty(self._split_shape(mode), np.float32)
        _lib.check(getattr(self.lib, SPLIT_MODES[mode].read)(self.handle, _fp(out)), SPLIT_MODES[mode].read, self.lib)
        return out

    def _set_split(self, mode: str, cells: np.ndarray):
        cells = np.ascontiguousarray(cells, np.float32)
        _lib.check(getattr(self.lib, SPLIT_MODES[mode].set)(self.handle, _fp(cells)), SPLIT_MODES[mode].set, self.lib)

    def _split_radiance(self, mode: str) -> np.ndarray:
        """the cells' rgb divided by the sample count like `pixels`"""
        return self._read_split(mode)[..., :3] / np.float32(self._cnt if self._cnt > 0 else 1)

    def _split_counts(self, mode: str) -> np.ndarray:
        return np.ascontiguousarray(self._read_split(mode)[..., 3])

    def tile_transient(self) -> np.ndarray:
        """This rank's raw bins, (n_bins, n_cols, h, 4) float32: summed r, g, b and the number of contributions."""
        return self._read_split("transient")

    def transient(self) -> np.ndarray:
        """(n_bins, w, h, 3) float32, index [t, x, y]: the radiance that arrived in time bin t, divided by the sample count like `pixels`.
        With a window that holds every path the bins sum to the steady image."""
        return self._split_radiance("transient")

    def transient_counts(self) -> np.ndarray:
        """(n_bins, w, h) float32: the number of contributions per bin (divide transient() * cnt by it for bdpt.py's copy_average)."""
        return self._split_counts("transient")

    def tile_path_lengths(self) -> np.ndarray:
        """This rank's raw planes, (max_bounce + 1, 2, n_cols, h, 4) float32, index [length - 1, part, x, y]: summed r, g, b and the number
        of contributions.  Part 0: the emitter was reached by a sampled ray, part 1: by a light sample."""
        return self._read_split("path_lengths")

    def path_lengths(self) -> np.ndarray:
        """(max_bounce + 1, 2, w, h, 3) float32: the radiance that arrived over paths of each length, by part, divided by the sample count
        like `pixels`; summed over lengths and parts it is `pixels` up to float summation order."""
        return self._split_radiance("path_lengths")

    def path_length_counts(self) -> np.ndarray:
        """(max_bounce + 1, 2, w, h) float32: the number of contributions per cell."""
        return self._split_counts("path_lengths")

    def emission(self) -> np.ndarray:
        """(w, h, 3): length 1, the emitters as the camera sees them."""
        return self.path_lengths()[0].sum(0)

    def direct(self) -> np.ndarray:
        """(w, h, 3): length 2, direct illumination - both parts, the two MIS strategies ((w, h, 3) of zeros with max_bounce = 0)."""
        return self.path_lengths()[1:2].sum((0, 1))

    def indirect(self) -> np.ndarray:
        """(w, h, 3): lengths 3 and more."""
        return self.path_lengths()[2:].sum((0, 1))

    def tile_light_groups(self) -> np.ndarray:
        """This rank's raw planes, (n_emitters, 2, n_cols, h, 4) float32, index [emitter, part, x, y]: summed r, g, b and the number of
        contributions.  Part 0: the emitter was reached by a sampled ray, part 1: by a light sample."""
        return self._read_split("light_groups")

    def light_groups(self) -> np.ndarray:
        """(n_emitters, 2, w, h, 3) float32: the radiance that came from each emitter, by part, divided by the sample count like `pixels`;
        summed over emitters and parts it is `pixels` up to float summation order."""
        return self._split_radiance("light_groups")

    def light_group_counts(self) -> np.ndarray:
        """(n_emitters, 2, w, h) float32: the number of contributions per cell."""
        return self._split_counts("light_groups")

    def light_gains(self, gains) -> np.ndarray:
        """-> (n_emitters, 3) float32 from a scalar per emitter, an rgb triple per emitter, or a dict from emitter id to either (emitters
        the dict does not name keep gain 1)."""
        self._need_split("light_groups")
        out = np.ones((self.n_groups, 3), np.float32)
        if isinstance(gains, dict):
            for key, g in gains.items():
                if key not in self.emitter_ids:
                    raise KeyError(f"no emitter with id {key!r}; this scene has {self.emitter_ids}")
                out[self.emitter_ids.index(key)] = np.broadcast_to(np.asarray(g, np.float32), (3,))
            return out
        g = np.asarray(gains, np.float32)
        if g.shape == (self.n_groups,):
            g = g[:, None]
        if g.shape not in ((self.n_groups, 1), (self.n_groups, 3)):
            raise ValueError(f"gains: one scalar or one rgb triple per emitter ({self.n_groups} emitters), or a dict by emitter id; got shape {g.shape}")
        out[:] = g
        return out

    def relit(self, gains) -> np.ndarray:
        """(w, h, 3) float32: the image with every emitter's share multiplied by its gain (`light_gains`), combined on the device
        (apt_relight) - what `pixels` would be had the emitters' intensities been scaled, on the same random stream."""
        g = np.ascontiguousarray(self.light_gains(gains))
        out = np.empty((self.n_cols, self.h, 3), np.float32)
        _lib.check(self.lib.apt_relight(self.handle, _fp(g), _fp(out)), "apt_relight", self.lib)
        return out

    def _set_cnt(self, v: int):
        self._steady_only("cnt[None] = ...")
        self._set_accum(self.tile_accum(), v)

    def _steady_only(self, what: str):
        if self.adaptive:
            raise RuntimeError(f"{what}: an adaptive renderer's per-pixel counts and moments would not follow; use load_check_point")

    # ----------------------------------------------------------- adaptive sampling
    def _need_adaptive(self):
        if not self.adaptive:
            raise RuntimeError("this renderer was created without adaptive=...: every pixel has cnt samples")

    def tile_sample_counts(self, with_mask: bool = False):
        """This rank's per-pixel sample counts, (n_cols, h) int32; with_mask: also the active flags, (n_cols, h) bool."""
        self._need_adaptive()
        n = np.empty((self.n_cols, self.h), np.int32)
        act = np.empty((self.n_cols, self.h), np.uint8)
        _lib.check(self.lib.apt_read_sample_counts(self.handle, _ip(n), act.ctypes.data_as(_lib.u8p)), "apt_read_sample_counts", self.lib)
        return (n, act.astype(bool)) if with_mask else n

    def tile_moments(self) -> np.ndarray:
        """This rank's float64 sums of squared sample values, (n_cols, h, 3)."""
        self._need_adaptive()
        s2 = np.empty((self.n_cols, self.h, 3), np.float64)
        _lib.check(self.lib.apt_read_moments(self.handle, s2.ctypes.data_as(_lib.f64p)), "apt_read_moments", self.lib)
        return s2

    def _tile_of(self, arr, tail, dtype):
        arr = np.ascontiguousarray(arr, dtype)
        if arr.shape == (self.n_cols, self.h) + tail:
            return arr
        if arr.shape == (self.w, self.h) + tail:
            return np.ascontiguousarray(arr[self.plan.columns(self.rank)])
        raise ValueError(f"expected ({self.w},{self.h}){tail} or the tile ({self.n_cols},{self.h}){tail}, got {arr.shape}")

    def _set_adaptive_state(self, counts, s2, active):
        n = self._tile_of(counts, (), np.int32)
        m = self._tile_of(s2, (3,), np.float64)
        a = self._tile_of(np.asarray(active).astype(np.uint8), (), np.uint8)
        _lib.check(self.lib.apt_set_adaptive_state(self.handle, _ip(n), m.ctypes.data_as(_lib.f64p), a.ctypes.data_as(_lib.u8p)),
                   "apt_set_adaptive_state", self.lib)

    def _full(self, tile):
        if self.world_size == 1:
            return tile
        from .tiles import gather_array
        return gather_array(tile, self.plan, self.rank, self.world_size, device=self.device)

    def sample_counts(self) -> np.ndarray:
        """(w, h) int32: the samples each pixel has taken (0 outside a crop window); the largest is cnt."""
        return self._full(self.tile_sample_counts())

    def std_error(self) -> np.ndarray:
        """(w, h, 3) float64: the standard error of each pixel's mean, per channel (NaN below two samples)."""
        self._need_adaptive()
        return _moments(self._full(self.tile_accum()), self._full(self.tile_moments()), self._full(self.tile_sample_counts()))[1]

    def relative_error(self) -> np.ndarray:
        """(w, h) float64: e_p, what the retirement rule holds against the threshold (+inf where not finite)."""
        self._need_adaptive()
        return relative_error(self._full(self.tile_accum()), self._full(self.tile_moments()), self._full(self.tile_sample_counts()))

    def active_fraction(self) -> float:
        """The share of this rank's sampled pixels (inside the crop window) that still take samples."""
        n, act = self.tile_sample_counts(with_mask=True)
        sampled = self._crop_mask().sum()
        return float(act.sum()) / float(max(1, sampled))

    def _crop_mask(self) -> np.ndarray:
        cols = self.plan.columns(self.rank)[:, None]
        rows = np.arange(self.h)[None, :]
        if not self.do_crop:
            return np.ones((self.n_cols, self.h), bool)
        return (cols >= self.start_x) & (cols < self.end_x) & (rows >= self.start_y) & (rows < self.end_y)

    def _set_accum(self, arr: np.ndarray, cnt: int):
        arr = np.ascontiguousarray(arr, np.float32)
        if arr.shape != (self.n_cols, self.h, 3):
            if arr.shape == (self.w, self.h, 3):
                arr = np.ascontiguousarray(arr[self.plan.columns(self.rank)])
            else:
                raise ValueError(f"accumulation must be ({self.w},{self.h},3) or the tile ({self.n_cols},{self.h},3)")
        _lib.check(self.lib.apt_set_accum(self.handle, _fp(arr), int(cnt)), "apt_set_accum", self.lib)
        self._cnt = int(cnt)

    def device_accum_ptr(self) -> int:
        p, c = C.c_void_p(), C.c_int32(0)
        _lib.check(self.lib.apt_device_ptr(self.handle, C.byref(p), C.byref(c)), "apt_device_ptr", self.lib)
        return int(p.value)

    def stream_ptr(self) -> int:
        p = C.c_void_p()
        _lib.check(self.lib.apt_stream(self.handle, C.byref(p)), "apt_stream", self.lib)
        return int(p.value or 0)

    def stats(self) -> dict:
        st = _lib.Stats()
        _lib.check(self.lib.apt_get_stats(self.handle, C.byref(st)), "apt_get_stats", self.lib)
        return st.as_dict()

    # ----------------------------------------------------------- unit entry points
    def intersect(self, o, d):
        o = np.ascontiguousarray(o, np.float32).reshape(-1, 3); d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        n = o.shape[0]
        prim, t, uv = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros((n, 2), np.float32)
        _lib.check(self.lib.apt_intersect(self.handle, n, _fp(o), _fp(d), _ip(prim), _fp(t), _fp(uv)), "apt_intersect", self.lib)
        return prim, t, uv

    def occluded(self, o, d, tmax):
        o = np.ascontiguousarray(o, np.float32).reshape(-1, 3); d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        tmax = np.ascontiguousarray(tmax, np.float32).reshape(-1)
        occ = np.zeros(o.shape[0], np.int32)
        _lib.check(self.lib.apt_occluded(self.handle, o.shape[0], _fp(o), _fp(d), _fp(tmax), _ip(occ)), "apt_occluded", self.lib)
        return occ

    def emitter_probe(self, in11, seed: int = 0) -> np.ndarray:
        """apt_emitter_probe: rows (src index, hit_pos, normal, ray_d, min_depth) -> (n,12)."""
        x = np.ascontiguousarray(in11, np.float32).reshape(-1, 11)
        out = np.zeros((x.shape[0], 12), np.float32)
        _lib.check(self.lib.apt_emitter_probe(self.scene.handle, x.shape[0], _fp(x), int(seed) & 0xffffffff, _fp(out)), "apt_emitter_probe", self.lib)
        return out

    def info(self) -> dict:
        b, nq, lds, tm = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
        qb = C.c_int64(0)
        name = C.c_char_p()
        _lib.check(self.lib.apt_renderer_info(self.handle, C.byref(b), C.byref(nq), C.byref(qb), C.byref(lds), C.byref(name), C.byref(tm)), "apt_renderer_info", self.lib)
        bb = C.c_int32(0)
        _lib.check(self.lib.apt_scene_bvh_builder(self.scene.handle, C.byref(bb)), "apt_scene_bvh_builder", self.lib)
        return {"spp_per_batch": b.value, "n_subqueues": nq.value, "queue_bytes": qb.value, "lds_bytes": lds.value,
                "shade_variant": name.value.decode() if name.value else "",
                "traversal": TRAVERSAL_NAMES.get(tm.value, str(tm.value)), "bvh_builder": BVH_BUILDER_NAMES.get(bb.value, str(bb.value)), "arithmetic": self.arithmetic,
                "sampling": "adaptive" if self.adaptive else "uniform", **({"adaptive": dict(self.adaptive)} if self.adaptive else {})}

    def camera_fused(self) -> bool:
        """apt_renderer_camera_fused: the camera vertex is shaded by the kernel that traces the camera ray (rays traced in place, steady
        full-film renders; APT_CAMERA_FUSE=0 at creation switches it off)."""
        f = C.c_int32(0)
        _lib.check(self.lib.apt_renderer_camera_fused(self.handle, C.byref(f)), "apt_renderer_camera_fused", self.lib)
        return bool(f.value)

    def light_strips(self) -> bool:
        """apt_renderer_light_strips: the camera-fed kernel sweeps the camera vertex's light samples against per-strip masks that leave
        some pair of an occluder list out (APT_LIGHT_STRIPS=0 at creation switches them off; cropped and adaptive renders have none)."""
        f = C.c_int32(0)
        _lib.check(self.lib.apt_renderer_light_strips(self.handle, C.byref(f)), "apt_renderer_light_strips", self.lib)
        return bool(f.value)

    def record_staged(self) -> bool:
        """apt_renderer_record_staged: the queue-fed shade kernel stages each row's path record in LDS a row ahead (rays traced in place,
        Lambertian surfaces under point lights; APT_RECORD_STAGE=0 at creation switches it off)."""
        f = C.c_int32(0)
        _lib.check(self.lib.apt_renderer_record_staged(self.handle, C.byref(f)), "apt_renderer_record_staged", self.lib)
        return bool(f.value)

    def live_rows(self) -> bool:
        """apt_renderer_live_rows: the staged and the camera-fed shade kernel run their live-row form (rays traced in place, Lambertian
        surfaces under point lights; APT_LIVE_ROWS=0 at creation selects the kernels that give dead lanes default values)."""
        f = C.c_int32(0)
        _lib.check(self.lib.apt_renderer_live_rows(self.handle, C.byref(f)), "apt_renderer_live_rows", self.lib)
        return bool(f.value)

    def record_compact(self) -> bool:
        """apt_renderer_record_compact: the traced kernels carry the 56-byte path record - hit point instead of ray origin and hit distance,
        no pdf (rays traced in place, Lambertian surfaces under point lights; APT_RECORD_COMPACT=0 at creation keeps the 64-byte record)."""
        f = C.c_int32(0)
        _lib.check(self.lib.apt_renderer_record_compact(self.handle, C.byref(f)), "apt_renderer_record_compact", self.lib)
        return bool(f.value)

    # ------------------------------------------------------------ checkpoint
    def get_check_point(self) -> dict:
        """Same keys as the reference's pickle (path_tracer.py:181-193)."""
        return {"w": self.w, "h": self.h, "crop_x": self.crop_x, "crop_y": self.crop_y, "crop_rx": self.crop_rx,
                "crop_ry": self.crop_ry, "focal": self.focal, "num_objects": self.num_objects, "num_prims": self.num_prims,
                "cam_orient": np.array(self.cam_orient), "src_num": self.src_num, "cam_t": np.array(self.cam_t),
                "accumulation": self.color.to_numpy(), "counter": self._cnt,
                **{m.key: self._read_split(mode) for mode, m in SPLIT_MODES.items() if getattr(self, m.n)},
                **({"aov_sums": self.tile_aov(), "aov_samples": self._aov_n} if self._aov_n else {}),
                **(self._adaptive_check_point() if self.adaptive else {})}

    _ADAPTIVE_KEYS = ("adaptive", "sample_counts", "moments", "active")

    def _adaptive_check_point(self) -> dict:
        """this rank's tiles (the whole film with one rank): counts, moments and mask, and the settings they were made with"""
        n, act = self.tile_sample_counts(with_mask=True)
        return {"adaptive": dict(self.adaptive), "sample_counts": n, "moments": self.tile_moments(), "active": act}

    def load_check_point(self, check_point: dict):
        if self.adaptive and "moments" not in check_point:
            raise ValueError("this checkpoint has no per-pixel moments (a uniform render's): an adaptive renderer cannot continue it")
        if not self.adaptive and any(k in check_point for k in self._ADAPTIVE_KEYS):
            raise ValueError("this checkpoint is an adaptive render's: continue it with Renderer(..., adaptive=...)")
        for key, val in check_point.items():
            if key in ("accumulation", "counter", "aov_sums", "aov_samples") + tuple(m.key for m in SPLIT_MODES.values()) + self._ADAPTIVE_KEYS:
                continue
            if key in ("cam_t", "cam_orient"):
                ok = np.abs(np.asarray(val) - np.asarray(getattr(self, key))).max() < 1e-4
            else:
                ok = val == getattr(self, key)
            if not ok:
                raise ValueError(f"'{key}' from the checkpoint is different.")
        self._set_accum(np.asarray(check_point["accumulation"], np.float32), int(check_point["counter"]))
        if self.adaptive:
            self._set_adaptive_state(check_point["sample_counts"], check_point["moments"], check_point["active"])
        # feature buffers: taken from the checkpoint where it has them for this film; else they start over and aov() restates them
        self._clear_aov()
        sums = check_point.get("aov_sums")
        if sums is not None and np.shape(sums) == (self.n_cols, self.h, 8) and 0 < int(check_point.get("aov_samples", 0)) <= min(self._cnt, self.aov_spp):
            sums = np.ascontiguousarray(sums, np.float32)
            _lib.check(self.lib.apt_set_aov(self.handle, _fp(sums)), "apt_set_aov", self.lib)
            self._aov_n = int(check_point["aov_samples"])
        for mode, m in SPLIT_MODES.items():      # (a checkpoint of another layout, or of a render without the mode, leaves the cells as they are)
            cells = check_point.get(m.key)
            if getattr(self, m.n) and cells is not None and np.shape(cells) == self._split_shape(mode):
                self._set_split(mode, cells)

    def summary(self) -> str:
        self.synchronize()
        msg = f"{'VPT' if self.volumetric else 'PT'} SPP = {self._cnt}. Rendering time: {time.time() - self._t0:.3f} s"
        if self.adaptive:
            n = self.tile_sample_counts()[self._crop_mask()]
            msg += f". Adaptive: mean spp {n.mean() if n.size else 0.0:.1f}, {100.0 * (1.0 - self.active_fraction()):.1f} % of the pixels converged"
        print(msg)
        return msg

    def close(self):
        if getattr(self, "handle", None):
            self.lib.apt_renderer_destroy(self.handle)
            self.handle = None
        if getattr(self, "scene", None):
            self.scene.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


AO_DEFAULTS = {"smp_hemisphere": 32, "depth_samples": 64, "sample_extent": 0.1}      # ssao.py:36-38


def ao_settings(prop: dict, **over) -> dict:
    """The three settings of the ambient-occlusion renderer: a keyword that is not None, else the sensor's key, else upstream's default"""
    unknown = set(over) - set(AO_DEFAULTS)
    if unknown:
        raise ValueError(f"ambient occlusion: unknown setting(s) {sorted(unknown)}")
    return {k: type(d)(over[k] if over.get(k) is not None else prop.get(k, d)) for k, d in AO_DEFAULTS.items()}


class AORenderer(Renderer):
    """Drop-in for the reference's `SSAORenderer` (renderer/ssao.py; `--type ao`): same constructor and surface as `Renderer`, screen-space
    ambient occlusion instead of path tracing.  Creation renders the depth map; every sample traces the camera ray,
    draws `smp_hemisphere` directions about the hit's shading normal and holds the points `sample_extent` along them against the depth map.

        rdr = AORenderer(emitters, array_info, objects, prop)      # reads the sensor's smp_hemisphere / depth_samples / sample_extent
        rdr.render(0, 0, 0, 0, 0, 0)   # +1 spp (or render(n_spp=...))
        rdr.pixels.to_numpy()          # (w, h, 3): channel 0 of color / cnt on all three channels where the last sample's ray hit, else 0
        rdr.color.to_numpy()           # (w, h, 3): the sum of (1 - occlusion), zero, the depth map - upstream's checkpoint layout
        rdr.depth_map()                # (w, h): the mean hit distance of each pixel's depth_samples camera rays (0: none hit)

    The three settings can be overridden by keyword.  `reset()` leaves the render alone like upstream's; `clear()` zeroes channel 0 and the
    counter and keeps the depth map.  One rank, no split mode, no adaptive sampling, no feature buffers: apt_renderer_create refuses the rest."""

    def __init__(self, emitters: List, array_info: dict, objects: List, prop: dict, *, smp_hemisphere: Optional[int] = None,
                 depth_samples: Optional[int] = None, sample_extent: Optional[float] = None, **kw):
        if kw.get("aov_spp"):
            raise ValueError("AORenderer: ambient occlusion keeps no feature buffers (aov_spp must be 0); depth_map() is its depth")
        kw["aov_spp"] = 0
        self.ao = ao_settings(prop, smp_hemisphere=smp_hemisphere, depth_samples=depth_samples, sample_extent=sample_extent)
        self.smp_hemisphere, self.depth_samples, self.sample_extent = self.ao["smp_hemisphere"], self.ao["depth_samples"], self.ao["sample_extent"]
        super().__init__(emitters, array_info, objects, prop, **kw)

    def _configure(self, cfg, prop: dict):
        cfg.ao = 1
        cfg.ao_smp_hemisphere, cfg.ao_depth_samples, cfg.ao_sample_extent = self.smp_hemisphere, self.depth_samples, float(self.sample_extent)

    def depth_map(self) -> np.ndarray:
        """(w, h) float32, index [x, y]: the depth map (apt_read_ao_depth)"""
        out = np.empty((self.n_cols, self.h), np.float32)
        _lib.check(self.lib.apt_read_ao_depth(self.handle, _fp(out)), "apt_read_ao_depth", self.lib)
        return out

    def info(self) -> dict:
        return {**super().info(), "pipeline": "ao", "ao": dict(self.ao)}

    def summary(self) -> str:
        self.synchronize()
        msg = f"SSAO SPP = {self._cnt}. Rendering time: {time.time() - self._t0:.3f} s"
        print(msg)
        return msg


SSAORenderer = AORenderer


class _MapView:
    """`rdr.depth_map` / `rdr.norm_map`: objects with .to_numpy(), as upstream's fields"""

    def __init__(self, read): self._read = read
    def to_numpy(self): return self._read()


def light_positions(positions) -> np.ndarray:
    """(F, 3) float32 from one position or a sequence of them; a ValueError for any other shape or a non-finite coordinate"""
    p = np.ascontiguousarray(positions, np.float32)
    if p.ndim == 1:
        p = p.reshape(1, -1)
    if p.ndim != 2 or p.shape[1] != 3 or p.shape[0] == 0:
        raise ValueError(f"light positions: expected (3,) or (F, 3) with F >= 1, got {np.shape(positions)}")
    if not np.isfinite(p).all():
        raise ValueError("light positions: every coordinate must be finite")
    return p


def unlit_objects(objects: List) -> List:
    """copies of the objects with no emitter attached: the viewer shades emissive objects like any other (direct_render.py:49-60 reads no
    emitter reference), and its scene holds one light, the point source"""
    import copy
    out = []
    for o in objects:
        o = copy.copy(o)
        o.emitter_ref_id = -1
        out.append(o)
    return out


class BlinnPhongTracer(Renderer):
    """Drop-in for the reference's `BlinnPhongTracer` (renderer/direct_render.py): the direct-light viewer.  One ray
    through the centre of every pixel of the whole film - no jitter, no crop, no random number -, traced once, when the object is made;
    every `render(emit_pos)` then shades those hits with a Blinn-Phong highlight under ONE point light at `emit_pos`, dimmed to a tenth
    where the light is occluded.  Nothing accumulates.

        bpt = BlinnPhongTracer(emitter, array_info, objects, prop)     # a point source: its intensity is used, its position is not
        bpt.render(emitter.pos)
        bpt.pixels.to_numpy()          # (w, h, 3): the frame of the last position shaded
        bpt.depth_map.to_numpy()       # (w, h): hit distance, 0 for a miss;   bpt.norm_map.to_numpy(): (w, h, 3), the shading normal
        bpt.render_sweep(positions)    # (F, w, h, 3): F positions in one launch, the hits read once

    `Renderer.direct()` is something else: the path-length split's direct light."""

    def __init__(self, emitter, array_info: dict, objects: List, prop: dict, *, device: int = 0, exact: Optional[bool] = None, profile: bool = False):
        if isinstance(emitter, (list, tuple)) or getattr(emitter, "type", None) != "point":
            what = f"{len(emitter)} emitters" if isinstance(emitter, (list, tuple)) else f"a '{getattr(emitter, 'type', type(emitter).__name__)}' emitter"
            raise ValueError(f"BlinnPhongTracer: this tracer only supports one point source (renderer/direct_render.py:30), got {what}")
        self.emit_int = np.float32(emitter.intensity).reshape(3)
        super().__init__([emitter], array_info, unlit_objects(objects), prop, device=device, exact=exact, profile=profile, aov_spp=0)
        # what TracerBase fixes whatever the sensor says (tracer_base.py:60-61); the loop of direct_render.py:64 has no crop test
        self.anti_alias = self.stratified_sample = False
        self.depth_map = _MapView(lambda: self._maps()[0])
        self.norm_map = _MapView(lambda: self._maps()[1])

    def _configure(self, cfg, prop: dict):
        cfg.direct = 1
        cfg.direct_intensity = (C.c_float * 3)(*self.emit_int.tolist())
        cfg.anti_alias = cfg.stratified = cfg.do_crop = 0
        cfg.start_x = cfg.start_y = 0
        cfg.end_x, cfg.end_y = cfg.width, cfg.height

    def _maps(self):
        depth, normal = np.empty((self.w, self.h), np.float32), np.empty((self.w, self.h, 3), np.float32)
        _lib.check(self.lib.apt_read_direct_maps(self.handle, _fp(depth), _fp(normal)), "apt_read_direct_maps", self.lib)
        return depth, normal

    def render(self, emit_pos):
        """Shade the film for a light at `emit_pos`; `pixels` holds the frame afterwards (direct_render.py:63-88)"""
        p = light_positions(emit_pos)
        if p.shape[0] != 1:
            raise ValueError("BlinnPhongTracer.render takes one light position; render_sweep takes several")
        _lib.check(self.lib.apt_render_direct(self.handle, _fp(p), 1, None), "apt_render_direct", self.lib)

    def render_sweep(self, positions, out: Optional[np.ndarray] = None) -> np.ndarray:
        """(F, w, h, 3) float32: the frames of F light positions, shaded in one launch (or a few, where the frame buffer sets a chunk);
        `pixels` holds the last one afterwards.  out: a C-contiguous float32 array of that shape to fill instead of a new one"""
        p = light_positions(positions)
        shape = (p.shape[0], self.w, self.h, 3)
        if out is None:
            out = np.empty(shape, np.float32)
        elif out.shape != shape or out.dtype != np.float32 or not out.flags["C_CONTIGUOUS"]:
            raise ValueError(f"render_sweep: out must be a C-contiguous float32 array of shape {shape}")
        _lib.check(self.lib.apt_render_direct(self.handle, _fp(p), p.shape[0], _fp(out)), "apt_render_direct", self.lib)
        return out

    def reset(self):
        """An empty kernel upstream (tracer_base.py:284-286): nothing to do"""

    clear = reset

    def get_check_point(self):
        raise NotImplementedError("Checkpoint saver is not implemented in TracerBase.")       # (tracer_base.py:104-106)

    def load_check_point(self, check_point: dict):
        raise NotImplementedError("BlinnPhongTracer keeps nothing a checkpoint could restore")

    def info(self) -> dict:
        return {**super().info(), "pipeline": "direct", "intensity": self.emit_int.tolist()}

    def summary(self) -> str:
        self.synchronize()
        msg = f"Blinn-Phong viewer, {self.w} x {self.h}. Time since creation: {time.time() - self._t0:.3f} s"
        print(msg)
        return msg


class VolumeRenderer(Renderer):
    """Drop-in for the reference's `VolumeRenderer` (renderer/vpt.py:29-50,145-262; `--type vpt`, the reference's default): same
    constructor and surface as `Renderer`, volumetric path tracing in homogeneous media (world medium, media attached to BSDF
    objects, null surfaces, transmittance-tracked light samples) and in one grid volume (`<volume>`, adapt_amd/volumes.py)."""
    VOLUMETRIC = True
