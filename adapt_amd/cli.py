"""`render.py`-compatible command line for the `pt` and `vpt` renderers on MI355X.

Mirrors the reference driver's flags and control flow for `--type pt|vpt --no_gui`
(`render.py:65-166`, `parsers/opts.py:15-44`): scene parsing, optional checkpoint load,
`iter_num + 1` samples (the reference's `--no_gui` loop runs `range(iter_num + 1)`,
render.py:80-81,118), periodic checkpoint saves, summary, optional quantile normalisation
(`utils/watermark.py:28-29`), image file `<output_path><img_name>-<scene file stem>-pt.<ext>`.
A cropped render writes the crop window `[start_x:end_x, start_y:end_y]` of the (w, h, 3) image; the reference slices
`[start_y:end_y, start_x:end_x]` on that same (w, h, 3) array (`utils/watermark.py:25`), which is the intended window only for
square crops - a deliberate deviation.
Differences: there is no GUI and no Taichi (`--arch` is accepted and ignored unless it is not
one of the known names), only `--type pt` and `--type vpt` exist (homogeneous media), the "RENDERED WITH AdaPT" watermark is not
stamped (`--no_watermark` is accepted), PNG/BMP are written by a small built-in encoder.
`--transient` (with `--type pt`): time-resolved rendering with the sensor's `sample_count` / `min_time` / `interval`; the frames are
written as upstream's `export_transient_profile` writes them (render.py:36-56,166): `<output_path>/<scene file stem>/img_001.<ext>` ...,
`--normalize` applied as one quantile over the whole cube, and the cube itself as `transient.npy` (n_bins, w, h, 3) next to them.
`--noise_threshold t` (with `--min_spp`, `--adaptive_step`): adaptive sampling; `--iter_num` is then the most samples
any pixel gets, and the per-pixel sample counts are written as `<img_name>-<scene file stem>-<type>-spp.npy` (w, h) int32 next to the
image (cropped like it).  Not with `--transient`.
`--path_lengths` (with `--type pt`): the render split by path length: one image per length - segments, camera to
emitter; 1 emission, 2 direct light, 3 and more indirect - as `<img_name>-<scene file stem>-pt-len01.<ext>` ..., both parts summed, cropped
and normalised like the image, and the (lengths, 2, w, h, 3) array as `...-pt-lengths.npy`.  Not with `--transient` or `--noise_threshold`.
`--light_groups` (with `--type pt`): the render split by emitter: one image per emitter of the scene file, in its order, as
`<img_name>-<scene file stem>-pt-light00.<ext>` ..., both parts summed, cropped and normalised like the image, and the (emitters, 2, w, h, 3)
array as `...-pt-lights.npy`.  `--light_gain id=g` or `id=r,g,b` (repeatable; `id` is the emitter's XML id, the others keep gain 1) also writes
the image relit with those gains as `...-pt-relit.<ext>`.  Not with `--transient`, `--path_lengths` or `--noise_threshold`.
`--denoise` (with `--type pt`; `--firefly_threshold t`, `--save_aov`): the frame through the firefly filter (t > 0) and the edge-avoiding
a-trous filter, written as `<img_name>-<scene file stem>-<type>-denoised.<ext>` next to the image (cropped and normalised
like it); `--save_aov` writes the feature buffers the filter was guided by as `...-<type>-aov.npz` (albedo, normal, depth, hit_fraction).
"""
from __future__ import annotations

import argparse
import os
import pickle
import struct
import sys
import time
import zlib

import numpy as np

__all__ = ["get_options", "main", "write_image", "to_display"]


def get_options(argv=None):
    p = argparse.ArgumentParser(description="AdaPT-compatible path tracing driver (HIP / MI355X)", fromfile_prefix_chars="@")
    p.add_argument("--config", default=None, help="file with one `key = value` (or `--key value`) per line")
    p.add_argument("--iter_num", default=-1, type=int, help="Number of iterations (-1: the scene's iter_num or 2000)")
    p.add_argument("--normalize", default=0., type=float, help="Normalize the output picture with its <x> quantile value")
    p.add_argument("--output_freq", default=0, type=int)
    p.add_argument("--input_path", default="./scenes/", type=str)
    p.add_argument("--output_path", default="./outputs/", type=str)
    p.add_argument("--chkpt_path", default="./checkpoint/", type=str)
    p.add_argument("--img_name", default="pbr", type=str)
    p.add_argument("--img_ext", default="png", choices=["png", "jpg", "bmp", "npy"])      # parsers/opts.py:25 (jpg through Pillow)
    p.add_argument("--scene", default="cbox", type=str)
    p.add_argument("--name", default="c2_cbox.xml", type=str)
    p.add_argument("--arch", default="hip", choices=["hip", "cpu", "gpu", "vulkan", "cuda"], help="kept for CLI compatibility; rendering always uses HIP")
    p.add_argument("--save_iter", default=-1, type=int)
    p.add_argument("--type", default="pt", choices=["pt", "vpt", "bdpt", "ao"])
    p.add_argument("-p", "--profile", default=False, action="store_true")
    p.add_argument("--no_gui", default=False, action="store_true")
    p.add_argument("-d", "--debug", default=False, action="store_true")
    p.add_argument("-a", "--analyze", default=False, action="store_true")
    p.add_argument("-l", "--load", default=False, action="store_true")
    p.add_argument("--no_cache", default=False, action="store_true")
    p.add_argument("--no_save_fig", default=False, action="store_true")
    p.add_argument("--no_watermark", default=False, action="store_true")
    # extensions
    p.add_argument("--device", default=0, type=int)
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--width", default=None, type=int)
    p.add_argument("--height", default=None, type=int)
    p.add_argument("--max_bounce", default=None, type=int)
    p.add_argument("--spp_per_batch", default=0, type=int, help="samples per wavefront batch (0: automatic)")
    p.add_argument("--transient", default=False, action="store_true", help="time-resolved output (pt only; the sensor's sample_count / min_time / interval)")
    p.add_argument("--path_lengths", default=False, action="store_true", help="also write one image per path length (pt only): ...-len01.<ext> (emission), -len02 (direct), ... and ...-lengths.npy")
    p.add_argument("--light_groups", default=False, action="store_true", help="also write one image per emitter (pt only): ...-light00.<ext>, -light01, ... and ...-lights.npy")
    p.add_argument("--light_gain", default=[], action="append", metavar="ID=G", help="with --light_groups: also write ...-relit.<ext>, the image with emitter ID's share times G (one number, or r,g,b); repeatable")
    p.add_argument("--noise_threshold", default=0., type=float, help="adaptive sampling: a pixel stops once the relative standard error of its mean is <= this (0: off)")
    p.add_argument("--min_spp", default=64, type=int, help="adaptive sampling: no pixel stops before this many samples")
    p.add_argument("--adaptive_step", default=32, type=int, help="adaptive sampling: pixels are retired at sample numbers that are multiples of this")
    p.add_argument("--denoise", default=False, action="store_true", help="also write the frame through the edge-avoiding denoiser (pt only), as ...-denoised.<ext>")
    p.add_argument("--firefly_threshold", default=0., type=float, help="--denoise: run the firefly filter first, with this rgb distance threshold (0: off; upstream's value is 0.4)")
    p.add_argument("--save_aov", default=False, action="store_true", help="--denoise: also write the feature buffers (albedo, normal, depth, hit_fraction) as ...-aov.npz")
    argv = list(sys.argv[1:] if argv is None else argv)
    pre, _ = p.parse_known_args(argv)
    if pre.config:
        extra = []
        for line in open(pre.config):
            line = line.split("#")[0].strip()
            if not line:
                continue
            key, _, val = line.partition("=")
            key, val = key.strip().lstrip("-"), val.strip()
            if val.lower() in ("false", "0", "no", "off") and any(a.dest == key and a.nargs == 0 for a in p._actions):
                continue                    # a switch set to false: leave it off (configargparse accepts `no_gui = false`)
            extra += [f"--{key}"] + ([val] if val and val.lower() not in ("true",) else [])
        argv = extra + argv           # command line wins over the file
    return p.parse_args(argv)


def to_display(img: np.ndarray) -> np.ndarray:
    """(w, h, 3) [x][y], y up  ->  (rows, cols, 3) uint8, row 0 on top (what ti.tools.imwrite stores)."""
    a = np.clip(np.nan_to_num(img, nan=0.0, posinf=1.0, neginf=0.0), 0.0, 1.0)
    a = np.ascontiguousarray(np.swapaxes(a, 0, 1)[::-1])
    return (a * 255.0 + 0.5).astype(np.uint8)


def write_image(img: np.ndarray, path: str):
    ext = path.rsplit(".", 1)[-1].lower()
    if ext == "npy":
        np.save(path, img)
        return
    px = to_display(img)
    h, w, _ = px.shape
    if ext in ("jpg", "jpeg"):
        from .parsers.image_io import write_jpeg
        write_jpeg(path, px)
        return
    if ext == "png":
        def chunk(tag, data):
            return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
        raw = b"".join(b"\x00" + px[r].tobytes() for r in range(h))
        blob = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b"")
    else:   # bmp, bottom-up BGR rows padded to 4 bytes
        row = (3 * w + 3) & ~3
        body = b"".join(px[r, :, ::-1].tobytes() + b"\x00" * (row - 3 * w) for r in range(h - 1, -1, -1))
        blob = b"BM" + struct.pack("<IHHI", 54 + len(body), 0, 0, 54) + struct.pack("<IiiHHIIiiII", 40, w, h, 1, 24, 0, len(body), 2835, 2835, 0, 0) + body
    with open(path, "wb") as f:
        f.write(blob)


def export_transient(rdr, out_path: str, out_name: str, out_ext: str, normalize: float = 0.) -> str:
    """render.py:36-56 export_transient_profile: one image per time bin, img_001.<ext> ..., normalised by ONE quantile of the whole
    cube when normalize > 0.9; the cube (n_bins, w, h, 3) is also saved as transient.npy.  Returns the folder."""
    folder = _folder(os.path.join(out_path, out_name))
    cube = rdr.transient()
    np.save(os.path.join(folder, "transient.npy"), cube)
    frames = cube[:, rdr.start_x:rdr.end_x, rdr.start_y:rdr.end_y, :] if rdr.do_crop else cube
    if normalize > 0.9:
        frames = frames / np.quantile(frames, normalize)
    for i in range(frames.shape[0]):
        write_image(frames[i], os.path.join(folder, f"img_{i + 1:03d}.{out_ext}"))
    print(f"[adapt_amd] wrote {frames.shape[0]} transient frames and transient.npy to {folder}")
    return folder


def _folder(path: str) -> str:
    os.makedirs(path, exist_ok=True)
    return path


def write_planes(planes: np.ndarray, shown, base: str, cube: str, frame: str, first: int, ext: str) -> int:
    """A split render's planes (n, 2, w, h, 3): the whole array as <base>-<cube>.npy, and one image per leading index - its two parts
    summed, through `shown` - as <base>-<frame>NN.<ext>, NN counting from `first`.  Returns n."""
    np.save(f"{base}-{cube}.npy", planes)
    frames = shown(planes.sum(1))
    for i in range(frames.shape[0]):
        write_image(frames[i], f"{base}-{frame}{i + first:02d}.{ext}")
    return frames.shape[0]


# The split renders' switches in the order their refusals are tried: option, what it writes (with its verb), its axis in a combined split.
SPLIT_OPTIONS = (("transient", "time-resolved output", "exists", "time"),
                 ("path_lengths", "path-length images", "exist", "length"),
                 ("light_groups", "light groups", "exist", "emitter"))


def split_refusal(opts) -> str:
    """Why this combination of split switches is not rendered, or "": each is `pt` only, no two combine, and (--transient says so
    itself, where the adaptive options are read) none combines with adaptive sampling."""
    for k, (opt, noun, verb, axis) in enumerate(SPLIT_OPTIONS):
        if not getattr(opts, opt):
            continue
        if opts.type != "pt":
            return f"--{opt}: {noun} {verb} for the surface renderer only (--type pt), not for --type {opts.type}"
        for other, _, _, other_axis in SPLIT_OPTIONS[:k]:
            if getattr(opts, other):
                return (f"--{opt} with --{other}: {other_axis} x {axis} {'cubes' if other == 'transient' else 'planes'} are not built; "
                        f"{noun} and --{other} do not combine")
        if opt != "transient" and opts.noise_threshold > 0:
            return f"--{opt} with --noise_threshold: {noun} need every pixel's samples; adaptive sampling and --{opt} do not combine"
    return ""


def parse_light_gains(items) -> dict:
    """["id=g", "id=r,g,b", ...] -> {id: g or (r, g, b)}; ValueError names the item it cannot read."""
    gains = {}
    for item in items:
        key, sep, val = item.partition("=")
        try:
            nums = [float(v) for v in val.split(",")]
        except ValueError:
            nums = []
        if not sep or not key or len(nums) not in (1, 3) or not all(np.isfinite(nums)):
            raise ValueError(f"{item!r} is not id=g or id=r,g,b with finite numbers")
        gains[key] = nums[0] if len(nums) == 1 else tuple(nums)
    return gains


def main(argv=None) -> int:
    opts = get_options(argv)
    if opts.type not in ("pt", "vpt"):
        print(f"--type {opts.type}: only the `pt` and `vpt` renderers exist in this build (bdpt/ao are outside its scope)", file=sys.stderr)
        return 2
    refusal = split_refusal(opts)
    if refusal:
        print(refusal, file=sys.stderr)
        return 2
    if opts.light_gain and not opts.light_groups:
        print("--light_gain: relighting needs the per-emitter planes; give --light_groups as well", file=sys.stderr)
        return 2
    try:
        light_gains = parse_light_gains(opts.light_gain)
    except ValueError as e:
        print(f"--light_gain: {e}", file=sys.stderr)
        return 2
    if (opts.denoise or opts.save_aov) and opts.type != "pt":
        print(f"--denoise / --save_aov: feature buffers and the denoiser exist for the surface renderer only (--type pt), not for --type {opts.type}", file=sys.stderr)
        return 2
    if opts.firefly_threshold < 0:
        print("--firefly_threshold must be >= 0 (0: no firefly filter)", file=sys.stderr)
        return 2
    adaptive = None
    if opts.noise_threshold > 0:
        if opts.transient:
            print("--transient with --noise_threshold: time-resolved output needs every pixel's samples; adaptive sampling and --transient do not combine", file=sys.stderr)
            return 2
        if opts.min_spp <= 0 or opts.adaptive_step <= 0:
            print("--min_spp and --adaptive_step must be > 0", file=sys.stderr)
            return 2
        adaptive = {"threshold": opts.noise_threshold, "min_spp": opts.min_spp, "step": opts.adaptive_step}
    elif opts.noise_threshold < 0:
        print("--noise_threshold must be >= 0 (0: every pixel takes every sample)", file=sys.stderr)
        return 2
    from .parsers.xml_parser import scene_parsing
    from .renderer import Renderer, VolumeRenderer
    if opts.type == "vpt":                      # render.py:33 rdr_mapping: "vpt" -> VolumeRenderer
        Renderer = VolumeRenderer
    t0 = time.time()
    emitters, array_info, objs, cfg = scene_parsing(os.path.join(opts.input_path, opts.scene), opts.name)
    print(f"[adapt_amd] scene '{opts.scene}/{opts.name}': {array_info['primitives'].shape[0]} primitives, {len(objs)} objects, "
          f"{len(emitters)} emitters, parsed in {time.time() - t0:.3f} s")
    unknown = [k for k in light_gains if k not in [e.id for e in emitters]]
    if unknown:
        print(f"--light_gain: no emitter with id {unknown[0]!r} in {opts.name}; it has {[e.id for e in emitters]}", file=sys.stderr)
        return 2
    rdr = Renderer(emitters, array_info, objs, cfg, device=opts.device, seed=opts.seed, profile=opts.profile,
                   width=opts.width, height=opts.height, max_bounce=opts.max_bounce, spp_per_batch=opts.spp_per_batch,
                   transient=True if opts.transient else None, adaptive=adaptive, path_lengths=opts.path_lengths, light_groups=opts.light_groups)
    stem = opts.name[:-4]
    max_iter = (opts.iter_num if opts.iter_num > 0 else cfg.get("iter_num", 2000)) + 1          # render.py:80-81
    chk_file = os.path.join(_folder(opts.chkpt_path), f"{opts.img_name}-{stem}-{opts.type}.pkl")
    if opts.load:
        with open(chk_file, "rb") as f:
            rdr.load_check_point(pickle.load(f))
        print(f"[adapt_amd] recovered from check-point, elapsed counter: {rdr.cnt[None]}")
    print(f"[adapt_amd] path tracing with {rdr.max_bounce} bounce(s), {rdr.w}x{rdr.h}, {max_iter} samples, {rdr.info()}")

    def save_chk():
        with open(chk_file, "wb") as f:
            pickle.dump(rdr.get_check_point(), f, protocol=pickle.HIGHEST_PROTOCOL)

    done = 0
    t1 = time.time()
    try:
        while done < max_iter:
            step = max_iter - done
            if opts.save_iter > 0:
                # the reference saves before iteration i whenever i % save_iter == 0 (render.py:119-121)
                if done % opts.save_iter == 0:
                    save_chk()
                step = min(step, opts.save_iter - done % opts.save_iter)
            rdr.render(n_spp=step)
            done += step
            if opts.output_freq > 0 and done % opts.output_freq == 0 and done < max_iter:
                out_dir = _folder(os.path.join(opts.output_path, f"{opts.img_name}-{stem}-{opts.type}"))
                write_image(rdr.pixels.to_numpy(), os.path.join(out_dir, f"img_{done:05d}.{opts.img_ext}"))
        rdr.synchronize()
    except KeyboardInterrupt:
        if opts.save_iter > 0:
            save_chk()
        print("[adapt_amd] quit on keyboard interruption")
    dt = time.time() - t1
    rdr.summary()
    n = rdr.w * rdr.h * done
    spp_map = None
    if adaptive:
        spp_map = rdr.sample_counts()
        if rdr.do_crop:
            spp_map = spp_map[rdr.start_x:rdr.end_x, rdr.start_y:rdr.end_y]
        n = int(rdr.stats()["n_samples"])
        print(f"[adapt_amd] adaptive sampling: {100.0 * (1.0 - rdr.active_fraction()):.2f} % of the pixels converged, "
              f"mean spp {spp_map.mean():.1f} (at most {done})")
    print(f"[adapt_amd] {n / max(dt, 1e-9) / 1e6:.1f} Msamples/s ({done} spp in {dt:.3f} s)")
    if opts.profile:
        st = rdr.stats()
        for k, ms in st["kernel_ms"].items():
            print(f"[adapt_amd]   {k:9s} {st['launches'][k]:6d} launches {ms:10.3f} ms")
    img = rdr.pixels.to_numpy()
    if rdr.do_crop:
        img = img[rdr.start_x:rdr.end_x, rdr.start_y:rdr.end_y, :]
    print(f"[adapt_amd] pixel max value = {np.nanmax(img):.3f}")
    scale = np.quantile(img, opts.normalize) if opts.normalize > 0.9 else None
    if scale is not None:
        img = img / scale
    if not opts.no_save_fig:
        out = os.path.join(_folder(opts.output_path), f"{opts.img_name}-{stem}-{opts.type}.{opts.img_ext}")
        write_image(img, out)
        print(f"[adapt_amd] wrote {out}")
        if spp_map is not None:
            out_spp = os.path.join(opts.output_path, f"{opts.img_name}-{stem}-{opts.type}-spp.npy")
            np.save(out_spp, spp_map)
            print(f"[adapt_amd] wrote {out_spp}")
    if (opts.denoise or opts.save_aov) and not opts.no_save_fig:
        base = os.path.join(opts.output_path, f"{opts.img_name}-{stem}-{opts.type}")

        def window(a):
            return a[rdr.start_x:rdr.end_x, rdr.start_y:rdr.end_y] if rdr.do_crop else a
        if opts.denoise:
            den = window(rdr.denoised(firefly_threshold=opts.firefly_threshold))
            if opts.normalize > 0.9:
                den = den / np.quantile(den, opts.normalize)
            write_image(den, f"{base}-denoised.{opts.img_ext}")
            print(f"[adapt_amd] wrote {base}-denoised.{opts.img_ext}")
        if opts.save_aov:
            np.savez(f"{base}-aov.npz", **{k: window(v) for k, v in rdr.aov().items()})
            print(f"[adapt_amd] wrote {base}-aov.npz")
    if (opts.path_lengths or opts.light_groups) and not opts.no_save_fig:
        base = os.path.join(opts.output_path, f"{opts.img_name}-{stem}-{opts.type}")

        def shown(a):                           # cropped and scaled like the image (its quantile): the written frames still add up to the written image
            a = a[..., rdr.start_x:rdr.end_x, rdr.start_y:rdr.end_y, :] if rdr.do_crop else a
            return a / scale if scale is not None else a
        if opts.path_lengths:
            n = write_planes(rdr.path_lengths(), shown, base, "lengths", "len", 1, opts.img_ext)
            print(f"[adapt_amd] wrote {n} path-length images {base}-len01.{opts.img_ext} ... and {base}-lengths.npy")
        if opts.light_groups:
            n = write_planes(rdr.light_groups(), shown, base, "lights", "light", 0, opts.img_ext)
            print(f"[adapt_amd] wrote {n} light-group images {base}-light00.{opts.img_ext} ... (emitters {rdr.emitter_ids}) and {base}-lights.npy")
            if light_gains:
                write_image(shown(rdr.relit(light_gains)), f"{base}-relit.{opts.img_ext}")
                print(f"[adapt_amd] wrote {base}-relit.{opts.img_ext} (gains {light_gains})")
    if opts.transient:
        export_transient(rdr, opts.output_path, stem, opts.img_ext, opts.normalize)      # render.py:166: folder named after the scene file
    rdr.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
