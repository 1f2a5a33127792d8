"""The direct-light viewer from the command line (upstream's `python direct_render.py`, without the window):

    python -m adapt_amd.direct_view --scene cbox --name c2_cbox.xml [--emit_pos x,y,z ...] [--width W --height H]

One light position - the scene's first emitter's own, unless --emit_pos says otherwise - writes phong.<ext>, depth.<ext> (depth / its
maximum) and normal.<ext> ((n + 1) / 2), as upstream's script does; several write phong_000.<ext>, phong_001.<ext>, ... from one sweep, and
the two maps once.  The scene's first emitter must be a point source: its intensity is the light's.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np


def parse_position(text: str) -> np.ndarray:
    """`x,y,z` -> float32 (3,); an argparse error for anything else"""
    parts = text.split(",")
    try:
        p = np.float32([float(v) for v in parts])
    except ValueError:
        raise argparse.ArgumentTypeError(f"'{text}' is not x,y,z") from None
    if p.shape != (3,) or not np.isfinite(p).all():
        raise argparse.ArgumentTypeError(f"'{text}' is not three finite numbers x,y,z")
    return p


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="adapt_amd.direct_view", description="Blinn-Phong direct-light viewer on HIP (upstream's renderer/direct_render.py)")
    p.add_argument("--scene", default="cbox", type=str)
    p.add_argument("--name", default="c2_cbox.xml", type=str)
    p.add_argument("--input_path", default="./scenes/", type=str)
    p.add_argument("--output_path", default="./outputs/", type=str)
    p.add_argument("--img_ext", default="png", choices=["png", "jpg", "bmp", "npy"])
    p.add_argument("--width", default=None, type=int)
    p.add_argument("--height", default=None, type=int)
    p.add_argument("--device", default=0, type=int)
    p.add_argument("--exact", default=False, action="store_true", help="the bit-parity build instead of the product build")
    p.add_argument("--emit_pos", default=[], action="append", type=parse_position, metavar="x,y,z",
                   help="a light position; repeatable (default: the first emitter's own position)")
    return p.parse_args(argv)


def output_names(n_positions: int, ext: str) -> list:
    """the frames' file names: phong.<ext> for one position, phong_000.<ext> ... for several"""
    return [f"phong.{ext}"] if n_positions == 1 else [f"phong_{k:03d}.{ext}" for k in range(n_positions)]


def map_images(depth: np.ndarray, normal: np.ndarray):
    """what upstream's script writes (direct_render.py:129-134): depth / its maximum (all zero where nothing was hit) and (n + 1) / 2, both (w, h, 3)"""
    top = float(depth.max()) if depth.size else 0.0
    d = depth / np.float32(top) if top > 0 else np.zeros_like(depth)
    return np.repeat(d[..., None], 3, -1).astype(np.float32), ((normal + np.float32(1.0)) / np.float32(2.0)).astype(np.float32)


def main(argv=None) -> int:
    opts = parse_args(argv)
    from .cli import write_image
    from .parsers import scene_parsing
    from .renderer import BlinnPhongTracer
    emitters, array_info, objs, cfg = scene_parsing(os.path.join(opts.input_path, opts.scene), opts.name)
    if not emitters:
        print("[adapt_amd.direct_view] the scene has no emitter", file=sys.stderr)
        return 2
    if opts.width:
        cfg["film"]["width"] = opts.width
    if opts.height:
        cfg["film"]["height"] = opts.height
    positions = np.stack(opts.emit_pos) if opts.emit_pos else np.float32(emitters[0].pos).reshape(1, 3)
    bpt = BlinnPhongTracer(emitters[0], array_info, objs, cfg, device=opts.device, exact=True if opts.exact else None)
    frames = bpt.render_sweep(positions)
    depth, normal = map_images(bpt.depth_map.to_numpy(), bpt.norm_map.to_numpy())
    bpt.close()
    os.makedirs(opts.output_path, exist_ok=True)
    written = []
    for name, img in list(zip(output_names(len(positions), opts.img_ext), frames)) + [(f"depth.{opts.img_ext}", depth), (f"normal.{opts.img_ext}", normal)]:
        path = os.path.join(opts.output_path, name)
        write_image(img, path)
        written.append(path)
    print(f"[adapt_amd.direct_view] {len(positions)} light position(s), {bpt.w} x {bpt.h}: " + ", ".join(written))
    return 0


if __name__ == "__main__":
    sys.exit(main())
