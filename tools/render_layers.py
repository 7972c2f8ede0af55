#!/usr/bin/env python3
"""Render the layers behind a frame (include/rt_hip_layers.h) of a mesh and write them out: every chosen layer as
<prefix>_<layer>.npy, and depth and normal as viewable 8-bit images, <prefix>_depth.pgm and <prefix>_normal.ppm.

    python3 tools/render_layers.py mesh.off out/bunny [-w 800 -h 600 -s 4 -a 3] [--eye x,y,z --look-at x,y,z --up x,y,z]
                                   [--layers hit,distance,normal,...]

Depth: the hit sub-pixels' distances mapped linearly to 255 (nearest) .. 1 (farthest), 0 where nothing is hit.  Normal:
(n + 1) / 2 per component, black where nothing is hit.  Both at the frame's sub-pixel resolution: ids and depths do not
average, so nothing is box-filtered here.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import opencl_raytracer_amd as rt  # noqa: E402


def triple(text):
    parts = text.split(",")
    if len(parts) != 3:
        raise argparse.ArgumentTypeError(f"expected x,y,z, got {text!r}")
    return tuple(float(p) for p in parts)


def depth_image(hit, distance) -> np.ndarray:
    """uint8 (H, W): 255 nearest .. 1 farthest over the finite hit distances, 0 where nothing is hit."""
    out = np.zeros(hit.shape, np.uint8)
    seen = hit.astype(bool) & np.isfinite(distance)
    if seen.any():
        d = distance[seen].astype(np.float64)
        span = d.max() - d.min()
        out[seen] = np.round(255.0 - 254.0 * ((d - d.min()) / span if span > 0 else 0.0)).astype(np.uint8)
    return out


def normal_image(hit, normal) -> np.ndarray:
    """uint8 (H, W, 3): (n + 1) / 2, black where nothing is hit (or the normal is not a number)."""
    n = np.nan_to_num(normal.astype(np.float64), nan=-1.0, posinf=1.0, neginf=-1.0)
    out = np.round(np.clip((n + 1.0) * 0.5, 0.0, 1.0) * 255.0).astype(np.uint8)
    out[~hit.astype(bool)] = 0
    return out


def pnm_bytes(image: np.ndarray) -> bytes:
    magic = b"P5" if image.ndim == 2 else b"P6"
    return magic + b"\n%d %d\n255\n" % (image.shape[1], image.shape[0]) + np.ascontiguousarray(image, np.uint8).tobytes()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], add_help=False)
    ap.add_argument("--help", action="help")
    ap.add_argument("mesh")
    ap.add_argument("prefix")
    ap.add_argument("-w", "--width", type=int, default=800)
    ap.add_argument("-h", "--height", type=int, default=600)
    ap.add_argument("-s", "--supersamples", type=int, default=1)
    ap.add_argument("-a", "--ambient-occlusion-samples", type=int, default=3)
    ap.add_argument("--bvh-strategy", choices=("longest", "sah"), default="longest")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--eye", type=triple)
    ap.add_argument("--look-at", type=triple, default=(0.0, 0.0, 0.0))
    ap.add_argument("--up", type=triple, default=(0.0, 1.0, 0.0))
    ap.add_argument("--layers", default=None, help="comma-separated; default: all the host has")
    args = ap.parse_args(argv)
    ao = args.ambient_occlusion_samples
    available = tuple(n for n in rt.LAYER_OUTPUTS if ao > 0 or n != "ao")
    names = available if args.layers is None else tuple(args.layers.split(","))
    unknown = [n for n in names if n not in available]
    if unknown:
        ap.error(f"unknown or unavailable layers {unknown}; choose from {available}")
    method = 0 if args.bvh_strategy == "longest" else 1
    opt = rt.Options.defaults(width=args.width, height=args.height, n_super_samples=args.supersamples, ao_num_samples=ao,
                              enable_ao=int(ao > 0), bvh_method=method)
    scene = rt.Scene.load_off(args.mesh).build_bvh(method)
    host = rt.Host(opt, args.device)
    if args.eye is not None:
        host.set_camera(rt.Camera.look_at(args.eye, args.look_at, args.up))
    host.upload_scene(scene)
    wanted = tuple(dict.fromkeys(names + ("hit", "distance", "normal")))
    layers = host.render_layers(wanted)
    ms = host.last_query_ms
    host.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.prefix)), exist_ok=True)
    for name in names:
        np.save(f"{args.prefix}_{name}.npy", layers[name])
    with open(f"{args.prefix}_depth.pgm", "wb") as f:
        f.write(pnm_bytes(depth_image(layers["hit"], layers["distance"])))
    with open(f"{args.prefix}_normal.ppm", "wb") as f:
        f.write(pnm_bytes(normal_image(layers["hit"], layers["normal"])))
    print(f"{opt.total_width}x{opt.total_height} sub-pixels, {int(layers['hit'].sum())} hit, {ms:.3f} ms on the device; wrote "
          f"{', '.join(names)} as .npy, {args.prefix}_depth.pgm, {args.prefix}_normal.ppm")


if __name__ == "__main__":
    main()
