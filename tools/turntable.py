#!/usr/bin/env python3
"""A turntable of a mesh from ONE upload (include/rt_hip_views.h): `--views` poses on an orbit around the model, rendered
in one render_views call, one PGM per view -- <prefix>_000.pgm ... -- in the format `render` writes.

    python3 tools/turntable.py mesh.off out/bunny [-w 800 -h 600 -s 4 -a 3] [--views 36] [--radius 2 --elevation 0.4]
                               [--look-at x,y,z] [--depth] [--instances grid:N | --instances poses.npy]

The eyes lie on a circle of `--radius` around the y axis through `--look-at`, `--elevation` above it, and look at it; view
0 is the reference's own direction (from +z).  With --depth a depth map per view is written as well, <prefix>_000_depth.pgm
(tools/render_layers.py: depth_image), from the same call.

With --instances the views show posed copies of the mesh (include/rt_hip_instance_views.h, render_instance_views): `grid:N`
places N x N x N copies on a grid 1.5 box widths apart, each turned about its own centre (seeded); a .npy file holds float32
(n, 3, 4), the rows of world_from_object.  --radius and --look-at are then the caller's to choose for the whole set.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import opencl_raytracer_amd as rt  # noqa: E402
from tools.render_layers import depth_image, pnm_bytes, triple  # noqa: E402


def orbit(views: int, radius: float, elevation: float, look_at) -> list:
    cx, cy, cz = look_at
    out = []
    for k in range(views):
        a = 2.0 * np.pi * k / views
        out.append(rt.Camera.look_at((cx + radius * np.sin(a), cy + elevation, cz + radius * np.cos(a)), look_at))
    return out


def instance_poses(spec: str, scene) -> np.ndarray:
    """float32 (n, 3, 4) from `grid:N` or a .npy file."""
    if not spec.startswith("grid:"):
        W = np.load(spec)
        if W.dtype != np.float32 or W.ndim != 3 or W.shape[1:] != (3, 4) or len(W) == 0:
            raise SystemExit(f"{spec}: expected a float32 array of shape (n, 3, 4), n >= 1")
        return np.ascontiguousarray(W)
    per_axis = int(spec[5:])
    if per_axis < 1:
        raise SystemExit("--instances grid:N needs N >= 1")
    rng = np.random.default_rng(1)
    lo, hi = scene.aabbs[0, :3].astype(np.float64), scene.aabbs[1, :3].astype(np.float64)
    centre, step = (lo + hi) / 2, float((hi - lo).max()) * 1.5
    W = []
    for cell in np.ndindex(per_axis, per_axis, per_axis):
        q, r = np.linalg.qr(rng.normal(size=(3, 3)))
        A = q * np.sign(np.diag(r))[None, :]
        if np.linalg.det(A) < 0:
            A[:, 0] = -A[:, 0]
        W.append(np.concatenate([A, (centre - A @ centre + (np.array(cell) - (per_axis - 1) / 2) * step)[:, None]], axis=1))
    return np.ascontiguousarray(np.stack(W), np.float32)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0], add_help=False)
    ap.add_argument("--help", action="help")
    ap.add_argument("mesh")
    ap.add_argument("prefix")
    ap.add_argument("-w", "--width", type=int, default=800)
    ap.add_argument("-h", "--height", type=int, default=600)
    ap.add_argument("-s", "--supersamples", type=int, default=4)
    ap.add_argument("-a", "--ambient-occlusion-samples", type=int, default=3)
    ap.add_argument("--bvh-strategy", choices=("longest", "sah"), default="longest")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--views", type=int, default=36)
    ap.add_argument("--radius", type=float, default=2.0)
    ap.add_argument("--elevation", type=float, default=0.4)
    ap.add_argument("--look-at", type=triple, default=(0.0, 0.0, 0.0))
    ap.add_argument("--depth", action="store_true")
    ap.add_argument("--instances", default=None, metavar="grid:N|FILE.npy")
    args = ap.parse_args(argv)
    if args.views < 1:
        ap.error("--views must be at least 1")
    ao = args.ambient_occlusion_samples
    method = 0 if args.bvh_strategy == "longest" else 1
    opt = rt.Options.defaults(width=args.width, height=args.height, n_super_samples=args.supersamples, ao_num_samples=ao,
                              enable_ao=int(ao > 0), bvh_method=method)
    scene = rt.Scene.load_off(args.mesh).build_bvh(method)
    host = rt.Host(opt, args.device)
    host.upload_scene(scene)
    render = host.render_views
    if args.instances:
        host.set_instances(instance_poses(args.instances, scene))
        render = host.render_instance_views
    got = render(orbit(args.views, args.radius, args.elevation, args.look_at), ("image", "hit", "distance") if args.depth else ("image",))
    ms, done = host.last_query_ms, host.last_views()
    host.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.prefix)), exist_ok=True)
    for v in range(args.views):
        with open(f"{args.prefix}_{v:03d}.pgm", "wb") as f:
            f.write(rt.pgm_bytes(got["image"][v]))
        if args.depth:
            with open(f"{args.prefix}_{v:03d}_depth.pgm", "wb") as f:
                f.write(pnm_bytes(depth_image(got["hit"][v], got["distance"][v])))
    print(f"{args.views} views of {args.width}x{args.height} ({opt.total_width}x{opt.total_height} sub-pixels) from one upload: "
          f"{ms:.3f} ms on the device in {done['chunks']} chunks, {done['ao_points']} points in the ambient-occlusion step; wrote "
          f"{args.prefix}_000.pgm ... {args.prefix}_{args.views - 1:03d}.pgm")


if __name__ == "__main__":
    main()
