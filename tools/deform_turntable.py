#!/usr/bin/env python3
"""A mesh that deforms while the camera orbits it, from ONE upload (include/rt_hip_update.h, include/rt_hip_views.h): the mesh is
twisted about the y axis a little more at each of `--steps` steps -- host.update_vertices refits the uploaded scene on the device,
nothing is uploaded again --, and every step is drawn from `--views` poses by one render_views call: one PGM per step and
view, <prefix>_s000_v000.pgm ..., in the format `render` writes.

    python3 tools/deform_turntable.py mesh.off out/bunny [-w 800 -h 600 -s 4 -a 3] [--steps 12] [--views 1] [--twist 1.5]
                                      [--radius 2 --elevation 0.4] [--look-at x,y,z] [--rebuild N]

The shading normals follow the deformation: Scene.refit recomputes them on the CPU for every step (the device keeps the
uploaded ones when an update gives none).  The tree keeps its shape, so a strong twist is walked less well than a fresh
upload of the twisted mesh would be; the images are the same.  `--rebuild N` repairs that on the device: at every N-th step
host.build_scene (include/rt_hip_build.h) makes the scene again from the step's own positions, tree included, instead of
refitting the old one -- still nothing is uploaded, and the images are the same again.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import opencl_raytracer_amd as rt  # noqa: E402
from tools.render_layers import triple  # noqa: E402
from tools.turntable import orbit  # noqa: E402


def twisted(v: np.ndarray, radians_per_unit: float) -> np.ndarray:
    """The (V, 4) float32 positions turned about the y axis by an angle that grows with height."""
    angle = np.float32(radians_per_unit) * v[:, 1]
    c, s = np.cos(angle).astype(np.float32), np.sin(angle).astype(np.float32)
    out = v.copy()
    out[:, 0] = v[:, 0] * c - v[:, 2] * s
    out[:, 2] = v[:, 0] * s + v[:, 2] * c
    return out


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
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--views", type=int, default=1)
    ap.add_argument("--twist", type=float, default=1.5, help="radians per unit of height at the last step")
    ap.add_argument("--radius", type=float, default=2.0)
    ap.add_argument("--elevation", type=float, default=0.4)
    ap.add_argument("--look-at", type=triple, default=(0.0, 0.0, 0.0))
    ap.add_argument("--rebuild", type=int, default=0, help="build the scene again on the device at every N-th step (0: refit only)")
    args = ap.parse_args(argv)
    if args.steps < 1 or args.views < 1 or args.rebuild < 0:
        ap.error("--steps and --views must be at least 1, --rebuild not negative")
    ao = args.ambient_occlusion_samples
    method = 0 if args.bvh_strategy == "longest" else 1
    opt = rt.Options.defaults(width=args.width, height=args.height, n_super_samples=args.supersamples, ao_num_samples=ao,
                              enable_ao=int(ao > 0), bvh_method=method)
    scene = rt.Scene.load_off(args.mesh).build_bvh(method)
    original = scene.vertices
    host = rt.Host(opt, args.device)
    host.upload_scene(scene)  # the one upload
    cameras = orbit(args.views, args.radius, args.elevation, args.look_at)
    os.makedirs(os.path.dirname(os.path.abspath(args.prefix)), exist_ok=True)
    update_ms = views_ms = build_ms = 0.0
    builds = 0
    faces = scene.faces.reshape(-1, 3).copy()
    for step in range(args.steps):
        scene.refit(twisted(original, args.twist * step / max(args.steps - 1, 1)))  # positions, normals and boxes on the CPU
        if args.rebuild and step and step % args.rebuild == 0:
            host.build_scene(scene.vertices, faces, scene.vnormals)                 # ... a new tree around them, on the device
            build_ms += host.last_build_ms
            builds += 1
        else:
            host.update_vertices(scene.vertices, scene.vnormals)                    # ... and the scene on the device
            update_ms += host.last_update_ms
        images = host.render_views(cameras, ("image",))["image"]
        views_ms += host.last_query_ms
        for v in range(args.views):
            with open(f"{args.prefix}_s{step:03d}_v{v:03d}.pgm", "wb") as f:
                f.write(rt.pgm_bytes(images[v]))
    host.close()
    print(f"{args.steps} steps x {args.views} views of {args.width}x{args.height} from one upload: {update_ms / max(args.steps - builds, 1):.3f} ms per update, "
          + (f"{build_ms / builds:.3f} ms per build ({builds} of them), " if builds else "") +
          f"{views_ms / args.steps:.3f} ms per step's views on the device; wrote {args.prefix}_s000_v000.pgm ... "
          f"{args.prefix}_s{args.steps - 1:03d}_v{args.views - 1:03d}.pgm")


if __name__ == "__main__":
    main()
