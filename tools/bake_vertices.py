#!/usr/bin/env python3
"""Per-vertex baking from one upload (include/rt_hip_directional.h): ambient occlusion, bent normals and the visibility
mask of every vertex of a mesh.

    python3 tools/bake_vertices.py MESH.off OUT.npz [--samples 3] [--distance 0.2] [--alpha-min 4] [--alpha-max 90]
                                                    [--random] [--bvh 0|1] [--device 0]

OUT.npz holds, per vertex of the file and in its order:
  ao    float32 (V,)       the reference's ambient-occlusion term, 1 - blocked / n
  bent  float32 (V, 3)     the sum of the directions of the vertex's open rays, in ray order, not normalised
  mask  uint32  (V, W)     bit k & 31 of word k >> 5: ray k was blocked (opencl_raytracer_amd.unpack_ao_mask)
  rays  float32 (V, R, 4)  the directions of the vertex's rays as cast (.w 0): what the bits of `mask` stand for
A vertex no face uses has a zero normal: its rays are not numbers, none is blocked, its `bent` is not a number.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import opencl_raytracer_amd as rt  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mesh")
    ap.add_argument("out")
    ap.add_argument("--samples", type=int, default=3, help="ao_num_samples: rings of the direction table, or samples with --random")
    ap.add_argument("--distance", type=float, default=0.2, help="ao_max_distance")
    ap.add_argument("--alpha-min", type=int, default=4)
    ap.add_argument("--alpha-max", type=int, default=90)
    ap.add_argument("--random", action="store_true", help="the RANDOM method (seeded by the vertex index)")
    ap.add_argument("--bvh", type=int, default=0, choices=(0, 1))
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.samples < 1:
        ap.error("--samples must be at least 1")
    scene = rt.Scene.load_off(args.mesh).build_bvh(args.bvh)
    opt = rt.Options.defaults(width=64, height=64, ao_num_samples=args.samples, ao_max_distance=args.distance,
                              ao_alpha_min=args.alpha_min, ao_alpha_max=args.alpha_max, ao_method=int(args.random), bvh_method=args.bvh)
    host = rt.Host(opt, args.device)
    host.upload_scene(scene)
    points, normals = scene.vertices, scene.vnormals
    baked = host.directional_occlusion(points, normals, outputs=("ao", "mask", "bent"))
    rays = host.ao_rays(points, normals)["directions"]
    per_point, _ = host.ao_rays_per_point
    host.close()
    np.savez(args.out, ao=baked["ao"], bent=baked["bent"], mask=baked["mask"], rays=rays)
    blocked = int(rt.unpack_ao_mask(baked["mask"], per_point).sum())
    print(f"{args.out}: {len(points)} vertices, {per_point} rays each, {blocked} of {len(points) * per_point} blocked, "
          f"mean ao {float(np.nanmean(baked['ao'])):.4f}")


if __name__ == "__main__":
    main()
