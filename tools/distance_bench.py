#!/usr/bin/env python3
"""Closest-point query throughput on the bunny (include/rt_hip_nearest.h): one JSON line per (set, form), appended to
profiles/distance_bench.jsonl.

Sets:   (a) the bunny's vertices pushed 1e-3 along their normals
        (b) --points points uniform in the root box
        (c) --points points in a shell two box sizes out
Forms:  sorted; unsorted; sorted without the starting bound; sorted without pruning (on --noprune-points of the set, --noprune-reps
        calls: every point then tests every leaf)
The two switches and the counters are the A/B build's (opencl_raytracer_amd/lib_knobs, rt_debug_set_nearest_walk): this tool
loads that build.  Device entry points on pre-loaded buffers; the time of a call is rt_last_query_ms (HIP events around sort +
walk), the median of --reps calls after --warmup; box tests and triangle tests per point come from one more, counted call.

    python3 tools/distance_bench.py [--reps 20] [--warmup 3] [--points 1048576] [--sets abc]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
os.environ.setdefault("OCRT_LIB_DIR", "lib_knobs")  # the build that has the switches

import opencl_raytracer_amd as rt  # noqa: E402
from opencl_raytracer_amd.api import RT_QUERY_NO_SORT, _HitArrays  # noqa: E402
from tools.meshes import bunny_path  # noqa: E402

FIELDS = ("hit", "distance", "leaf", "barycentric", "position", "normal")


def main():
    import torch

    torch.zeros(1, device="cuda:0")  # torch's HIP runtime up BEFORE the library is loaded (as bench.py does)
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--noprune-points", type=int, default=16384)
    ap.add_argument("--noprune-reps", type=int, default=3)
    ap.add_argument("--sets", default="abc")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distance_bench.jsonl"))
    args = ap.parse_args()
    lib = rt.load_library()
    dev = torch.device("cuda:0")
    scene = rt.Scene.load_off(bunny_path()).build_bvh(0)
    host = rt.Host(rt.Options.defaults(width=64, height=48, n_super_samples=1), 0)
    host.upload_scene(scene)
    lo, hi = scene.aabbs[0, :3].astype(np.float64), scene.aabbs[1, :3].astype(np.float64)
    centre, size = (lo + hi) / 2.0, float(np.linalg.norm(hi - lo))
    rng = np.random.default_rng(1)
    sets = {}
    if "a" in args.sets:
        sets["a_vertices_off_1e-3"] = (scene.vertices[:, :3] + np.float32(1e-3) * scene.vnormals[:, :3]).astype(np.float32)
    if "b" in args.sets:
        sets["b_uniform_in_box"] = (lo + rng.random((args.points, 3)) * (hi - lo)).astype(np.float32)
    if "c" in args.sets:
        d = rng.normal(size=(args.points, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        sets["c_shell_two_sizes_out"] = (centre + d * size * (2.0 + 0.2 * rng.random((args.points, 1)))).astype(np.float32)
    lines = []

    def emit(**kv):
        print(json.dumps(kv), flush=True)
        lines.append(json.dumps(kv))

    for name, points in sets.items():
        p4 = np.zeros((len(points), 4), np.float32)
        p4[:, :3] = points
        tp = torch.from_numpy(p4).to(dev)
        n = len(points)
        out = {"hit": torch.empty(n, dtype=torch.uint8, device=dev), "distance": torch.empty(n, dtype=torch.float32, device=dev),
               "leaf": torch.empty(n, dtype=torch.uint32, device=dev), "barycentric": torch.empty((n, 3), dtype=torch.float32, device=dev),
               "position": torch.empty((n, 3), dtype=torch.float32, device=dev), "normal": torch.empty((n, 3), dtype=torch.float32, device=dev)}
        arrays = _HitArrays(*[out[f].data_ptr() for f in FIELDS])
        torch.cuda.synchronize()
        forms = (("sorted", 0, {}, n, args.reps), ("unsorted", RT_QUERY_NO_SORT, {}, n, args.reps),
                 ("sorted_no_starting_bound", 0, {"no_start": True}, n, args.reps),
                 ("sorted_no_pruning", 0, {"no_prune": True}, min(n, args.noprune_points), args.noprune_reps))
        for form, flags, switches, m, reps in forms:
            def call(m=m, flags=flags):
                rc = lib.rt_closest_points_device(host._h, tp.data_ptr(), m, float("inf"), flags, C.byref(arrays), None)
                assert rc == 0, rc

            host.set_nearest_walk(**switches)
            for _ in range(args.warmup if reps > 3 else 1):
                call()
            ms = []
            for _ in range(reps):
                call()
                ms.append(host.last_query_ms)
            host.set_nearest_walk(count=True, **switches)
            call()
            nodes, tris = host.last_nearest_counts()
            host.set_nearest_walk()
            med = float(np.median(ms))
            emit(set=name, form=form, points=m, median_ms=med, min_ms=float(np.min(ms)), mpoints_per_s=m / med / 1e3,
                 box_tests_per_point=nodes / m, triangle_tests_per_point=tris / m, leaves=int(scene.num_faces),
                 found=int(out["hit"][:m].sum().item()))
        del tp, out
    host.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
