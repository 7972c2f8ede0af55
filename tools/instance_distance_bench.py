#!/usr/bin/env python3
"""Instanced closest-point query throughput on the bunny (include/rt_hip_instance_nearest.h): one JSON line per (instance set,
point set), appended to profiles/instance_distance_bench.jsonl.

Instance sets (--instances, repeatable):  identity | grid:N (N x N x N copies, translated and rotated, 1.6 box sizes apart) |
                                          many:N (tests/instance_cases.py: N rotated, scaled copies scattered over a cube)
Point sets:  (a) --points points uniform in the top-level root box
             (b) points on the world surface: the copies' vertices pushed 1e-3 along their world normals (at most --points)
             (c) --points points far away: a shell two top-level box sizes out
The counters are the A/B build's (opencl_raytracer_amd/lib_knobs, rt_debug_set_nearest_walk): this tool loads that build.
Device entry points on pre-loaded buffers; the time of a call is rt_last_query_ms (HIP events around sort + walk), the median
of --reps calls after --warmup; box tests and triangle tests per point come from one more, counted call.  With --plain the
same points also go through rt_closest_points (the uploaded scene alone), for the instanced-to-plain ratio of `identity`.

    python3 tools/instance_distance_bench.py [--instances identity --instances grid:3 ...] [--reps 20] [--points 1048576]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
os.environ.setdefault("OCRT_LIB_DIR", "lib_knobs")  # the build that has the counters

import opencl_raytracer_amd as rt  # noqa: E402
from opencl_raytracer_amd.api import _HitArrays, _InstanceHitArrays  # noqa: E402
from tools.meshes import bunny_path  # noqa: E402

FIELDS = ("hit", "distance", "leaf", "barycentric", "position", "normal")


def rotation(rng) -> np.ndarray:
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))[None, :]
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def transforms(spec: str, scene) -> np.ndarray:
    lo, hi = scene.aabbs[0, :3].astype(np.float64), scene.aabbs[1, :3].astype(np.float64)
    centre, ext = (lo + hi) / 2, hi - lo
    kind, _, count = spec.partition(":")
    if kind == "identity":
        W = np.zeros((1, 3, 4))
        W[0, :, :3] = np.eye(3)
    elif kind == "grid":
        n, rng, W = int(count), np.random.default_rng(17), []
        for i in range(n):
            for j in range(n):
                for k in range(n):
                    A = rotation(rng)
                    W.append(np.concatenate([A, (centre - A @ centre + (np.array([i, j, k]) - (n - 1) / 2) * ext.max() * 1.6)[:, None]], axis=1))
        W = np.stack(W)
    elif kind == "many":
        import instance_cases

        W = instance_cases.many(scene, int(count))
    else:
        raise SystemExit(f"unknown instance set {spec!r}")
    return np.ascontiguousarray(W, np.float32)


def main():
    import torch

    torch.zeros(1, device="cuda:0")  # torch's HIP runtime up BEFORE the library is loaded (as bench.py does)
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", action="append", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--sets", default="abc")
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "instance_distance_bench.jsonl"))
    args = ap.parse_args()
    lib = rt.load_library()
    dev = torch.device("cuda:0")
    scene = rt.Scene.load_off(bunny_path()).build_bvh(0)
    host = rt.Host(rt.Options.defaults(width=64, height=48, n_super_samples=1), 0)
    host.upload_scene(scene)
    lines = []

    def emit(**kv):
        print(json.dumps(kv), flush=True)
        lines.append(json.dumps(kv))

    for spec in args.instances or ["identity", "grid:3", "grid:5", "many:1000"]:
        W = transforms(spec, scene)
        host.set_instances(W)
        plan = host.instances()
        lo, hi = plan["nodes"]["lo"][0].astype(np.float64), plan["nodes"]["hi"][0].astype(np.float64)
        centre, size = (lo + hi) / 2.0, float(np.linalg.norm(hi - lo))
        rng = np.random.default_rng(1)
        sets = {}
        if "a" in args.sets:
            sets["a_uniform_in_top_box"] = (lo + rng.random((args.points, 3)) * (hi - lo)).astype(np.float32)
        if "b" in args.sets:
            per_copy = max(1, min(len(scene.vertices), args.points // len(W)))
            pick = rng.choice(len(scene.vertices), per_copy, replace=False)
            v, vn = scene.vertices[pick, :3].astype(np.float64), scene.vnormals[pick, :3].astype(np.float64)
            on = []
            for w in W.astype(np.float64):
                normal = vn @ np.linalg.inv(w[:, :3])
                normal /= np.maximum(np.linalg.norm(normal, axis=1, keepdims=True), 1e-30)
                on.append(v @ w[:, :3].T + w[:, 3] + 1e-3 * normal)
            sets["b_world_vertices_off_1e-3"] = np.concatenate(on).astype(np.float32)
        if "c" in args.sets:
            d = rng.normal(size=(args.points, 3))
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            sets["c_shell_two_sizes_out"] = (centre + d * size * (2.0 + 0.2 * rng.random((args.points, 1)))).astype(np.float32)
        for name, points in sets.items():
            n = len(points)
            p4 = np.zeros((n, 4), np.float32)
            p4[:, :3] = points
            tp = torch.from_numpy(p4).to(dev)
            out = {"hit": torch.empty(n, dtype=torch.uint8, device=dev), "distance": torch.empty(n, dtype=torch.float32, device=dev),
                   "leaf": torch.empty(n, dtype=torch.uint32, device=dev), "barycentric": torch.empty((n, 3), dtype=torch.float32, device=dev),
                   "position": torch.empty((n, 3), dtype=torch.float32, device=dev), "normal": torch.empty((n, 3), dtype=torch.float32, device=dev),
                   "instance": torch.empty(n, dtype=torch.uint32, device=dev)}
            hits = _HitArrays(*[out[f].data_ptr() for f in FIELDS])
            arrays = _InstanceHitArrays(hits, out["instance"].data_ptr())
            torch.cuda.synchronize()

            def instanced():
                rc = lib.rt_instances_closest_points_device(host._h, tp.data_ptr(), n, float("inf"), 0, C.byref(arrays), None)
                assert rc == 0, rc

            def plain():
                rc = lib.rt_closest_points_device(host._h, tp.data_ptr(), n, float("inf"), 0, C.byref(hits), None)
                assert rc == 0, rc

            for form, call in (("instanced", instanced),) + ((("plain", plain),) if args.plain else ()):
                host.set_nearest_walk()
                for _ in range(args.warmup):
                    call()
                ms = []
                for _ in range(args.reps):
                    call()
                    ms.append(host.last_query_ms)
                host.set_nearest_walk(count=True)
                call()
                nodes, tris = host.last_nearest_counts()
                host.set_nearest_walk()
                med = float(np.median(ms))
                emit(instances=spec, copies=len(W), set=name, form=form, points=n, median_ms=med, min_ms=float(np.min(ms)),
                     max_ms=float(np.max(ms)), mpoints_per_s=n / med / 1e3, box_tests_per_point=nodes / n,
                     triangle_tests_per_point=tris / n, leaves=int(scene.num_faces), found=int(out["hit"].sum().item()))
            del tp, out
    host.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
