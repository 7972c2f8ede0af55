#!/usr/bin/env python3
"""Voxelises a mesh with the signed distance queries (include/rt_hip_signed.h) and times the grid form against the point form
on the same voxels: one JSON line per form, appended to profiles/sdf_bench.jsonl.

Forms:  grid               rt_signed_distance_grid_device, distances alone (one float per voxel)
        grid_with_leaf     the same with the leaf array
        points_sorted      rt_signed_distance_device on the voxels' points written out, every output
        points_unsorted    the same with RT_QUERY_NO_SORT
        points_distance    sorted and unsorted once more with `distance` as the only output
        closest_points     rt_closest_points_device on the same points, sorted: what the sign costs
        table_build        rt_prepare_signed_distance after a fresh upload (sorts, incidence, sums), --table-reps uploads
        table_refresh      the sums alone, after rt_update_vertices
The grid is --grid^3 voxels over the mesh's box scaled by --factor about its centre.  Device entry points on pre-loaded
buffers; the time of a call is rt_last_query_ms (HIP events around sort + walk), the median of --reps calls after --warmup.
The forms are checked against each other before anything is timed: every voxel equals the point form's distance, bit for bit.

    python3 tools/sdf_bench.py [--grid 128] [--reps 20] [--warmup 3] [--mesh bunny]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import opencl_raytracer_amd as rt  # noqa: E402
from opencl_raytracer_amd.api import RT_QUERY_NO_SORT, _HitArrays, _SignedArrays  # noqa: E402
from tools.meshes import bunny_path  # noqa: E402

FIELDS = ("hit", "distance", "leaf", "barycentric", "position", "normal")


def main():
    import torch

    torch.zeros(1, device="cuda:0")  # torch's HIP runtime up BEFORE the library is loaded (as bench.py does)
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--factor", type=float, default=1.25)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--table-reps", type=int, default=5)
    ap.add_argument("--mesh", default="bunny", help="bunny, or the path of an OFF file")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sdf_bench.jsonl"))
    args = ap.parse_args()
    lib = rt.load_library()
    dev = torch.device("cuda:0")
    scene = rt.Scene.load_off(bunny_path() if args.mesh == "bunny" else args.mesh).build_bvh(0)
    opts = rt.Options.defaults(width=64, height=48, n_super_samples=1)
    host = rt.Host(opts, 0)
    host.upload_scene(scene)
    lo, hi = scene.aabbs[0, :3].astype(np.float64), scene.aabbs[1, :3].astype(np.float64)
    centre, half = (lo + hi) / 2.0, (hi - lo) / 2.0 * args.factor
    g = args.grid
    origin = (centre - half).astype(np.float32)
    spacing = (2.0 * half / max(g - 1, 1)).astype(np.float32)
    dims = np.array([g, g, g], np.uint32)
    n = g ** 3
    lines = []

    def emit(**kv):
        kv = dict(mesh=args.mesh, leaves=int(scene.num_faces), grid=g, voxels=n, **kv)
        print(json.dumps(kv), flush=True)
        lines.append(json.dumps(kv))

    def timed(call, reps=args.reps):
        for _ in range(args.warmup):
            call()
        ms = []
        for _ in range(reps):
            call()
            ms.append(host.last_query_ms)
        return float(np.median(ms)), float(np.min(ms))

    # the table: a fresh upload each time, then an update
    build_ms, refresh_ms = [], []
    for _ in range(args.table_reps):
        fresh = rt.Host(opts, 0)
        fresh.upload_scene(scene)
        fresh.prepare_signed_distance()
        build_ms.append(fresh.last_sign_build_ms())
        fresh.update_vertices(scene.vertices)
        fresh.prepare_signed_distance()
        refresh_ms.append(fresh.last_sign_build_ms())
        fresh.close()
    emit(form="table_build", median_ms=float(np.median(build_ms)), min_ms=float(np.min(build_ms)), table_bytes=120 * int(scene.num_faces))
    emit(form="table_refresh", median_ms=float(np.median(refresh_ms)), min_ms=float(np.min(refresh_ms)))

    host.prepare_signed_distance()  # (kept out of the first query's time)
    # the voxels' points, as the header states them
    axis = [origin[k] + np.arange(g, dtype=np.float32) * spacing[k] for k in range(3)]
    zz, yy, xx = np.meshgrid(axis[2], axis[1], axis[0], indexing="ij")
    p4 = np.zeros((n, 4), np.float32)
    p4[:, 0], p4[:, 1], p4[:, 2] = xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)
    tp = torch.from_numpy(p4).to(dev)
    out = {"hit": torch.empty(n, dtype=torch.uint8, device=dev), "distance": torch.empty(n, dtype=torch.float32, device=dev),
           "leaf": torch.empty(n, dtype=torch.uint32, device=dev), "barycentric": torch.empty((n, 3), dtype=torch.float32, device=dev),
           "position": torch.empty((n, 3), dtype=torch.float32, device=dev), "normal": torch.empty((n, 3), dtype=torch.float32, device=dev)}
    feature = torch.empty(n, dtype=torch.uint8, device=dev)
    pseudo = torch.empty((n, 4), dtype=torch.float32, device=dev)
    grid = torch.empty((g, g, g), dtype=torch.float32, device=dev)
    grid_leaf = torch.empty((g, g, g), dtype=torch.uint32, device=dev)
    record = _HitArrays(*[out[f].data_ptr() for f in FIELDS])
    everything = _SignedArrays(record, feature.data_ptr(), pseudo.data_ptr())
    distance_only = _SignedArrays(_HitArrays(None, out["distance"].data_ptr(), None, None, None, None), None, None)
    inf = float("inf")

    def grid_call(with_leaf):
        rc = lib.rt_signed_distance_grid_device(host._h, origin.ctypes.data, spacing.ctypes.data, dims.ctypes.data, inf, grid.data_ptr(),
                                                grid_leaf.data_ptr() if with_leaf else None, None)
        assert rc == 0, rc

    def point_call(arrays, flags):
        rc = lib.rt_signed_distance_device(host._h, tp.data_ptr(), n, inf, flags, C.byref(arrays), None)
        assert rc == 0, rc

    def plain_call():
        rc = lib.rt_closest_points_device(host._h, tp.data_ptr(), n, inf, 0, C.byref(record), None)
        assert rc == 0, rc

    # the forms agree before anything is timed
    grid_call(True)
    point_call(everything, 0)
    torch.cuda.synchronize()
    assert torch.equal(grid.reshape(-1).view(torch.int32), out["distance"].view(torch.int32)), "the grid differs from the point form"
    assert torch.equal(grid_leaf.reshape(-1).view(torch.int32), out["leaf"].view(torch.int32)), "the grid's leaves differ from the point form's"
    inside = int((grid < 0).sum().item())

    for form, call in (("grid", lambda: grid_call(False)), ("grid_with_leaf", lambda: grid_call(True)),
                       ("points_sorted", lambda: point_call(everything, 0)),
                       ("points_unsorted", lambda: point_call(everything, RT_QUERY_NO_SORT)),
                       ("points_distance_sorted", lambda: point_call(distance_only, 0)),
                       ("points_distance_unsorted", lambda: point_call(distance_only, RT_QUERY_NO_SORT)),
                       ("closest_points_sorted", plain_call)):
        med, least = timed(call)
        emit(form=form, median_ms=med, min_ms=least, mvoxels_per_s=n / med / 1e3, inside=inside)
    host.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
