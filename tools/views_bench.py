#!/usr/bin/env python3
"""What multi-view rendering costs (include/rt_hip_views.h) beside the route it replaces -- an upload and a layers call
per view --: one JSON line per measurement, appended to profiles/views_bench.jsonl (--out).

Bunny, 1920x1080, -s 1 -a 3, the eight orbit poses of tools/camera_bench.py; device entry points on pre-allocated
tensors; the time of a call is rt_last_query_ms (HIP events around everything the call enqueues, the waits for the
chunks' hit counts included); the median of --reps calls after --warmup, --rounds rounds:

  this library   rt_render_views_device against ONE host without a pose: all eight views in one call (V = 8) and each
                 view in a call of its own (V = 1), for ("value",), for ("value", "image") and for the record layers
                 alone (hit ... normal and direction: no ambient-occlusion step)
  the baseline   (--baseline-lib-dir, a directory of this package that holds a libocrt_hip.so built from the parent
                 commit, loaded through OCRT_LIB_DIR in a process of its own per round, alternating with this library's
                 rounds): per pose a host posed at that view -- its upload's wall time -- and rt_render_layers_device for
                 ("value",)

The last line is the gate: the slowest round of the V = 8 call for ("value",) must not exceed the sum, over the eight
poses, of the slowest baseline round of the layers call at that pose -- per view, the batch is no slower than the layers
call it stands for (it walks the same rays and casts fewer ambient-occlusion lanes).  It also says whether every view's
`value` of the V = 8 call sums to what the baseline's layers call at that pose sums to (the same reduction over the same
shape: equal bits give equal sums).

    python3 tools/views_bench.py [--baseline-lib-dir lib_parent] [--reps 20] [--warmup 5] [--rounds 3] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

RECORD_LAYERS = ("hit", "distance", "leaf", "barycentric", "position", "normal", "direction")
SETS = {"value": ("value",), "value_image": ("value", "image"), "records": RECORD_LAYERS}


def orbit(rt):
    out = []
    for k in range(8):
        a = 2 * np.pi * k / 8
        out.append((f"orbit_{45 * k}", rt.Camera.look_at((2 * np.sin(a), 0.4, 2 * np.cos(a)), (0, 0, 0))))
    return out


def emit(out, **kv):
    line = json.dumps(kv)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def timed(host, call, reps, warmup):
    for _ in range(warmup):
        assert call() == 0
    ms = []
    for _ in range(reps):
        assert call() == 0
        ms.append(host.last_query_ms)
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def baseline_round(args):
    """One round of the baseline, in a process of its own (OCRT_LIB_DIR chooses the library): upload and layers call per pose."""
    import torch

    torch.zeros(1, device="cuda:0")  # torch's HIP runtime up BEFORE the library is loaded (as bench.py does)
    import opencl_raytracer_amd as rt
    from opencl_raytracer_amd.api import _LayerArrays
    from tools.meshes import bunny_path

    lib = rt.load_library()
    scene = rt.Scene.load_off(bunny_path()).build_bvh(0)
    opt = rt.Options.defaults(width=args.width, height=args.height, n_super_samples=1, ao_num_samples=3)
    value = torch.empty((opt.total_height, opt.total_width), dtype=torch.float32, device="cuda:0")
    arrays = _LayerArrays(value=value.data_ptr())
    for name, cam in orbit(rt):
        host = rt.Host(opt, 0)
        host.expect_frames(1 << 20)  # (a stream host: the upload a turntable of frames pays)
        host.set_camera(cam)
        t0 = time.perf_counter()
        host.upload_scene(scene)
        upload_ms = (time.perf_counter() - t0) * 1e3
        med, best, worst = timed(host, lambda: lib.rt_render_layers_device(host._h, C.byref(arrays), None), args.reps, args.warmup)
        torch.cuda.synchronize()
        emit(args.out, bench="views", library="baseline", what="render_layers_value", pose=name, round=args.round, median_ms=med,
             min_ms=best, max_ms=worst, upload_wall_ms=upload_ms, value_sum=float(value.sum()), reps=args.reps, warmup=args.warmup)
        host.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib-dir", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "views_bench.jsonl"))
    ap.add_argument("--baseline-round", action="store_true", help=argparse.SUPPRESS)  # (the child processes)
    ap.add_argument("--round", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.baseline_round:
        return baseline_round(args)
    import torch

    torch.zeros(1, device="cuda:0")
    import opencl_raytracer_amd as rt
    from opencl_raytracer_amd.api import _LayerArrays, _ViewArrays
    from tools.meshes import bunny_path

    lib = rt.load_library()
    scene = rt.Scene.load_off(bunny_path()).build_bvh(0)
    opt = rt.Options.defaults(width=args.width, height=args.height, n_super_samples=1, ao_num_samples=3)
    poses = orbit(rt)
    cameras = np.stack([cam.as_array() for _, cam in poses])
    host = rt.Host(opt, 0)
    t0 = time.perf_counter()
    host.upload_scene(scene)
    emit(args.out, bench="views", library="this", what="upload", upload_wall_ms=(time.perf_counter() - t0) * 1e3)
    first = host.render_views(cameras, rt.VIEW_OUTPUTS, as_torch=True)  # pre-allocated outputs, and what the hits are
    torch.cuda.synchronize()
    hits = [int(first["hit"][v].sum()) for v in range(8)]

    def arrays_of(names, v0, v1):
        ptr = {n: first[n][v0:v1].data_ptr() for n in names}
        return _ViewArrays(_LayerArrays(**{n: p for n, p in ptr.items() if n != "image"}), ptr.get("image"))

    medians = {}
    for round_ in range(args.rounds):
        if args.baseline_lib_dir:
            env = dict(os.environ, OCRT_LIB_DIR=args.baseline_lib_dir, OCRT_ALLOW_OLD_LIB="1")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--baseline-round", "--round", str(round_), "--reps", str(args.reps),
                            "--warmup", str(args.warmup), "--width", str(args.width), "--height", str(args.height), "--out", args.out],
                           env=env, check=True, timeout=900)
        for set_name, names in SETS.items():
            arrays = arrays_of(names, 0, 8)
            med, best, worst = timed(host, lambda: lib.rt_render_views_device(host._h, cameras.ctypes.data, 8, C.byref(arrays), None),
                                     args.reps, args.warmup)
            done = host.last_views()
            medians.setdefault((set_name, "v8"), []).append(med)
            emit(args.out, bench="views", library="this", what="render_views", outputs=set_name, views=8, round=round_, median_ms=med, min_ms=best,
                 max_ms=worst, ms_per_view=med / 8, chunks=done["chunks"], ao_points=done["ao_points"], sub_pixels=8 * opt.total_width * opt.total_height,
                 reps=args.reps, warmup=args.warmup)
            for v, (name, _) in enumerate(poses):
                one = arrays_of(names, v, v + 1)
                med, best, worst = timed(host, lambda: lib.rt_render_views_device(host._h, cameras[v:v + 1].ctypes.data, 1, C.byref(one), None),
                                         args.reps, args.warmup)
                medians.setdefault((set_name, name), []).append(med)
                emit(args.out, bench="views", library="this", what="render_views", outputs=set_name, views=1, pose=name, round=round_, median_ms=med,
                     min_ms=best, max_ms=worst, hits=hits[v], ao_points=host.last_views()["ao_points"], reps=args.reps, warmup=args.warmup)
    torch.cuda.synchronize()
    # (what the timed calls left in the arrays: the last V = 1 calls of the record layers, under them the V = 8 values)
    arrays = arrays_of(SETS["value"], 0, 8)
    assert lib.rt_render_views_device(host._h, cameras.ctypes.data, 8, C.byref(arrays), None) == 0
    torch.cuda.synchronize()
    value_sums = {name: float(first["value"][v].sum()) for v, (name, _) in enumerate(poses)}
    host.close()
    # the gate, from the baseline's lines of this run
    baseline = {}
    if args.baseline_lib_dir and os.path.exists(args.out):
        for line in open(args.out):
            kv = json.loads(line)
            if kv.get("library") == "baseline" and kv.get("what") == "render_layers_value":
                baseline.setdefault(kv["pose"], []).append(kv)
        baseline = {pose: rows[-args.rounds:] for pose, rows in baseline.items()}
    v8_worst = max(medians[("value", "v8")])
    gate = dict(bench="views_gate", v8_value_slowest_round_ms=v8_worst, v8_value_ms_per_view=v8_worst / 8,
                v8_value_image_slowest_round_ms=max(medians[("value_image", "v8")]), v8_records_slowest_round_ms=max(medians[("records", "v8")]),
                v1_value_sum_of_slowest_rounds_ms=sum(max(medians[("value", name)]) for name, _ in poses), hits=hits)
    if len(baseline) == 8:
        slowest = {pose: max(r["median_ms"] for r in rows) for pose, rows in baseline.items()}
        uploads = [r["upload_wall_ms"] for rows in baseline.values() for r in rows]
        total = sum(slowest.values())
        gate.update(baseline_layers_value_sum_of_slowest_rounds_ms=total, baseline_layers_value_ms_per_view=total / 8,
                    baseline_upload_wall_ms_median=float(np.median(uploads)), v8_over_baseline=v8_worst / total,
                    gate_v8_not_slower_than_baseline=bool(v8_worst <= total),
                    v1_not_slower_by_pose={name: bool(max(medians[("value", name)]) <= slowest[name]) for name, _ in poses},
                    value_sums_equal_baseline=all(r["value_sum"] == value_sums[pose] for pose, rows in baseline.items() for r in rows),
                    views_per_s_batch=8e3 / v8_worst, views_per_s_upload_per_view=8e3 / (total + 8 * float(np.median(uploads))))
    emit(args.out, **gate)


if __name__ == "__main__":
    main()
