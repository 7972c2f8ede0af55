#!/usr/bin/env python3
"""Directional occlusion queries against the ambient-occlusion query they extend (include/rt_hip_directional.h,
include/rt_hip_ao.h): the bunny, default AO options, the closest hits of the 1920 x 1080 reference camera -- DESIGN.md 11's
set, 1 154 670 points, 32.3 M rays.  Device tensors on one torch stream, sort=False, the time of a call is
rt_last_query_ms; the median of --reps calls after --warmup, over --rounds alternating rounds, every round in a process of
its own per library.  One JSON line per row and round, appended to --out:

  ao_query            rt_trace_ao_device                                       (baseline library, and this one)
  mask                rt_trace_ao_directional_device, ("mask",)
  mask_bent           ("mask", "bent")
  all                 ("ao", "occluded", "mask", "bent")
  ao_rays             rt_ao_rays_device, origins and directions
  composed            the route without the fused query: rt_ao_rays_device, rt_trace_occluded_device over the n x R rays,
                      the flags packed into words in torch (HIP events on the stream around the three steps)

    python3 tools/directional_bench.py --baseline-lib-dir lib_parent     # a build of the parent commit in the package

The gate (last line): the slowest round of `mask` may exceed the baseline's slowest `ao_query` round by the baseline's own
spread over its rounds or by 1 %, whichever is larger.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def emit(path, **kv):
    line = json.dumps(kv)
    print(line, flush=True)
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def one_round(args):
    """One library, one process: its rows."""
    import torch

    torch.zeros(1, device="cuda:0")  # torch's HIP runtime up BEFORE the library is loaded (as bench.py does)
    import opencl_raytracer_amd as rt
    import orc
    import query_oracle as qo
    from opencl_raytracer_amd.api import RT_QUERY_NO_SORT, _HitArrays
    from tools.meshes import bunny_path

    lib = rt.load_library()
    dev = torch.device("cuda:0")
    scene = rt.Scene.load_off(bunny_path()).build_bvh(0)
    opt = rt.Options.defaults(width=args.width, height=args.height, n_super_samples=1)
    host = rt.Host(opt, 0)
    host.upload_scene(scene)
    R, _ = host.ao_rays_per_point
    o4, d4 = qo.camera_rays(orc.params_from_options(opt))
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        cam = host.trace_closest(torch.from_numpy(o4).to(dev), torch.from_numpy(d4).to(dev), outputs=("hit", "position", "normal"))
        hit = cam["hit"].bool()
        points = torch.nn.functional.pad(cam["position"][hit], (0, 1)).contiguous()
        normals = torch.nn.functional.pad(cam["normal"][hit], (0, 1)).contiguous()
        n = int(points.shape[0])
        ao = torch.empty(n, dtype=torch.float32, device=dev)
        occluded = torch.empty(n, dtype=torch.uint32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        side.synchronize()
        del cam
        rows = {"ao_query": lambda: lib.rt_trace_ao_device(host._h, points.data_ptr(), normals.data_ptr(), None, n, RT_QUERY_NO_SORT,
                                                           ao.data_ptr(), occluded.data_ptr(), stream)}
        if args.library == "this":
            from opencl_raytracer_amd.api import _DirectionalArrays

            W = host.ao_mask_words
            mask = torch.empty((n, W), dtype=torch.uint32, device=dev)
            bent = torch.empty((n, 3), dtype=torch.float32, device=dev)
            origins = torch.empty((n, 4), dtype=torch.float32, device=dev)
            directions = torch.empty((n, R, 4), dtype=torch.float32, device=dev)
            flags = torch.empty(n * R, dtype=torch.uint8, device=dev)
            sets = {"mask": _DirectionalArrays(None, None, mask.data_ptr(), None),
                    "mask_bent": _DirectionalArrays(None, None, mask.data_ptr(), bent.data_ptr()),
                    "all": _DirectionalArrays(ao.data_ptr(), occluded.data_ptr(), mask.data_ptr(), bent.data_ptr())}
            for name, arrays in sets.items():
                rows[name] = lambda arrays=arrays: lib.rt_trace_ao_directional_device(
                    host._h, points.data_ptr(), normals.data_ptr(), None, n, RT_QUERY_NO_SORT, C.byref(arrays), stream)
            rows["ao_rays"] = lambda: lib.rt_ao_rays_device(host._h, points.data_ptr(), normals.data_ptr(), None, n, origins.data_ptr(),
                                                            directions.data_ptr(), stream)
        for name, call in rows.items():
            ms = []
            for i in range(args.warmup + args.reps):
                assert call() == 0, name
                if i >= args.warmup:
                    ms.append(host.last_query_ms)
            emit(args.out, bench="directional", library=args.library, row=name, round=args.round, points=n, rays_per_point=R, rays=n * R,
                 median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), reps=args.reps, warmup=args.warmup)
        if args.library == "this":
            # the composed route, for comparison; and what it computes is what the fused query does
            weights = (torch.ones(32, dtype=torch.int64, device=dev) << torch.arange(32, device=dev))
            k = torch.arange(R, device=dev)
            md = float(opt.ao_max_distance)

            def composed():
                assert rows["ao_rays"]() == 0
                every = origins.repeat_interleave(R, dim=0)
                assert lib.rt_trace_occluded_device(host._h, every.data_ptr(), directions.data_ptr(), n * R, md, RT_QUERY_NO_SORT,
                                                    flags.data_ptr(), stream) == 0
                packed = torch.zeros((n, W), dtype=torch.int64, device=dev)
                packed.index_add_(1, k >> 5, flags.view(n, R).to(torch.int64) * weights[k & 31])
                every.record_stream(torch.cuda.current_stream(dev))
                return packed

            ms, walks = [], []
            for i in range(args.warmup + args.reps):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                packed = composed()
                t1.record()
                t1.synchronize()
                if i >= args.warmup:
                    ms.append(t0.elapsed_time(t1))
                    walks.append(host.last_query_ms)
            assert rows["mask"]() == 0
            side.synchronize()
            same = bool((packed == mask.view(torch.int32).to(torch.int64).bitwise_and(0xFFFFFFFF)).all())
            emit(args.out, bench="directional", library="this", row="composed", round=args.round, points=n, rays_per_point=R, rays=n * R,
                 median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)),
                 occluded_query_median_ms=float(np.median(walks)), equals_fused_mask=same, reps=args.reps, warmup=args.warmup)
            assert same, "the composed route and the fused query disagree"
        side.synchronize()
    host.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib-dir", default=None, help="a directory of the package holding a build of the parent commit's library")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "directional_bench.jsonl"))
    ap.add_argument("--library", default=None, help=argparse.SUPPRESS)  # (the child processes)
    ap.add_argument("--round", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.library:
        return one_round(args)
    before = sum(1 for _ in open(args.out)) if os.path.exists(args.out) else 0
    for round_ in range(args.rounds):
        for library in (["baseline"] if args.baseline_lib_dir else []) + ["this"]:
            env = dict(os.environ)
            if library == "baseline":
                env.update(OCRT_LIB_DIR=args.baseline_lib_dir, OCRT_ALLOW_OLD_LIB="1")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--library", library, "--round", str(round_), "--reps", str(args.reps),
                            "--warmup", str(args.warmup), "--width", str(args.width), "--height", str(args.height), "--out", args.out],
                           env=env, check=True, timeout=900)
    lines = [json.loads(line) for line in open(args.out)][before:]
    medians = {}
    for kv in lines:
        medians.setdefault((kv["library"], kv["row"]), []).append(kv["median_ms"])
    gate = dict(bench="directional_gate", rounds=args.rounds,
                **{f"{lib_}_{row}_slowest_round_ms": max(v) for (lib_, row), v in sorted(medians.items())})
    if ("baseline", "ao_query") in medians:
        base = medians[("baseline", "ao_query")]
        allowance = max(max(base) - min(base), 0.01 * max(base))
        gate.update(baseline_spread_ms=max(base) - min(base), allowance_ms=allowance, limit_ms=max(base) + allowance,
                    passed=max(medians[("this", "mask")]) <= max(base) + allowance)
    emit(args.out, **gate)
    if gate.get("passed") is False:
        sys.exit("directional_bench: the mask query is slower than the baseline's ambient-occlusion query allows")


if __name__ == "__main__":
    main()
