#!/usr/bin/env python3
"""What the frame layers cost (include/rt_hip_layers.h) beside the route they replace: one JSON line per measurement,
appended to profiles/layers_bench.jsonl (--out).

Bunny, 1920x1080, -s 1 -a 3, a host without a pose, one given the default pose and one at orbit_135; device entry points on pre-allocated tensors;
the time of a call is rt_last_query_ms (HIP events around everything the call enqueues); the median of --reps calls
after --warmup, in --rounds alternating rounds within one process:

  (a) the six record layers plus `direction` through rt_render_layers_device
  (b) the route without them: rt_trace_closest_device with RT_QUERY_NO_SORT on the same rays -- the `direction` layer and
      the eye as float4 in index order --, all six outputs
  (c) the `ao` layer alone
  (d) rt_trace_ao_device with RT_QUERY_NO_SORT over the same N points (the position and normal layers as float4)

The last line per pose is the gate: the slowest round of (a) must not exceed the slowest round of (b).

    python3 tools/layers_bench.py [--reps 20] [--warmup 5] [--rounds 3] [--width 1920 --height 1080] [--out FILE]
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
from opencl_raytracer_amd.api import RT_QUERY_NO_SORT, _HitArrays, _LayerArrays  # noqa: E402
from tools.meshes import bunny_path  # noqa: E402

RECORD = ("hit", "distance", "leaf", "barycentric", "position", "normal")


def poses():
    a = np.radians(135)
    # (default_pose: the reference's view through the posed instantiation -- what the pose itself costs, the view being equal)
    return (("unposed", None), ("default_pose", rt.Camera.default()),
            ("orbit_135", rt.Camera.look_at((2 * np.sin(a), 0.0, 2 * np.cos(a)), (0, 0, 0))))


def main():
    import torch

    torch.zeros(1, device="cuda:0")  # torch's HIP runtime up BEFORE the library is loaded (as bench.py does)
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layers_bench.jsonl"))
    args = ap.parse_args()
    lib = rt.load_library()
    dev = torch.device("cuda:0")
    scene = rt.Scene.load_off(bunny_path()).build_bvh(0)
    opt = rt.Options.defaults(width=args.width, height=args.height, n_super_samples=1, ao_num_samples=3)
    n = opt.total_width * opt.total_height
    sink = open(args.out, "a")

    def emit(**kv):
        line = json.dumps(kv)
        print(line, flush=True)
        sink.write(line + "\n")
        sink.flush()

    def timed(host, call):
        for _ in range(args.warmup):
            assert call() == 0
        ms = []
        for _ in range(args.reps):
            assert call() == 0
            ms.append(host.last_query_ms)
        return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))

    for pose_name, cam in poses():
        host = rt.Host(opt, 0)
        if cam is not None:
            host.set_camera(cam)
        host.upload_scene(scene)
        first = host.render_layers(as_torch=True)  # the inputs of (b) and (d), and what their results are compared with
        torch.cuda.synchronize()
        eye = torch.tensor(list(host.camera().as_array()[0]) + [0.0], dtype=torch.float32, device=dev)
        origins = eye.repeat(n, 1).contiguous()
        directions = torch.nn.functional.pad(first["direction"].reshape(n, 3), (0, 1)).contiguous()
        points = torch.nn.functional.pad(first["position"].reshape(n, 3), (0, 1)).contiguous()
        normals = torch.nn.functional.pad(first["normal"].reshape(n, 3), (0, 1)).contiguous()
        out_a = {f: torch.empty_like(first[f]) for f in RECORD + ("direction",)}
        out_b = {f: torch.empty_like(first[f]) for f in RECORD}
        ao_c, ao_d = torch.empty_like(first["ao"]), torch.empty_like(first["ao"])
        torch.cuda.synchronize()
        arrays_a = _LayerArrays(**{f: t.data_ptr() for f, t in out_a.items()})
        arrays_b = _HitArrays(*[out_b[f].data_ptr() for f in RECORD])
        arrays_c = _LayerArrays(ao=ao_c.data_ptr())
        calls = {
            "a_layers_records": lambda: lib.rt_render_layers_device(host._h, C.byref(arrays_a), None),
            "b_trace_closest": lambda: lib.rt_trace_closest_device(host._h, origins.data_ptr(), directions.data_ptr(), n, 100000.0,
                                                                   RT_QUERY_NO_SORT, C.byref(arrays_b), None),
            "c_layers_ao": lambda: lib.rt_render_layers_device(host._h, C.byref(arrays_c), None),
            "d_trace_ao": lambda: lib.rt_trace_ao_device(host._h, points.data_ptr(), normals.data_ptr(), None, n, RT_QUERY_NO_SORT,
                                                         ao_d.data_ptr(), None, None),
        }
        medians = {name: [] for name in calls}
        for round_ in range(args.rounds):
            for name, call in calls.items():
                med, best, worst = timed(host, call)
                medians[name].append(med)
                emit(bench="layers", pose=pose_name, width=opt.total_width, height=opt.total_height, sub_pixels=n, round=round_, what=name,
                     median_ms=med, min_ms=best, max_ms=worst, reps=args.reps, warmup=args.warmup)
        torch.cuda.synchronize()
        hit = first["hit"].bool()
        same = all(bool((out_a[f].view(torch.int32) == out_b[f].view(torch.int32)).all()) if out_a[f].dtype != torch.uint8
                   else bool((out_a[f] == out_b[f]).all()) for f in RECORD)
        same_ao = bool((ao_c[hit].view(torch.int32) == ao_d[hit].view(torch.int32)).all())
        a_worst, b_worst = max(medians["a_layers_records"]), max(medians["b_trace_closest"])
        emit(bench="layers_gate", pose=pose_name, sub_pixels=n, hits=int(hit.sum()), a_slowest_round_ms=a_worst, b_slowest_round_ms=b_worst,
             a_over_b=a_worst / b_worst, gate_a_not_slower_than_b=bool(a_worst <= b_worst), c_slowest_round_ms=max(medians["c_layers_ao"]),
             d_slowest_round_ms=max(medians["d_trace_ao"]), a_equals_b_bitwise=same, c_equals_d_where_hit_bitwise=same_ao)
        host.close()
    sink.close()


if __name__ == "__main__":
    main()
