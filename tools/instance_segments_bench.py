#!/usr/bin/env python3
"""Instanced segment-query throughput (include/rt_hip_instance_segments.h): JSON lines appended to
profiles/instance_segments_bench.jsonl.

  identity        ONE identity instance against the plain form on the same build and the same inputs:
                  rt_instances_segments_occluded_device / rt_segments_occluded_device and the closest forms on --pairs box
                  segments, rt_instances_visibility_masks_device / rt_visibility_masks_device on --grid P T.  What the
                  nested walk costs where it buys nothing: a one-record top-level tree, twelve scalar loads, eighteen
                  multiply-adds and a second make_ray per packet.
  --instances S   the same three instanced calls against the set S (`grid:N`, tools/turntable.py's grammar: N x N x N turned
                  copies 1.5 box widths apart; or a .npy of float32 (n, 3, 4)), the ends uniform in the top-level root box.

Device entry points on buffers loaded beforehand.  The time of a call is rt_last_query_ms (HIP events around sort + walk +
resolve).  The forms of a comparison ALTERNATE, call by call, --warmup rounds untimed and then --reps rounds; a line holds the
median, the minimum and the quartiles of a form's times (tools/visibility_bench.py's `alternate`).

    python3 tools/instance_segments_bench.py [--mesh meshes/bunny.off] [--pairs 1048576] [--grid 4096 4096] [--instances grid:10]
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
from opencl_raytracer_amd.api import _HitArrays, _InstanceHitArrays, _VisibilityArrays  # noqa: E402
from tools.meshes import bunny_path  # noqa: E402
from tools.turntable import instance_poses  # noqa: E402
from tools.visibility_bench import alternate  # noqa: E402


def main():
    import torch

    torch.zeros(1, device="cuda:0")  # torch's HIP runtime up BEFORE the library is loaded (as bench.py does)
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default=None, help="an OFF file (default: the bunny)")
    ap.add_argument("--pairs", type=int, default=1 << 20)
    ap.add_argument("--grid", type=int, nargs=2, default=(4096, 4096), metavar=("P", "T"))
    ap.add_argument("--instances", default="grid:10", metavar="grid:N|FILE.npy")
    ap.add_argument("--interval", type=float, nargs=2, default=(1e-4, 1 - 1e-4), metavar=("LO", "HI"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "instance_segments_bench.jsonl"))
    args = ap.parse_args()
    if rt.device_count() < 1:
        sys.exit("instance_segments_bench: no HIP device visible (there is no CPU path to time)")
    t_lo, t_hi = (float(x) for x in args.interval)
    lib = rt.load_library()
    dev = torch.device("cuda:0")
    mesh = args.mesh or bunny_path()
    scene = rt.Scene.load_off(mesh).build_bvh(0)
    host = rt.Host(rt.Options.defaults(width=64, height=48, n_super_samples=1), 0)
    host.upload_scene(scene)
    rng = np.random.default_rng(1)
    lines = []
    common = {"mesh": os.path.basename(mesh), "leaves": int(scene.num_faces), "t_lo": t_lo, "t_hi": t_hi, "reps": args.reps,
              "warmup": args.warmup}

    def emit(**kv):
        kv = {**common, **kv}
        print(json.dumps(kv), flush=True)
        lines.append(json.dumps(kv))

    def in_box(n, lo, hi):
        p4 = np.zeros((n, 4), np.float32)
        p4[:, :3] = lo + rng.random((n, 3)) * (hi - lo)
        return torch.from_numpy(p4).to(dev)

    def query_ms(rc):
        assert rc == 0, rc
        return host.last_query_ms

    n, (n_points, n_targets) = args.pairs, args.grid
    total, words = n_points * n_targets, (n_targets + 31) // 32
    flag = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    distance = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
    leaf = torch.empty(max(n, 1), dtype=torch.uint32, device=dev)
    position = torch.empty((max(n, 1), 3), dtype=torch.float32, device=dev)
    normal = torch.empty((max(n, 1), 3), dtype=torch.float32, device=dev)
    instance = torch.empty(max(n, 1), dtype=torch.uint32, device=dev)
    record = _HitArrays(flag.data_ptr(), distance.data_ptr(), leaf.data_ptr(), None, position.data_ptr(), normal.data_ptr())
    instanced_record = _InstanceHitArrays(record, instance.data_ptr())
    mask = torch.empty((n_points, words), dtype=torch.uint32, device=dev)
    count = torch.empty(n_points, dtype=torch.uint32, device=dev)
    rows = _VisibilityArrays(mask.data_ptr(), count.data_ptr())

    def forms_for(a, b, points, targets, plain: bool) -> dict:
        forms = {}
        if plain:
            forms["segments_occluded"] = lambda: query_ms(lib.rt_segments_occluded_device(
                host._h, a.data_ptr(), b.data_ptr(), n, t_lo, t_hi, 0, flag.data_ptr(), None))
        forms["instances_segments_occluded"] = lambda: query_ms(lib.rt_instances_segments_occluded_device(
            host._h, a.data_ptr(), b.data_ptr(), n, t_lo, t_hi, 0, flag.data_ptr(), None))
        if plain:
            forms["segments_closest"] = lambda: query_ms(lib.rt_segments_closest_device(
                host._h, a.data_ptr(), b.data_ptr(), n, t_lo, t_hi, 0, C.byref(record), None))
        forms["instances_segments_closest"] = lambda: query_ms(lib.rt_instances_segments_closest_device(
            host._h, a.data_ptr(), b.data_ptr(), n, t_lo, t_hi, 0, C.byref(instanced_record), None))
        if plain:
            forms["visibility_masks"] = lambda: query_ms(lib.rt_visibility_masks_device(
                host._h, points.data_ptr(), n_points, targets.data_ptr(), n_targets, t_lo, t_hi, 0, C.byref(rows), None))
        forms["instances_visibility_masks"] = lambda: query_ms(lib.rt_instances_visibility_masks_device(
            host._h, points.data_ptr(), n_points, targets.data_ptr(), n_targets, t_lo, t_hi, 0, C.byref(rows), None))
        return forms

    def run(case: str, instances: int, lo, hi, plain: bool):
        a, b = in_box(n, lo, hi), in_box(n, lo, hi)
        points, targets = in_box(n_points, lo, hi), in_box(n_targets, lo, hi)
        torch.cuda.synchronize()
        forms = forms_for(a, b, points, targets, plain)
        got = alternate(forms, args.warmup, args.reps)
        for name, call in forms.items():  # (once more each, for the blocked share of the form's own answer)
            call()
            torch.cuda.synchronize()
            if "visibility" in name:
                items, blocked = total, int(count.view(torch.int32).sum(dtype=torch.int64).item())
            else:
                items, blocked = n, int(flag[:n].sum(dtype=torch.int64).item())
            emit(case=case, form=name, instances=instances, segments=items, points=n_points if "visibility" in name else None,
                 targets=n_targets if "visibility" in name else None, msegments_per_s=items / got[name]["median_ms"] / 1e3, blocked=blocked,
                 **got[name])
        if plain:
            for name in ("segments_occluded", "segments_closest", "visibility_masks"):
                emit(case=case, form="ratio " + name, instanced_over_plain=got["instances_" + name]["median_ms"] / got[name]["median_ms"])

    box_lo, box_hi = scene.aabbs[0, :3].astype(np.float64), scene.aabbs[1, :3].astype(np.float64)
    host.set_instances(np.eye(3, 4, dtype=np.float32)[None])
    run("identity", 1, box_lo, box_hi, plain=True)
    if args.instances:
        W = instance_poses(args.instances, scene)
        host.set_instances(W)
        nodes = host.instances()["nodes"]
        run(args.instances, len(W), nodes["lo"][0].astype(np.float64), nodes["hi"][0].astype(np.float64), plain=False)
    host.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
