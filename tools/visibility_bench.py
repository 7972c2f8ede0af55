#!/usr/bin/env python3
"""Segment-query throughput (include/rt_hip_segment.h) against the ray queries it stands beside: JSON lines appended to
profiles/visibility_bench.jsonl.

  --pairs N        N segments with both endpoints uniform in the root box: rt_segments_occluded_device against
                   rt_trace_occluded_device on the rays (a, b - a) with max_distance = t_hi -- the same walk, plus one
                   compare per accepted triangle and one subtraction per ray --, each sorted and with RT_QUERY_NO_SORT.
  --grid P T       P points against T targets (may be given more than once): rt_visibility_masks_device against
                   rt_trace_occluded_device on the P x T rays written out point by point (the walk alone, in the mask
                   form's ray order when unsorted), with the time and the bytes of writing those rays out listed apart,
                   and the mask form without its counts (one launch fewer).
  --interval LO HI the fractions of the segment (default 1e-4 0.9999)

Device entry points on buffers loaded beforehand.  The time of a call is rt_last_query_ms (HIP events around sort + walk +
resolve); the rays are written out by torch between two HIP events of its own.  Per comparison the forms ALTERNATE, call by
call, --warmup rounds untimed and then --reps rounds; a line holds the median, the minimum and the quartiles of a form's
times, so that the spread -- the run-to-run noise on a shared machine -- stands next to every difference.

    python3 tools/visibility_bench.py [--mesh meshes/bunny.off] [--pairs 1048576] [--grid 35290 32] [--grid 4096 4096]
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
from opencl_raytracer_amd.api import RT_QUERY_NO_SORT, _VisibilityArrays  # noqa: E402
from tools.meshes import bunny_path  # noqa: E402


def stats(ms) -> dict:
    q1, med, q3 = np.percentile(ms, [25, 50, 75])
    return {"median_ms": float(med), "min_ms": float(np.min(ms)), "q1_ms": float(q1), "q3_ms": float(q3), "max_ms": float(np.max(ms)),
            "spread": float((q3 - q1) / med) if med > 0 else 0.0}


def alternate(forms: dict, warmup: int, reps: int) -> dict:
    """forms: {name: call() -> ms}.  Round by round, every form once; the first `warmup` rounds are not kept."""
    times = {name: [] for name in forms}
    for round_ in range(warmup + reps):
        for name, call in forms.items():
            ms = call()
            if round_ >= warmup:
                times[name].append(ms)
    return {name: stats(ms) for name, ms in times.items()}


def main():
    import torch

    torch.zeros(1, device="cuda:0")  # torch's HIP runtime up BEFORE the library is loaded (as bench.py does)
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default=None, help="an OFF file (default: the bunny)")
    ap.add_argument("--pairs", type=int, default=1 << 20)
    ap.add_argument("--grid", type=int, nargs=2, action="append", metavar=("P", "T"))
    ap.add_argument("--interval", type=float, nargs=2, default=(1e-4, 1 - 1e-4), metavar=("LO", "HI"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "visibility_bench.jsonl"))
    args = ap.parse_args()
    if rt.device_count() < 1:
        sys.exit("visibility_bench: no HIP device visible (there is no CPU path to time)")
    grids = args.grid if args.grid is not None else [[35290, 32], [4096, 4096]]
    t_lo, t_hi = (float(x) for x in args.interval)
    lib = rt.load_library()
    dev = torch.device("cuda:0")
    mesh = args.mesh or bunny_path()
    scene = rt.Scene.load_off(mesh).build_bvh(0)
    host = rt.Host(rt.Options.defaults(width=64, height=48, n_super_samples=1), 0)
    host.upload_scene(scene)
    lo, hi = scene.aabbs[0, :3].astype(np.float64), scene.aabbs[1, :3].astype(np.float64)
    rng = np.random.default_rng(1)
    lines = []
    common = {"mesh": os.path.basename(mesh), "leaves": int(scene.num_faces), "t_lo": t_lo, "t_hi": t_hi, "reps": args.reps,
              "warmup": args.warmup}

    def emit(**kv):
        kv = {**common, **kv}
        print(json.dumps(kv), flush=True)
        lines.append(json.dumps(kv))

    def in_box(n):
        p4 = np.zeros((n, 4), np.float32)
        p4[:, :3] = lo + rng.random((n, 3)) * (hi - lo)
        return torch.from_numpy(p4).to(dev)

    def query_ms(rc):
        assert rc == 0, rc
        return host.last_query_ms

    if args.pairs > 0:
        n = args.pairs
        a, b = in_box(n), in_box(n)
        d = b - a  # (float32, one subtraction per component: the segment kernel's own)
        flag_s, flag_r = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        forms = {}
        for sort_name, flags in (("sorted", 0), ("unsorted", RT_QUERY_NO_SORT)):
            forms["segments_occluded " + sort_name] = lambda flags=flags: query_ms(lib.rt_segments_occluded_device(
                host._h, a.data_ptr(), b.data_ptr(), n, t_lo, t_hi, flags, flag_s.data_ptr(), None))
            forms["trace_occluded " + sort_name] = lambda flags=flags: query_ms(lib.rt_trace_occluded_device(
                host._h, a.data_ptr(), d.data_ptr(), n, t_hi, flags, flag_r.data_ptr(), None))
        got = alternate(forms, args.warmup, args.reps)
        torch.cuda.synchronize()
        for name, s in got.items():
            blocked = flag_s if name.startswith("segments") else flag_r
            emit(case="pairs", form=name, segments=n, msegments_per_s=n / s["median_ms"] / 1e3, blocked=int(blocked.sum().item()), **s)
        for sort_name in ("sorted", "unsorted"):
            emit(case="pairs", form="ratio " + sort_name, segments=n,
                 segments_over_trace=got["segments_occluded " + sort_name]["median_ms"] / got["trace_occluded " + sort_name]["median_ms"])
        del a, b, d, flag_s, flag_r

    for n_points, n_targets in grids:
        total = n_points * n_targets
        words = (n_targets + 31) // 32
        points, targets = in_box(n_points), in_box(n_targets)
        mask = torch.empty((n_points, words), dtype=torch.uint32, device=dev)
        count = torch.empty(n_points, dtype=torch.uint32, device=dev)
        out = _VisibilityArrays(mask.data_ptr(), count.data_ptr())
        mask_alone = _VisibilityArrays(mask.data_ptr(), None)  # (no resolve launch: what the counts cost)
        flag_r = torch.empty(total, dtype=torch.uint8, device=dev)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        rays = {}

        def write_rays():
            """The P x T rays written out, point by point: what a caller without the mask form has to do first."""
            start.record()
            rays["o"] = points[:, None, :].expand(n_points, n_targets, 4).reshape(total, 4).contiguous()
            rays["d"] = (targets[None, :, :] - points[:, None, :]).reshape(total, 4)
            stop.record()
            stop.synchronize()
            return start.elapsed_time(stop)

        write_rays()
        torch.cuda.synchronize()
        forms = {"write_rays": write_rays}
        for sort_name, flags in (("sorted", 0), ("unsorted", RT_QUERY_NO_SORT)):
            forms["visibility_masks " + sort_name] = lambda flags=flags: query_ms(lib.rt_visibility_masks_device(
                host._h, points.data_ptr(), n_points, targets.data_ptr(), n_targets, t_lo, t_hi, flags, C.byref(out), None))
            forms["visibility_masks, mask alone " + sort_name] = lambda flags=flags: query_ms(lib.rt_visibility_masks_device(
                host._h, points.data_ptr(), n_points, targets.data_ptr(), n_targets, t_lo, t_hi, flags, C.byref(mask_alone), None))
            forms["trace_occluded on written rays " + sort_name] = lambda flags=flags: query_ms(lib.rt_trace_occluded_device(
                host._h, rays["o"].data_ptr(), rays["d"].data_ptr(), total, t_hi, flags, flag_r.data_ptr(), None))
        got = alternate(forms, args.warmup, args.reps)
        torch.cuda.synchronize()
        ray_bytes = 2 * 16 * total
        for name, s in got.items():
            extra = {}
            if name == "write_rays":
                extra = {"ray_bytes": ray_bytes, "input_bytes": 16 * (n_points + n_targets)}
            elif name.startswith("visibility"):
                extra = {"msegments_per_s": total / s["median_ms"] / 1e3, "blocked": int(count.view(torch.int32).sum(dtype=torch.int64).item()),
                         "output_bytes": 4 * n_points * (words + 1)}
            else:
                extra = {"msegments_per_s": total / s["median_ms"] / 1e3, "blocked": int(flag_r.sum(dtype=torch.int64).item()), "output_bytes": total}
            emit(case="grid", form=name, points=n_points, targets=n_targets, segments=total, **extra, **s)
        for sort_name in ("sorted", "unsorted"):
            walk = got["trace_occluded on written rays " + sort_name]["median_ms"]
            emit(case="grid", form="ratio " + sort_name, points=n_points, targets=n_targets, segments=total,
                 mask_over_walk_alone=got["visibility_masks " + sort_name]["median_ms"] / walk,
                 mask_over_write_plus_walk=got["visibility_masks " + sort_name]["median_ms"] / (walk + got["write_rays"]["median_ms"]))
        del points, targets, mask, count, flag_r, rays

    host.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
