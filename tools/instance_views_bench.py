#!/usr/bin/env python3
"""Instanced views and instanced ambient occlusion on the bunny (include/rt_hip_instance_views.h): one JSON line per
measurement, appended to profiles/instance_views_bench.jsonl (--out); the first line of a run is its invocation.

Bunny, 1920x1080, -s 1 -a 3 (bench.py's ambient-occlusion options), device outputs on pre-allocated tensors; the time of a
call is rt_last_query_ms (HIP events around everything the call enqueues, the waits for the chunks' hit counts included)
after --warmup calls: median, minimum and the spread (max - min) / median of --reps calls.

  (a) the top level's cost: ONE identity instance, the eight orbit poses of tools/views_bench.py in one call, ("value",);
      rt_render_instance_views_device against rt_render_views_device on the same host, the two alternating call by call.
      ratio = instanced / plain, with its range.  Reported, not gated.
  (b) the case the feature exists for: a 10 x 10 x 10 grid of turned bunnies (tools/instances_bench.py's), eight poses on an
      orbit around the grid, ("value", "image"): ms per view, and rays per second over the camera rays plus the
      ambient-occlusion rays the call cast (rt_debug_last_views' points x rays per point).  The split into the ray kernel
      and the ambient-occlusion step comes from a kernel trace of `--sets b --reps 3` in a run of its own.
  (c) instanced ambient occlusion at --points points on the grid's surfaces (hit points of camera-like and random rays with
      their normals, in the rays' order), sorted and unsorted.
  (d) with --parent-tree DIR (a built checkout of the commit before): nothing existing moved.  bench.py, tools/views_bench.py
      and sets (a) and (b) of tools/instances_bench.py there and here, alternating, --rounds times each, every run a child
      process of its own, before this process opens the device.  Per metric: the parent's values, this tree's, and whether
      this tree's median lies inside the range the parent's runs span -- as it is, widened by its own width, and widened by
      the spread the parent's calls show within one run.

    python3 tools/instance_views_bench.py [--reps 20] [--warmup 3] [--points 1048576] [--sets abc] [--parent-tree DIR] [--rounds 4]
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

OUT = os.path.join(ROOT, "profiles", "instance_views_bench.jsonl")


def emit(out, **kv):
    line = json.dumps(kv)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def stats(ms):
    ms = np.asarray(ms, np.float64)
    med = float(np.median(ms))
    return {"median_ms": med, "min_ms": float(ms.min()), "max_ms": float(ms.max()), "spread": float((ms.max() - ms.min()) / med)}


def json_lines(text):
    out = []
    for line in text.splitlines():
        if line.startswith("{"):
            try:
                out.append(json.loads(line))
            except ValueError:
                pass
    return out


def nothing_moved(args):
    """(d): the three existing measurements on the parent's build and on this one, alternating."""
    trees = (("parent", os.path.abspath(args.parent_tree)), ("branch", ROOT))
    scratch = os.path.join(os.path.dirname(os.path.abspath(args.out)), "instance_views_bench_d")
    os.makedirs(scratch, exist_ok=True)
    values, spreads = {}, {}  # per (metric, side): the runs' medians; the runs' own call-to-call spreads, where a run reports one
    runs = args.d_runs.split(",")

    def child(tree, argv, what):
        run = subprocess.run([sys.executable] + argv, cwd=tree, capture_output=True, text=True, timeout=900)
        if run.returncode != 0:
            raise SystemExit(f"{what} failed in {tree}:\n{run.stdout[-1500:]}\n{run.stderr[-2500:]}")
        return json_lines(run.stdout)

    for r in range(1, args.rounds + 1):
        for side, tree in trees if "bench" in runs else ():
            res = child(tree, ["bench.py", "--gpus", "1", "--steps", "200", "--warmup", "20"], "bench.py")[-1]
            values.setdefault(("bench_py_ms_per_step", side), []).append(res["ms_per_step"])
            emit(args.out, set="d_bench_py", side=side, round=r, value=res["value"], unit=res["unit"], ms_per_step=res["ms_per_step"])
        for side, tree in trees if "views" in runs else ():
            rows = child(tree, ["tools/views_bench.py", "--rounds", "1", "--reps", str(args.reps), "--warmup", "5", "--out",
                                os.path.join(scratch, f"views_{side}_{r}.jsonl")], "views_bench.py")
            for row in rows:
                if row.get("what") == "render_views" and row.get("views") == 8:
                    values.setdefault((f"views_bench_v8_{row['outputs']}_ms", side), []).append(row["median_ms"])
                    spreads.setdefault((f"views_bench_v8_{row['outputs']}_ms", side), []).append((row["max_ms"] - row["min_ms"]) / row["median_ms"])
                    emit(args.out, set="d_views_bench", side=side, round=r, outputs=row["outputs"], views=8, median_ms=row["median_ms"],
                         min_ms=row["min_ms"], max_ms=row["max_ms"])
        for side, tree in trees if "instances" in runs else ():
            rows = child(tree, ["tools/instances_bench.py", "--sets", "ab", "--reps", str(args.reps), "--warmup", str(args.warmup)],
                         "instances_bench.py")
            for row in rows:
                if row.get("set") == "a_identity":
                    key = f"instances_bench_a_{row['rays_from']}_{row['form']}_instanced_ms"
                    med, spread = row["instanced"]["median_ms"], row["instanced"]["spread"]
                elif row.get("set") == "b_grid_camera_like":
                    key = f"instances_bench_b_{row['form']}_{row['order']}_ms"
                    med, spread = row["median_ms"], row["spread"]
                else:
                    continue
                values.setdefault((key, side), []).append(med)
                spreads.setdefault((key, side), []).append(spread)
                emit(args.out, set="d_instances_bench", side=side, round=r, metric=key, median_ms=med, spread=spread)
    inside_all = True
    for metric in sorted({m for m, _ in values}):
        parent, branch = np.asarray(values[(metric, "parent")]), np.asarray(values[(metric, "branch")])
        width = float(parent.max() - parent.min())
        median = float(np.median(branch))
        inside = bool(parent.min() <= median <= parent.max())
        widened = bool(parent.min() - width <= median <= parent.max() + width)
        # ... and by the spread the parent's calls show WITHIN a run, (max - min) / median of its timed calls, where the runs say it
        within = float(np.median(spreads[(metric, "parent")])) if (metric, "parent") in spreads else None
        by_calls = None if within is None else bool(parent.min() - within * np.median(parent) <= median <= parent.max() + within * np.median(parent))
        inside_all = inside_all and (widened or bool(by_calls))
        emit(args.out, set="d_verdict", metric=metric, parent=parent.tolist(), branch=branch.tolist(), branch_median=median,
             parent_median=float(np.median(parent)), inside_parent_range=inside, inside_range_widened_by_parent_range=widened,
             parent_spread_within_a_run=within, inside_range_widened_by_parent_spread_within_a_run=by_calls)
    emit(args.out, set="d_nothing_moved", every_median_inside_the_widened_parent_range=inside_all, rounds=args.rounds, runs=runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--sets", default="abc")
    ap.add_argument("--parent-tree", default=None, help="(d) a built checkout of the parent commit")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--d-runs", default="bench,views,instances", help="(d) which of the three existing measurements to repeat")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    emit(args.out, set="invocation", argv=sys.argv[1:], reps=args.reps, warmup=args.warmup, points=args.points, sets=args.sets,
         width=args.width, height=args.height)
    if args.parent_tree:
        nothing_moved(args)
    if not set("abc") & set(args.sets):
        return
    import torch

    torch.zeros(1, device="cuda:0")  # torch's HIP runtime up BEFORE the library is loaded (as bench.py does)
    import opencl_raytracer_amd as rt
    from opencl_raytracer_amd.api import _InstanceViewArrays, _LayerArrays, _ViewArrays
    from tools.instances_bench import camera_like, poses, random_rays
    from tools.meshes import bunny_path

    dev = torch.device("cuda:0")
    lib = rt.load_library()
    scene = rt.Scene.load_off(bunny_path()).build_bvh(0)
    opt = rt.Options.defaults(width=args.width, height=args.height, n_super_samples=1, ao_num_samples=3)
    host = rt.Host(opt, 0)
    host.upload_scene(scene)
    n = opt.total_width * opt.total_height
    per_point = host.ao_rays_per_point[0]
    rng = np.random.default_rng(1)
    value = torch.empty((8, opt.total_height, opt.total_width), dtype=torch.float32, device=dev)
    image = torch.empty((8, opt.height, opt.width), dtype=torch.uint8, device=dev)

    def view_calls(cameras, with_image):
        plain = _ViewArrays(_LayerArrays(value=value.data_ptr()), image.data_ptr() if with_image else None)
        inst = _InstanceViewArrays(plain, None)
        return (lambda: lib.rt_render_views_device(host._h, cameras.ctypes.data, len(cameras), C.byref(plain), None),
                lambda: lib.rt_render_instance_views_device(host._h, cameras.ctypes.data, len(cameras), C.byref(inst), None))

    def orbit(centre, radius, lift):
        out = []
        for k in range(8):
            a = 2 * np.pi * k / 8
            eye = (centre[0] + radius * np.sin(a), centre[1] + lift, centre[2] + radius * np.cos(a))
            out.append(rt.Camera.look_at(eye, tuple(float(c) for c in centre)).as_array())
        return np.ascontiguousarray(np.stack(out), np.float32)

    if "a" in args.sets:
        host.set_instances(np.eye(3, 4, dtype=np.float32)[None])
        cameras = orbit((0.0, 0.0, 0.0), 2.0, 0.4)  # (tools/views_bench.py's poses)
        plain, inst = view_calls(cameras, False)
        for _ in range(args.warmup):
            assert plain() == 0 and inst() == 0
        p_ms, i_ms = [], []
        for _ in range(args.reps):  # alternating, so that a drift of the clock hits both alike
            assert plain() == 0
            p_ms.append(host.last_query_ms)
            points_plain = host.last_views()["ao_points"]
            assert inst() == 0
            i_ms.append(host.last_query_ms)
        ratios = np.asarray(i_ms) / np.asarray(p_ms)
        done = host.last_views()
        emit(args.out, set="a_identity_views", views=8, outputs="value", sub_pixels=8 * n, ao_points=done["ao_points"],
             ao_points_plain=points_plain, plain=stats(p_ms), instanced=stats(i_ms), ratio_median=float(np.median(ratios)),
             ratio_min=float(ratios.min()), ratio_max=float(ratios.max()))

    if set("bc") & set(args.sets):
        W = poses(scene, 10, rng)
        host.set_instances(W)
        nodes = host.instances()["nodes"]
        lo, hi = nodes["lo"][0].astype(np.float64), nodes["hi"][0].astype(np.float64)
        centre, radius = (lo + hi) / 2, float(np.linalg.norm(hi - lo)) / 2

    if "b" in args.sets:
        cameras = orbit(centre, radius * 1.6, radius * 0.5)
        _, inst = view_calls(cameras, True)
        for _ in range(args.warmup):
            assert inst() == 0
        ms = []
        for _ in range(args.reps):
            assert inst() == 0
            ms.append(host.last_query_ms)
        done, s = host.last_views(), stats(ms)
        rays = 8 * n + done["ao_points"] * per_point
        emit(args.out, set="b_grid_views", instances=len(W), views=8, outputs="value,image", sub_pixels=8 * n, ao_points=done["ao_points"],
             chunks=done["chunks"], hit_share=done["ao_points"] / (8 * n), rays=rays, ms_per_view=s["median_ms"] / 8,
             mrays_per_s=rays / s["median_ms"] / 1e3, **s)

    if "c" in args.sets:
        side = int(np.ceil(np.sqrt(args.points / 0.3)))  # (about four camera-like rays in ten hit a copy)
        got = []
        for o4, d4 in (camera_like(nodes, side, rng), random_rays(lo, hi, args.points, rng)):
            to, td = torch.from_numpy(o4).to(dev), torch.from_numpy(d4).to(dev)
            rec = host.trace_instances_closest(to, td, outputs=("hit", "distance", "position", "normal"))
            at = rec["hit"].bool() & torch.isfinite(rec["distance"])
            got.append((rec["position"][at], rec["normal"][at]))
            del to, td, rec
        points = torch.cat([g[0] for g in got])[:args.points].contiguous()
        normals = torch.cat([g[1] for g in got])[:args.points].contiguous()
        m = int(points.shape[0])
        ao = torch.empty(m, dtype=torch.float32, device=dev)
        p4, n4 = torch.nn.functional.pad(points, (0, 1)).contiguous(), torch.nn.functional.pad(normals, (0, 1)).contiguous()
        torch.cuda.synchronize()
        for sort in (True, False):
            call = lambda: lib.rt_trace_instances_ao_device(host._h, p4.data_ptr(), n4.data_ptr(), None, m, 0 if sort else 1, ao.data_ptr(),
                                                            None, None)
            for _ in range(args.warmup):
                assert call() == 0
            ms = []
            for _ in range(args.reps):
                assert call() == 0
                ms.append(host.last_query_ms)
            s = stats(ms)
            emit(args.out, set="c_grid_ao_points", instances=len(W), points=m, rays=m * per_point, order="sorted" if sort else "unsorted",
                 mean_ao=float(ao.mean()), mrays_per_s=m * per_point / s["median_ms"] / 1e3, **s)
    host.close()


if __name__ == "__main__":
    main()
