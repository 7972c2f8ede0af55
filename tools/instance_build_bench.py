#!/usr/bin/env python3
"""Device-side instance sets (include/rt_hip_instance_build.h) on the bunny: one JSON line per measurement, appended to
profiles/instance_build_bench.jsonl (the first line of a run is its invocation).

  (s) a step with the poses in a DEVICE tensor, n = 1000, 32768 and 2^20 instances, wall clock around the step, by two routes,
      each in a child process of its own:
        today  tensor.cpu().numpy() and host.set_instances(...): the download, the host planner, three uploads -- run from a
               built checkout of the PARENT commit (--parent-tree), whose code this is;
        built  host.build_instances(tensor): kernels and one 36-byte read (and rt_last_instance_build_ms, the launches alone)
  (b), (c) tools/instances_bench.py's grid sets -- 10 x 10 x 10 bunnies, 1 M camera-like rays, 1 M random rays -- on BOTH
      trees, set_instances's median split and build_instances's radix tree, alternating call by call
  (f) with --parent-tree: `python bench.py --gpus 1 --steps 200 --warmup 20` there and here, alternating, --frame-rounds
      times each, every run a child process, before this process opens the device

Median, minimum and spread (max - min) / median of --reps steps or calls after --warmup.

    python3 tools/instance_build_bench.py [--reps 20] [--warmup 3] [--sizes 1000,32768,1048576] [--sets sbc] [--parent-tree DIR]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "instance_build_bench.jsonl")


def emit(**kv):
    line = json.dumps(kv)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def stats(ms):
    ms = np.asarray(ms, np.float64)
    med = float(np.median(ms))
    return {"median_ms": med, "min_ms": float(ms.min()), "spread": float((ms.max() - ms.min()) / med)}


def rigid_poses(lo, hi, n, rng):
    """n rotated copies scattered over a cube that grows with n: float32 (n, 3, 4), rotations from unit quaternions."""
    centre, side = (lo + hi) / 2, max(1.0, float(n) ** (1.0 / 3.0)) * float((hi - lo).max()) * 1.5
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    A = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], axis=1),
                  np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], axis=1),
                  np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)
    W = np.zeros((n, 3, 4))
    W[:, :, :3] = A
    W[:, :, 3] = centre - A @ centre + (rng.random((n, 3)) - 0.5) * side
    return np.ascontiguousarray(W, np.float32)


def child(route, tree, sizes, reps, warmup):
    """One route's steps on the build of `tree`; prints one JSON line per size."""
    sys.path[:0] = [tree, os.path.join(tree, "tests")]
    import torch

    torch.zeros(1, device="cuda:0")  # torch's HIP runtime up BEFORE the library is loaded (as bench.py does)
    import opencl_raytracer_amd as rt
    from tools.meshes import bunny_path

    scene = rt.Scene.load_off(bunny_path()).build_bvh(0)
    host = rt.Host(rt.Options.defaults(width=64, height=48, n_super_samples=1), 0)
    host.upload_scene(scene)
    lo, hi = scene.aabbs[0, :3].astype(np.float64), scene.aabbs[1, :3].astype(np.float64)
    rng = np.random.default_rng(3)
    for n in sizes:
        tensors = [torch.from_numpy(rigid_poses(lo, hi, n, rng)).to("cuda:0") for _ in range(2)]  # (new poses every step, in turn)
        torch.cuda.synchronize()
        wall, launches = [], []
        for step in range(warmup + reps):
            t = tensors[step % 2]
            t0 = time.perf_counter()
            if route == "today":
                host.set_instances(t.cpu().numpy())
            else:
                host.build_instances(t)
            t1 = time.perf_counter()
            if step >= warmup:
                wall.append((t1 - t0) * 1e3)
                if route == "built":
                    launches.append(host.last_instance_build_ms())
        line = {"set": "s_step", "route": route, "instances": n, "reps": reps, "step_wall": stats(wall)}
        if launches:
            line["planning_launches"] = stats(launches)
        print(json.dumps(line), flush=True)
    host.close()


def steps(parent_tree, sizes, reps, warmup):
    for route, tree in (("today", os.path.abspath(parent_tree) if parent_tree else None), ("built", ROOT)):
        if tree is None:
            emit(set="s_step", route=route, skipped="no --parent-tree: today's route is measured on the parent's build")
            continue
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", route, "--tree", tree, "--sizes", ",".join(map(str, sizes)),
                              "--reps", str(reps), "--warmup", str(warmup)], capture_output=True, text=True, timeout=1500)
        if run.returncode != 0:
            raise SystemExit(f"the {route} route failed on {tree}:\n{run.stdout[-1000:]}\n{run.stderr[-3000:]}")
        for line in run.stdout.strip().splitlines():
            if line.startswith("{"):
                emit(tree="parent" if route == "today" else "branch", **json.loads(line))


def frames(parent_tree, rounds):
    """(f): bench.py's headline on the parent's build and on this one, alternating."""
    for r in range(1, rounds + 1):
        for side, tree in (("parent", os.path.abspath(parent_tree)), ("branch", ROOT)):
            run = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "200", "--warmup", "20"], cwd=tree,
                                 capture_output=True, text=True, timeout=300)
            if run.returncode != 0:
                raise SystemExit(f"bench.py failed in {tree}:\n{run.stderr[-2000:]}")
            res = json.loads(run.stdout.strip().splitlines()[-1])
            emit(set="frames_bench_py", side=side, round=r, value=res["value"], unit=res["unit"], ms_per_step=res["ms_per_step"],
                 steps=res["steps"], warmup=res["warmup"])


def queries(args):
    """(b), (c): the grid's rays on both trees."""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch

    torch.zeros(1, device="cuda:0")
    import opencl_raytracer_amd as rt
    from tools.instances_bench import camera_like, poses, random_rays
    from tools.meshes import bunny_path

    dev = torch.device("cuda:0")
    scene = rt.Scene.load_off(bunny_path()).build_bvh(0)
    host = rt.Host(rt.Options.defaults(width=64, height=48, n_super_samples=1), 0)
    host.upload_scene(scene)
    rng = np.random.default_rng(1)
    W = poses(scene, 10, rng)
    host.set_instances(W)
    nodes = host.instances()["nodes"]
    cases = []
    if "b" in args.sets:
        cases.append(("b_grid_camera_like", camera_like(nodes, 1024, rng)))
    if "c" in args.sets:
        cases.append(("c_grid_random", random_rays(nodes["lo"][0].astype(np.float64), nodes["hi"][0].astype(np.float64), args.random, rng)))
    trees = (("median_split", lambda: host.set_instances(W)), ("lbvh", lambda: host.build_instances(W)))
    for name, (o4, d4) in cases:
        to, td = torch.from_numpy(o4).to(dev), torch.from_numpy(d4).to(dev)
        for form in ("closest", "occluded"):
            call = (lambda: host.trace_instances_closest(to, td)) if form == "closest" else (lambda: host.trace_instances_occluded(to, td))
            ms = {tree: [] for tree, _ in trees}
            for rep in range(args.warmup + args.reps):  # alternating, so that a drift of the clock hits both alike
                for tree, make in trees:
                    make()
                    call()
                    if rep >= args.warmup:
                        ms[tree].append(host.last_query_ms)
            ratios = np.asarray(ms["lbvh"]) / np.asarray(ms["median_split"])
            emit(set=name, form=form, instances=len(W), rays=len(o4), median_split=stats(ms["median_split"]), lbvh=stats(ms["lbvh"]),
                 ratio_median=float(np.median(ratios)), ratio_min=float(ratios.min()), ratio_max=float(ratios.max()))
        del to, td
    host.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="1000,32768,1048576")
    ap.add_argument("--random", type=int, default=1 << 20)
    ap.add_argument("--sets", default="sbc")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: today's route and (f)")
    ap.add_argument("--frame-rounds", type=int, default=4)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",") if s]
    if args.child:
        child(args.child, args.tree, sizes, args.reps, args.warmup)
        return
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    emit(set="invocation", argv=sys.argv[1:], reps=args.reps, warmup=args.warmup, sizes=sizes, random=args.random, sets=args.sets)
    if args.parent_tree and args.frame_rounds > 0:
        frames(args.parent_tree, args.frame_rounds)
    if "s" in args.sets:
        steps(args.parent_tree, sizes, args.reps, args.warmup)
    if set("bc") & set(args.sets):
        queries(args)


if __name__ == "__main__":
    main()
