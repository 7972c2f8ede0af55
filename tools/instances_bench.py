#!/usr/bin/env python3
"""Instanced ray queries on the bunny (include/rt_hip_instances.h): one JSON line per measurement, appended to
profiles/instances_bench.jsonl.

  (a) ONE identity instance against rt_trace_closest / rt_trace_occluded on the same rays in the same run, the two
      alternating call by call: the 1920x1080 reference camera rays and uniformly random rays in the scene box (the rays of
      tools/query_bench.py's sets (a) and (c)).  ratio = instanced / plain: what the top level costs where it buys nothing.
  (b) a 10 x 10 x 10 grid of translated and rotated bunnies, 1 M camera-like rays (a pinhole outside the grid, looking at its
      centre): both forms, sorted and unsorted
  (c) the same grid, 1 M uniformly random rays with origins in the top-level root box
  (d) 1000 instances given new poses every step, 100 steps: the host's wall time in set_instances (inverses, tree, upload)
      per step, the query's device time, and the share of a step the host spends in set_instances
  (f) with --parent-tree DIR (a built checkout of the commit before): `python bench.py --gpus 1 --steps 200 --warmup 20` there
      and here, alternating, --frame-rounds times each, every run a child process of its own, before this process opens the
      device; one "frames_bench_py" line per run

Device tensors on the host's stream; the time of a call is rt_last_query_ms (HIP events around sort + walk) after warm-up
calls: median, minimum and the spread (max - min) / median of --reps calls.

    python3 tools/instances_bench.py [--reps 20] [--warmup 3] [--random 1048576] [--sets abcd] [--parent-tree DIR]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import opencl_raytracer_amd as rt  # noqa: E402
import orc  # noqa: E402
import query_oracle as qo  # noqa: E402
from tools.meshes import bunny_path  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "instances_bench.jsonl")


def emit(**kv):
    line = json.dumps(kv)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def stats(ms):
    ms = np.asarray(ms, np.float64)
    med = float(np.median(ms))
    return {"median_ms": med, "min_ms": float(ms.min()), "spread": float((ms.max() - ms.min()) / med)}


def rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))[None, :]
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def poses(scene, per_axis, rng, spacing=1.5):
    """per_axis^3 bunnies on a grid, each turned about its box centre: float32 (n, 3, 4)."""
    lo, hi = scene.aabbs[0, :3].astype(np.float64), scene.aabbs[1, :3].astype(np.float64)
    centre, step = (lo + hi) / 2, float((hi - lo).max()) * spacing
    W = np.zeros((per_axis ** 3, 3, 4))
    k = 0
    for i in range(per_axis):
        for j in range(per_axis):
            for l in range(per_axis):
                A = rotation(rng)
                W[k, :, :3] = A
                W[k, :, 3] = centre - A @ centre + (np.array([i, j, l]) - (per_axis - 1) / 2) * step
                k += 1
    return np.ascontiguousarray(W, np.float32)


def camera_like(nodes, side, rng):
    """side x side pinhole rays from outside the top-level root box towards its centre: (n, 4) float32 each."""
    lo, hi = nodes["lo"][0].astype(np.float64), nodes["hi"][0].astype(np.float64)
    centre, radius = (lo + hi) / 2, float(np.linalg.norm(hi - lo)) / 2
    eye = centre + np.array([0.3, 0.4, 1.0]) / np.linalg.norm([0.3, 0.4, 1.0]) * radius * 1.6
    forward = (centre - eye) / np.linalg.norm(centre - eye)
    right = np.cross(forward, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, forward)
    u = (np.arange(side) + 0.5) / side - 0.5
    d = forward[None, None, :] + 1.2 * (u[None, :, None] * right[None, None, :] - u[:, None, None] * up[None, None, :])
    d = (d / np.linalg.norm(d, axis=2, keepdims=True)).reshape(-1, 3)
    o4, d4 = np.zeros((side * side, 4), np.float32), np.zeros((side * side, 4), np.float32)
    o4[:, :3], d4[:, :3] = eye, d
    return o4, d4


def random_rays(lo, hi, n, rng):
    o4, d4 = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    o4[:, :3] = lo + rng.random((n, 3)) * (hi - lo)
    d = rng.normal(size=(n, 3))
    d4[:, :3] = d / np.linalg.norm(d, axis=1, keepdims=True)
    return o4, d4


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--random", type=int, default=1 << 20)
    ap.add_argument("--sets", default="abcd")
    ap.add_argument("--parent-tree", default=None, help="(f) a built checkout of the parent commit")
    ap.add_argument("--frame-rounds", type=int, default=4)
    args = ap.parse_args()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    emit(set="invocation", argv=sys.argv[1:], reps=args.reps, warmup=args.warmup, random=args.random, sets=args.sets)
    if args.parent_tree:
        frames(args.parent_tree, args.frame_rounds)
    import torch

    torch.zeros(1, device="cuda:0")  # torch's HIP runtime up BEFORE the library is loaded (as bench.py does)
    dev = torch.device("cuda:0")
    scene = rt.Scene.load_off(bunny_path()).build_bvh(0)
    opt = rt.Options.defaults(width=1920, height=1080, n_super_samples=1)
    host = rt.Host(opt, 0)
    host.upload_scene(scene)
    rng = np.random.default_rng(1)

    def on_device(o4, d4):
        return torch.from_numpy(o4).to(dev), torch.from_numpy(d4).to(dev)

    def run(call, reps=None):
        for _ in range(args.warmup):
            call()
        ms = []
        for _ in range(reps or args.reps):
            call()
            ms.append(host.last_query_ms)
        return ms

    if "a" in args.sets:
        host.set_instances(np.eye(3, 4, dtype=np.float32)[None])
        lo, hi = scene.aabbs[0, :3].astype(np.float64), scene.aabbs[1, :3].astype(np.float64)
        for name, (o4, d4) in (("camera", qo.camera_rays(orc.params_from_options(opt))), ("random", random_rays(lo, hi, args.random, rng))):
            to, td = on_device(o4, d4)
            for form in ("closest", "occluded"):
                plain = (lambda: host.trace_closest(to, td)) if form == "closest" else (lambda: host.trace_occluded(to, td))
                inst = (lambda: host.trace_instances_closest(to, td)) if form == "closest" else (lambda: host.trace_instances_occluded(to, td))
                for _ in range(args.warmup):
                    plain(), inst()
                p_ms, i_ms = [], []
                for _ in range(args.reps):  # alternating, so that a drift of the clock hits both alike
                    plain()
                    p_ms.append(host.last_query_ms)
                    inst()
                    i_ms.append(host.last_query_ms)
                ratios = np.asarray(i_ms) / np.asarray(p_ms)
                emit(set="a_identity", rays_from=name, form=form, rays=len(o4), plain=stats(p_ms), instanced=stats(i_ms),
                     ratio_median=float(np.median(ratios)), ratio_min=float(ratios.min()), ratio_max=float(ratios.max()))
            del to, td

    if set("bc") & set(args.sets):
        W = poses(scene, 10, rng)
        t0 = time.perf_counter()
        host.set_instances(W)
        set_ms = (time.perf_counter() - t0) * 1e3
        nodes = host.instances()["nodes"]
        emit(set="grid", instances=len(W), set_instances_wall_ms=set_ms)
        cases = []
        if "b" in args.sets:
            cases.append(("b_grid_camera_like", camera_like(nodes, 1024, rng)))
        if "c" in args.sets:
            cases.append(("c_grid_random", random_rays(nodes["lo"][0].astype(np.float64), nodes["hi"][0].astype(np.float64), args.random, rng)))
        for name, (o4, d4) in cases:
            to, td = on_device(o4, d4)
            for form in ("closest", "occluded"):
                for sort in (True, False):
                    if form == "closest":
                        ms = run(lambda: host.trace_instances_closest(to, td, sort=sort))
                        share = float(host.trace_instances_closest(to, td, outputs=("hit",))["hit"].float().mean())
                    else:
                        ms = run(lambda: host.trace_instances_occluded(to, td, sort=sort))
                        share = float(host.trace_instances_occluded(to, td).float().mean())
                    s = stats(ms)
                    emit(set=name, form=form, order="sorted" if sort else "unsorted", instances=len(W), rays=len(o4), hit_share=share,
                         mrays_per_s=len(o4) / s["median_ms"] / 1e3, **s)
            del to, td

    if "d" in args.sets:
        steps, per_axis = 100, 10
        o4, d4 = None, None
        set_ms, query_ms, wall_ms = [], [], []
        for step in range(steps + args.warmup):
            W = poses(scene, per_axis, rng)  # (new poses: not part of the step's time)
            t0 = time.perf_counter()
            host.set_instances(W)
            t1 = time.perf_counter()
            if o4 is None:
                o4, d4 = camera_like(host.instances()["nodes"], 512, rng)
                to, td = on_device(o4, d4)
                t1 = time.perf_counter()
            host.trace_instances_closest(to, td)
            q = host.last_query_ms  # (waits for the query)
            t2 = time.perf_counter()
            if step >= args.warmup:
                set_ms.append((t1 - t0) * 1e3)
                query_ms.append(q)
                wall_ms.append((t2 - t0) * 1e3)
        emit(set="d_moving", instances=per_axis ** 3, steps=steps, rays=len(o4), set_instances_wall=stats(set_ms), query=stats(query_ms),
             step_wall=stats(wall_ms), host_share_in_set_instances=float(np.median(np.asarray(set_ms) / np.asarray(wall_ms))))
    host.close()


if __name__ == "__main__":
    main()
