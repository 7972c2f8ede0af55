#!/usr/bin/env python3
"""Instanced multi-hit and instanced directional occlusion queries on the bunny (include/rt_hip_instance_multihit.h,
include/rt_hip_instance_directional.h): one JSON line per measurement, appended to profiles/instance_multihit_bench.jsonl,
the invocation first.

  (a) ONE identity instance against the plain query on the same inputs in the same run, the two alternating call by call:
      trace_instances_multihit against trace_multihit (k = 4, 16 and the count alone) on the 1920x1080 reference camera rays
      and on uniformly random rays in the scene box; instances_directional_occlusion against directional_occlusion on the
      camera's hit points.  ratio = instanced / plain: what the top level costs where it buys nothing.  (The plain kernels
      of this build are the parent's instruction for instruction; with --parent-tree DIR the plain side is measured once
      more by a child process on the parent's own library, for the record: "a_parent_plain".)
  (b) a 10 x 10 x 10 grid of translated and rotated bunnies (tools/instances_bench.py's), 1 M camera-like rays and 1 M
      uniformly random rays: multi-hit with k = 4, 16 and the count alone, sorted and unsorted
  (c) instanced masks against what the library allowed before: ao_rays + trace_instances_occluded on the written rays + the
      packing of the flags (torch, on the device), on the grid, at points on its surfaces; the three steps' device times
      (rt_last_query_ms each; the packing by torch's events) are summed.  ratio = masks / written-out
  (f) with --parent-tree DIR: `python bench.py --gpus 1 --steps 200 --warmup 20` there and here, alternating, --frame-rounds
      times each, every run a child process of its own, before this process opens the device

Device tensors on ONE torch stream of the tool's own, which the library is handed for every call (the host's own stream is
a non-blocking one: under torch's default stream, whose handle is NULL, the library would enqueue on the host's stream, in no
order with torch's own kernels -- the padding of (N, 3) inputs, the gather of the hit points -- and a query whose inputs change
while it runs may read anything); every call is waited for before the next (rt_last_query_ms).  The time of a call is
rt_last_query_ms (HIP events around sort + walk + resolve) after warm-up calls: median, minimum and the spread (max - min) /
median of --reps calls.

    python3 tools/instance_multihit_bench.py [--reps 20] [--warmup 3] [--random 1048576] [--sets abc] [--parent-tree DIR]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import opencl_raytracer_amd as rt  # noqa: E402
import orc  # noqa: E402
import query_oracle as qo  # noqa: E402
from tools.instances_bench import camera_like, poses, random_rays, stats  # noqa: E402
from tools.meshes import bunny_path  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "instance_multihit_bench.jsonl")
KS = (4, 16, 0)  # (0: the count alone)
AO = dict(ao_num_samples=3, ao_max_distance=0.2)  # 28 rays a point, the frame's own reach

# The plain side of (a) on another build of the library: run with that tree as the working directory.
PARENT_PLAIN = r"""
import json, sys
import numpy as np
import torch
torch.zeros(1, device="cuda:0")
sys.path[:0] = [".", "tests"]
import opencl_raytracer_amd as rt, orc, query_oracle as qo
from tools.meshes import bunny_path
reps, warmup = int(sys.argv[1]), int(sys.argv[2])
opt = rt.Options.defaults(width=1920, height=1080, n_super_samples=1, ao_num_samples=3, ao_max_distance=0.2)
host = rt.Host(opt, 0)
host.upload_scene(rt.Scene.load_off(bunny_path()).build_bvh(0))
o4, d4 = qo.camera_rays(orc.params_from_options(opt))
side = torch.cuda.Stream(device="cuda:0")
def run(call):
    ms = []
    for i in range(warmup + reps):
        call()
        t = host.last_query_ms
        if i >= warmup:
            ms.append(t)
    return ms
out = {}
with torch.cuda.stream(side):
    to, td = torch.from_numpy(o4).to("cuda:0"), torch.from_numpy(d4).to("cuda:0")
    side.synchronize()
    for k in (4, 16, 0):
        outputs = rt.api.MULTIHIT_OUTPUTS if k else ("count",)
        out["multihit_k%d" % k] = run(lambda: host.trace_multihit(to, td, k=k, outputs=outputs))
    near = host.trace_closest(to, td, outputs=("hit", "position", "normal"))
    side.synchronize()
    hit = near["hit"].bool()
    p = torch.nn.functional.pad(near["position"][hit], (0, 1)).contiguous()
    q = torch.nn.functional.pad(near["normal"][hit], (0, 1)).contiguous()
    side.synchronize()
    out["directional"] = run(lambda: host.directional_occlusion(p, q))
    out["points"] = int(p.shape[0])
    side.synchronize()
host.close()
print(json.dumps(out))
"""


def emit(**kv):
    line = json.dumps(kv)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


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


def parent_plain(parent_tree, reps, warmup):
    run = subprocess.run([sys.executable, "-c", PARENT_PLAIN, str(reps), str(warmup)], cwd=os.path.abspath(parent_tree),
                         capture_output=True, text=True, timeout=600)
    if run.returncode != 0:
        raise SystemExit(f"the plain side failed in {parent_tree}:\n{run.stderr[-2000:]}")
    res = json.loads(run.stdout.strip().splitlines()[-1])
    for name, ms in res.items():
        if name != "points":
            emit(set="a_parent_plain", query=name, points=res["points"] if name == "directional" else None, **stats(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--random", type=int, default=1 << 20)
    ap.add_argument("--sets", default="abc")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: (f), and the plain side of (a) once more")
    ap.add_argument("--frame-rounds", type=int, default=4)
    args = ap.parse_args()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    emit(set="invocation", argv=sys.argv[1:], reps=args.reps, warmup=args.warmup, random=args.random, sets=args.sets)
    if args.parent_tree:
        frames(args.parent_tree, args.frame_rounds)
        if "a" in args.sets:
            parent_plain(args.parent_tree, args.reps, args.warmup)
    import torch

    torch.zeros(1, device="cuda:0")  # torch's HIP runtime up BEFORE the library is loaded (as bench.py does)
    dev = torch.device("cuda:0")
    scene = rt.Scene.load_off(bunny_path()).build_bvh(0)
    opt = rt.Options.defaults(width=1920, height=1080, n_super_samples=1, **AO)
    host = rt.Host(opt, 0)
    host.upload_scene(scene)
    rng = np.random.default_rng(1)
    rays_per_point = host.ao_rays_per_point[0]

    side = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(side)  # (every torch kernel and, through the binding, every query below: this one stream)

    def on_device(*arrays):
        out = tuple(torch.from_numpy(a).to(dev) for a in arrays)
        side.synchronize()
        return out

    def timed(call):
        """One call and its time; waits for it, so nothing it reads or writes is reused while it runs."""
        call()
        return host.last_query_ms

    def run(call):
        for _ in range(args.warmup):
            timed(call)
        return [timed(call) for _ in range(args.reps)]

    def alternating(plain, inst):
        for _ in range(args.warmup):
            timed(plain), timed(inst)
        p_ms, i_ms = [], []
        for _ in range(args.reps):  # alternating, so that a drift of the clock hits both alike
            p_ms.append(timed(plain))
            i_ms.append(timed(inst))
        ratios = np.asarray(i_ms) / np.asarray(p_ms)
        return dict(plain=stats(p_ms), instanced=stats(i_ms), ratio_median=float(np.median(ratios)), ratio_min=float(ratios.min()),
                    ratio_max=float(ratios.max()))

    def multihit_outputs(k, instanced):
        return (rt.INSTANCE_MULTIHIT_OUTPUTS if instanced else rt.api.MULTIHIT_OUTPUTS) if k else ("count",)

    def surface_points(to, td, limit):
        """(points, normals) float32 (n, 4) on the device: the hit points of the rays, made once and waited for."""
        near = host.trace_instances_closest(to, td, outputs=("hit", "position", "normal"))
        side.synchronize()
        hit = near["hit"].bool()
        p = torch.nn.functional.pad(near["position"][hit][:limit], (0, 1)).contiguous()
        q = torch.nn.functional.pad(near["normal"][hit][:limit], (0, 1)).contiguous()
        side.synchronize()
        return p, q

    def host_instances():
        return int(rt.load_library().rt_instance_count(host._h))

    def masks_against_written_out(p, q):
        """(c) at the points (p, q), float32 (n, 4) on the device."""
        n, R = int(p.shape[0]), rays_per_point
        weights = (torch.ones(32, dtype=torch.int64, device=dev) << torch.arange(32, device=dev)).view(1, 1, 32)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def written_out():
            """ao_rays, trace_instances_occluded on the written rays, the packing: the sum of the three device times."""
            rays = host.ao_rays(p, q)
            ms = host.last_query_ms
            origins = rays["origins"].repeat_interleave(R, dim=0)  # (R float4 origins a point: what the occlusion query reads)
            flags = host.trace_instances_occluded(origins, rays["directions"].view(n * R, 4), max_distance=float(opt.ao_max_distance))
            ms += host.last_query_ms
            start.record(side)
            padded = torch.zeros((n, ((R + 31) // 32) * 32), dtype=torch.int64, device=dev)
            padded[:, :R] = flags.view(n, R)
            mask = (padded.view(n, -1, 32) * weights).sum(dim=2).to(torch.int32)
            stop.record(side)
            stop.synchronize()
            return ms + start.elapsed_time(stop), mask

        def masks():
            got = host.instances_directional_occlusion(p, q, outputs=("mask",))
            return host.last_query_ms, got["mask"]

        _, want = written_out()
        _, got = masks()
        if not torch.equal(got.view(torch.int32), want):
            raise SystemExit("(c): the masks differ from the written-out rays' flags")
        for _ in range(args.warmup):
            written_out(), masks()
        w_ms, m_ms = [], []
        for _ in range(args.reps):
            w_ms.append(written_out()[0])
            m_ms.append(masks()[0])
        ratios = np.asarray(m_ms) / np.asarray(w_ms)
        emit(set="c_masks_against_written_out_rays", instances=host_instances(), points=n, rays_per_point=R, written_out=stats(w_ms),
             masks=stats(m_ms), blocked_share=float((want != 0).any(dim=1).float().mean()), ratio_median=float(np.median(ratios)),
             ratio_min=float(ratios.min()), ratio_max=float(ratios.max()))

    if "a" in args.sets:
        host.set_instances(np.eye(3, 4, dtype=np.float32)[None])
        lo, hi = scene.aabbs[0, :3].astype(np.float64), scene.aabbs[1, :3].astype(np.float64)
        camera = qo.camera_rays(orc.params_from_options(opt))
        for name, (o4, d4) in (("camera", camera), ("random", random_rays(lo, hi, args.random, rng))):
            to, td = on_device(o4, d4)
            for k in KS:
                res = alternating(lambda: host.trace_multihit(to, td, k=k, outputs=multihit_outputs(k, False)),
                                  lambda: host.trace_instances_multihit(to, td, k=k, outputs=multihit_outputs(k, True)))
                emit(set="a_identity_multihit", rays_from=name, k=k, rays=len(o4), **res)
            del to, td
        to, td = on_device(*camera)
        p, q = surface_points(to, td, 1 << 22)
        res = alternating(lambda: host.directional_occlusion(p, q), lambda: host.instances_directional_occlusion(p, q))
        emit(set="a_identity_directional", points=int(p.shape[0]), rays_per_point=rays_per_point, **res)
        del to, td, p, q

    if set("bc") & set(args.sets):
        W = poses(scene, 10, rng)
        host.set_instances(W)
        nodes = host.instances()["nodes"]
        top_lo, top_hi = nodes["lo"][0].astype(np.float64), nodes["hi"][0].astype(np.float64)
        if "b" in args.sets:
            for name, (o4, d4) in (("b_grid_camera_like", camera_like(nodes, 1024, rng)),
                                   ("b_grid_random", random_rays(top_lo, top_hi, args.random, rng))):
                to, td = on_device(o4, d4)
                count = host.count_instances_hits(to, td)
                side.synchronize()
                count = count.double()
                for k in KS:
                    for sort in (True, False):
                        s = stats(run(lambda: host.trace_instances_multihit(to, td, k=k, outputs=multihit_outputs(k, True), sort=sort)))
                        emit(set=name, k=k, order="sorted" if sort else "unsorted", instances=len(W), rays=len(o4),
                             members_per_ray=float(count.mean()), most_members=int(count.max()), mrays_per_s=len(o4) / s["median_ms"] / 1e3, **s)
                del to, td
        if "c" in args.sets:
            to, td = on_device(*camera_like(nodes, 1024, rng))
            every = surface_points(to, td, 1 << 22)
            del to, td
            # (about a million written-out rays -- launches and the sort weigh in -- and every hit point of the camera-like rays)
            for limit in ((1 << 20) // rays_per_point, int(every[0].shape[0])):
                masks_against_written_out(every[0][:limit].contiguous(), every[1][:limit].contiguous())
    side.synchronize()
    host.close()


if __name__ == "__main__":
    main()
