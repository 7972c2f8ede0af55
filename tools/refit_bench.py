#!/usr/bin/env python3
"""Vertex updates against re-uploads (include/rt_hip_update.h): JSON lines, printed and appended to profiles/refit_bench.jsonl.

Per mesh -- the bunny (70 570 triangles) and the 2 M-triangle height field of tools/big_meshes.py --:

  update   host.update_vertices on device tensors (positions and normals of a twisted copy, on the device before the first
           call): rt_last_update_ms, HIP events around the update's launches, median of --reps after --warmup, for every
           group size of --groups (the sweep the default S is chosen from); beside it the wall clock of the call with the
           wait for the device.  The first update of an upload, which also copies the faces and the schedule, is reported
           on its own.
  upload   the wall clock of a full host.upload_scene of the same mesh, median of --upload-reps after one that is not
           counted: on this library, and -- the figure an update is to be compared with -- on the PARENT commit's library,
           built into opencl_raytracer_amd/<--parent-lib> and loaded by a child process of this tool (OCRT_LIB_DIR,
           OCRT_ALLOW_OLD_LIB=1: that library lacks the update's entry points, which the child does not call).

    python3 tools/refit_bench.py [--meshes bunny,terrain] [--reps 20] [--warmup 3] [--groups 64,128,256,512]
                                 [--upload-reps 5] [--parent-lib lib_old]
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

OPTIONS = dict(width=64, height=48, n_super_samples=1, ao_num_samples=3, ao_max_distance=0.2)


def load(rt, name):
    from tools.big_meshes import terrain
    from tools.meshes import bunny_path

    if name == "bunny":
        return rt.Scene.load_off(bunny_path()).build_bvh(0)
    if name == "terrain":
        v, f = terrain(1000)
        return rt.Scene.from_arrays(v, f).build_bvh(0)
    raise SystemExit(f"unknown mesh {name}")


def upload_ms(rt, scene, reps):
    host = rt.Host(rt.Options.defaults(**OPTIONS), 0)
    wall = []
    for i in range(reps + 1):
        t0 = time.perf_counter()
        host.upload_scene(scene)
        if i:
            wall.append((time.perf_counter() - t0) * 1e3)
    host.close()
    return float(np.median(wall)), float(np.min(wall))


def main():
    import torch

    torch.zeros(1, device="cuda:0")  # torch's HIP runtime up BEFORE the library is loaded (as bench.py does)
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", default="bunny,terrain")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--groups", default="64,128,256,512")
    ap.add_argument("--upload-reps", type=int, default=5)
    ap.add_argument("--parent-lib", default="lib_old")
    ap.add_argument("--upload-only", action="store_true", help="(the child process on the parent's library)")
    args = ap.parse_args()
    import opencl_raytracer_amd as rt

    lines = []

    def emit(**kv):
        print(json.dumps(kv), flush=True)
        lines.append(kv)

    for name in args.meshes.split(","):
        scene = load(rt, name)
        facts = dict(mesh=name, triangles=scene.num_faces, nodes=scene.num_nodes, vertices=scene.num_vertices)
        med, best = upload_ms(rt, scene, args.upload_reps)
        emit(set="upload", library="parent" if args.upload_only else "this", median_wall_ms=med, min_wall_ms=best, **facts)
        if args.upload_only:
            continue
        from refit_cases import twist

        dev = torch.device("cuda:0")
        original = scene.vertices
        moved = rt.Scene.from_arrays(twist(original), scene.faces.reshape(-1, 3))  # (for its normals)
        tv = [torch.from_numpy(original).to(dev), torch.from_numpy(moved.vertices).to(dev)]
        tn = [torch.from_numpy(scene.vnormals).to(dev), torch.from_numpy(moved.vnormals).to(dev)]
        torch.cuda.synchronize()
        for group in [int(g) for g in args.groups.split(",")]:
            host = rt.Host(rt.Options.defaults(**OPTIONS), 0)
            host.upload_scene(scene)
            host.set_refit_group(group)
            t0 = time.perf_counter()
            host.update_vertices(tv[1], tn[1])
            torch.cuda.synchronize()
            first_wall = (time.perf_counter() - t0) * 1e3
            first_ms = host.last_update_ms
            ms, wall = [], []
            for i in range(args.warmup + args.reps):
                t0 = time.perf_counter()
                host.update_vertices(tv[i & 1], tn[i & 1])  # back and forth between the two poses
                torch.cuda.synchronize()
                if i >= args.warmup:
                    wall.append((time.perf_counter() - t0) * 1e3)
                    ms.append(host.last_update_ms)
            passes = scene.refit_schedule(group, packed_tree=True)["passes"]
            emit(set="update", group_nodes=group, launches=1 + passes, median_ms=float(np.median(ms)), min_ms=float(np.min(ms)),
                 median_wall_ms=float(np.median(wall)), first_update_ms=first_ms, first_update_wall_ms=first_wall, **facts)
            host.close()
        del tv, tn
    if args.upload_only:
        return
    parent = os.path.join(ROOT, "opencl_raytracer_amd", args.parent_lib, "libocrt_hip.so")
    if os.path.exists(parent):
        env = dict(os.environ, OCRT_LIB_DIR=args.parent_lib, OCRT_ALLOW_OLD_LIB="1")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--upload-only", "--meshes", args.meshes, "--upload-reps",
                            str(args.upload_reps)], capture_output=True, text=True, env=env)
        if r.returncode != 0:
            raise SystemExit("the run on the parent's library failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
        for line in r.stdout.splitlines():
            if line.startswith("{"):
                emit(**json.loads(line))
    else:
        print(f"(no parent library at {parent}: the re-upload figure of the comparison is missing)", file=sys.stderr)
    for up in [x for x in lines if x["set"] == "upload" and x["library"] == "parent"]:
        for u in [x for x in lines if x["set"] == "update" and x["mesh"] == up["mesh"]]:
            emit(set="update_vs_parent_upload", mesh=up["mesh"], group_nodes=u["group_nodes"], update_ms=u["median_ms"],
                 update_wall_ms=u["median_wall_ms"], parent_upload_wall_ms=up["median_wall_ms"],
                 upload_over_update=up["median_wall_ms"] / u["median_wall_ms"], faster=u["median_wall_ms"] < up["median_wall_ms"])
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "refit_bench.jsonl"), "a") as f:
        for kv in lines:
            f.write(json.dumps(kv) + "\n")


if __name__ == "__main__":
    main()
