#!/usr/bin/env python3
"""Device-side builds against uploads (include/rt_hip_build.h): JSON lines, printed and appended to profiles/build_bench.jsonl.

Per mesh -- the bunny (70 570 triangles) and the 2 M-triangle height field of tools/big_meshes.py --:

  build    host.build_scene on device tensors (vertices, normals and faces on the device before the first call):
           rt_last_build_ms (HIP events around the build's two runs of launches) and the wall clock of the call, median of
           --reps after --warmup; apart, from rt_debug_last_build_times: the topology's kernels, the records' kernels and the
           host's step between them (the schedule of the inner boxes made from the downloaded skips and copied back).
  upload   the wall clock of Scene.build_bvh(0) + host.upload_scene and of host.upload_scene alone, median of --upload-reps
           after one that is not counted, on the PARENT commit's library, built into opencl_raytracer_amd/<--parent-lib> and
           loaded by a child process of this tool (OCRT_LIB_DIR, OCRT_ALLOW_OLD_LIB=1); and on this library.
  walk     what the built tree costs the queries: sets (a) -- the 1920 x 1080 reference camera rays, closest hit -- and (c) --
           --random uniformly random rays in the scene box, closest hit and occlusion -- of tools/query_bench.py, unsorted,
           rt_last_query_ms, on a built host and on a host that uploaded the same mesh, in the same run.

    python3 tools/build_bench.py [--meshes bunny,terrain] [--reps 20] [--warmup 3] [--upload-reps 5] [--random 4194304]
                                 [--parent-lib lib_old]
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
    """A scene without a tree."""
    from tools.big_meshes import terrain
    from tools.meshes import bunny_path

    if name == "bunny":
        return rt.Scene.load_off(bunny_path())
    if name == "terrain":
        v, f = terrain(1000)
        return rt.Scene.from_arrays(v, f)
    raise SystemExit(f"unknown mesh {name}")


def upload_legs(rt, scene, reps, emit, library, facts):
    host = rt.Host(rt.Options.defaults(**OPTIONS), 0)
    both, alone, tree = [], [], []
    for i in range(reps + 1):
        t0 = time.perf_counter()
        scene.build_bvh(0)
        t1 = time.perf_counter()
        host.upload_scene(scene)
        t2 = time.perf_counter()
        if i:
            both.append((t2 - t0) * 1e3)
            alone.append((t2 - t1) * 1e3)
            tree.append((t1 - t0) * 1e3)
    host.close()
    emit(set="upload", library=library, build_bvh_and_upload_wall_ms=float(np.median(both)), upload_wall_ms=float(np.median(alone)),
         build_bvh_wall_ms=float(np.median(tree)), reps=reps, **facts)


def query_ms(host, call, reps, warmup):
    import torch

    for _ in range(warmup):
        call()
    ms = []
    for _ in range(reps):
        call()
        ms.append(host.last_query_ms)
    torch.cuda.synchronize()
    return float(np.median(ms))


def main():
    import torch

    torch.zeros(1, device="cuda:0")  # torch's HIP runtime up BEFORE the library is loaded (as bench.py does)
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", default="bunny,terrain")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--upload-reps", type=int, default=5)
    ap.add_argument("--random", type=int, default=4 << 20)
    ap.add_argument("--parent-lib", default="lib_old")
    ap.add_argument("--upload-only", action="store_true", help="(the child process on the parent's library)")
    args = ap.parse_args()
    import opencl_raytracer_amd as rt

    lines = []

    def emit(**kv):
        print(json.dumps(kv), flush=True)
        lines.append(kv)

    dev = torch.device("cuda:0")
    for name in args.meshes.split(","):
        scene = load(rt, name)
        facts = dict(mesh=name, triangles=scene.num_faces, vertices=scene.num_vertices)
        upload_legs(rt, scene, args.upload_reps, emit, "parent" if args.upload_only else "this", facts)
        if args.upload_only:
            continue
        import orc
        import query_oracle as qo

        tv, tn = torch.from_numpy(scene.vertices.copy()).to(dev), torch.from_numpy(scene.vnormals.copy()).to(dev)
        tf = torch.from_numpy(scene.faces.astype(np.int32).reshape(-1, 3)).to(dev)
        torch.cuda.synchronize()
        built = rt.Host(rt.Options.defaults(**OPTIONS), 0)
        ms, wall, parts = [], [], []
        for i in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            built.build_scene(tv, tf, tn)
            torch.cuda.synchronize()
            if i >= args.warmup:
                wall.append((time.perf_counter() - t0) * 1e3)
                ms.append(built.last_build_ms)
                parts.append(built.last_build_times())
        emit(set="build", median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), median_wall_ms=float(np.median(wall)),
             topology_ms=float(np.median([p["topology_ms"] for p in parts])), records_ms=float(np.median([p["records_ms"] for p in parts])),
             schedule_host_ms=float(np.median([p["schedule_host_ms"] for p in parts])), reps=args.reps, **facts)
        # walk quality: the same rays, unsorted, on the built tree and on the uploaded one
        uploaded = rt.Host(rt.Options.defaults(**OPTIONS), 0)
        uploaded.upload_scene(scene)  # (scene holds the longest-axis tree of the upload legs)
        lo, hi = scene.aabbs[0, :3], scene.aabbs[1, :3]
        o4, d4 = qo.camera_rays(orc.params_from_options(rt.Options.defaults(width=1920, height=1080, n_super_samples=1)))
        rng = np.random.default_rng(1)
        ro, rd = np.zeros((args.random, 4), np.float32), np.zeros((args.random, 4), np.float32)
        ro[:, :3] = lo + rng.random((args.random, 3), dtype=np.float32) * (hi - lo)
        rd[:, :3] = rng.normal(size=(args.random, 3)).astype(np.float32)
        rd[:, :3] /= np.linalg.norm(rd[:, :3], axis=1, keepdims=True)
        sets = (("a_camera_closest", True, o4, d4), ("c_random_closest", True, ro, rd), ("c_random_occluded", False, ro, rd))
        for label, closest, o, d in sets:
            to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
            torch.cuda.synchronize()
            got = {}
            for which, host in (("built", built), ("uploaded", uploaded)):
                call = (lambda h=host: h.trace_closest(to, td, outputs=("hit", "distance"), sort=False)) if closest else \
                       (lambda h=host: h.trace_occluded(to, td, sort=False))
                got[which] = query_ms(host, call, args.reps, args.warmup)
            emit(set="walk", rays_set=label, rays=int(o.shape[0]), built_ms=got["built"], uploaded_ms=got["uploaded"],
                 built_over_uploaded=got["built"] / got["uploaded"], **facts)
            del to, td
        built.close()
        uploaded.close()
        del tv, tn, tf
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
        print(f"(no parent library at {parent}: the upload figures of the comparison are this library's alone)", file=sys.stderr)
    for up in [x for x in lines if x["set"] == "upload" and x["library"] == "parent"]:
        for b in [x for x in lines if x["set"] == "build" and x["mesh"] == up["mesh"]]:
            emit(set="build_vs_parent_upload", mesh=up["mesh"], build_wall_ms=b["median_wall_ms"], build_ms=b["median_ms"],
                 parent_upload_wall_ms=up["upload_wall_ms"], parent_build_bvh_and_upload_wall_ms=up["build_bvh_and_upload_wall_ms"],
                 upload_over_build=up["upload_wall_ms"] / b["median_wall_ms"], faster_than_upload_alone=b["median_wall_ms"] < up["upload_wall_ms"])
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "build_bench.jsonl"), "a") as f:
        for kv in lines:
            f.write(json.dumps(kv) + "\n")


if __name__ == "__main__":
    main()
