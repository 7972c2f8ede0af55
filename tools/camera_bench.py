#!/usr/bin/env python3
"""What a posed camera costs (include/rt_hip_camera.h): one JSON line per measurement, appended to
profiles/camera_bench.jsonl.  HIP-event kernel times (rt_last_kernel_ms and, per pass, rt_last_ao_ms; the primary pass
alone is the frame with -a 0), the median of --reps frames after --warmup; 1920 x 1080, -s 1 -a 3 unless said otherwise.

  1. headline (bunny), no camera set: this library against a BASELINE build of the parent commit (--baseline-lib-dir, a
     directory of this package that holds its libocrt_hip.so, e.g. lib_parent), one-shot host and ring of three.  The two
     are measured in processes of their own that ALTERNATE, --rounds times: the spread of the baseline's rounds is what a
     difference has to exceed to mean anything.
  2. the same frame with the default pose through the posed path: the price of the posed form alone.
  3. an orbit of eight eyes around the bunny and one eye inside each interior stand-in: frame ms, primary ms, hits,
     Grays/s, upload ms (what a turntable pays per view today).
  4. a far eye at ten extents on the fast walk, and one at 1e7 on the exact form.

    python3 tools/camera_bench.py [--sets 1,2,3,4] [--baseline-lib-dir lib_parent] [--rounds 3] [--reps 20] [--warmup 5]
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

W, H = 1920, 1080


def emit(out, **kv):
    line = json.dumps(kv)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def median_frames(host, reps, warmup):
    k, a = [], []
    for i in range(warmup + reps):
        host.render()
        if i >= warmup:
            k.append(host.last_kernel_ms)
            a.append(host.last_ao_ms)
    return float(np.median(k)), float(np.min(k)), float(np.median(a))


def one_shot(rt, scene, cam, ao, reps, warmup, stream=True):
    """(frame ms median, min, ao_kernel ms, upload ms, stats) of a host on its own."""
    opt = rt.Options.defaults(width=W, height=H, n_super_samples=1, ao_num_samples=ao)
    host = rt.Host(opt, 0)
    if stream:
        host.expect_frames(1 << 20)
    if cam is not None:
        host.set_camera(cam)
    t0 = time.perf_counter()
    host.upload_scene(scene)
    upload_ms = (time.perf_counter() - t0) * 1e3
    med, best, ao_ms = median_frames(host, reps, warmup)
    stats = host.stats()
    host.close()
    return med, best, ao_ms, upload_ms, stats


def ring_ms(rt, scene, cam, reps, warmup):
    """ms per frame of a ring of three in steady state (wall clock around run() + drain(), frames in flight)."""
    opt = rt.Options.defaults(width=W, height=H, n_super_samples=1, ao_num_samples=3)
    kw = {"camera": cam} if cam is not None else {}
    ring = rt.FrameRing(opt, scene, device=0, hosts=3, **kw)
    ring.run(warmup * 3)
    ring.drain()
    samples = []
    for _ in range(5):
        t0 = time.perf_counter()
        ring.run(reps * 3)
        ring.drain()
        samples.append((time.perf_counter() - t0) * 1e3 / (reps * 3))
    ring.close()
    return float(np.median(samples)), float(np.min(samples))


def measure_headline(args, label):
    """Set 1's body, run in a process of its own per library (OCRT_LIB_DIR chooses it)."""
    import opencl_raytracer_amd as rt
    from tools.meshes import bunny_path

    scene = rt.Scene.load_off(bunny_path()).build_bvh(0)
    frame, best, ao_ms, upload_ms, stats = one_shot(rt, scene, None, 3, args.reps, args.warmup)
    primary, primary_best, _, _, _ = one_shot(rt, scene, None, 0, args.reps, args.warmup)
    ring, ring_best = ring_ms(rt, scene, None, args.reps, args.warmup)
    emit(args.out, set="1_headline_no_camera", library=label, round=args.round, frame_ms=frame, frame_min_ms=best, ao_kernel_ms=ao_ms,
         primary_ms=primary, primary_min_ms=primary_best, ring3_ms_per_frame=ring, ring3_min_ms_per_frame=ring_best, upload_ms=upload_ms,
         primary_hits=stats["primary_hits"], ao_occluded=stats["ao_occluded"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="1,2,3,4")
    ap.add_argument("--baseline-lib-dir", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "camera_bench.jsonl"))
    ap.add_argument("--headline-only", default=None, help=argparse.SUPPRESS)  # (the child processes of set 1)
    ap.add_argument("--round", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.headline_only:
        return measure_headline(args, args.headline_only)
    sets = set(args.sets.split(","))
    if "1" in sets:
        for r in range(args.rounds):
            for label, lib_dir in (("baseline", args.baseline_lib_dir), ("this", None)):
                if label == "baseline" and not lib_dir:
                    continue
                env = dict(os.environ)
                if lib_dir:
                    env["OCRT_LIB_DIR"], env["OCRT_ALLOW_OLD_LIB"] = lib_dir, "1"
                subprocess.run([sys.executable, os.path.abspath(__file__), "--headline-only", label, "--round", str(r), "--reps", str(args.reps),
                                "--warmup", str(args.warmup), "--out", args.out], env=env, check=True, timeout=600)
    if not sets & {"2", "3", "4"}:
        return
    import opencl_raytracer_amd as rt
    from tools.meshes import bunny_path, interior_hard_path, interior_path

    bunny = rt.Scene.load_off(bunny_path()).build_bvh(0)

    def posed(name, scene, cam, set_name, **extra):
        frame, best, ao_ms, upload_ms, stats = one_shot(rt, scene, cam, 3, args.reps, args.warmup)
        primary, primary_best, _, _, _ = one_shot(rt, scene, cam, 0, args.reps, args.warmup)
        rays = stats["primary_rays"] + stats["ao_rays"]
        emit(args.out, set=set_name, pose=name, frame_ms=frame, frame_min_ms=best, ao_kernel_ms=ao_ms, primary_ms=primary, primary_min_ms=primary_best,
             upload_ms=upload_ms, primary_hits=stats["primary_hits"], ao_occluded=stats["ao_occluded"], grays_per_s=rays / frame / 1e6, **extra)

    if "2" in sets:
        for r in range(args.rounds):
            posed("default_pose", bunny, rt.Camera.default(), "2_headline_default_pose_posed_path", round=r)
            posed("no_camera", bunny, None, "2_headline_default_pose_posed_path", round=r)
        ring, ring_best = ring_ms(rt, bunny, rt.Camera.default(), args.reps, args.warmup)
        emit(args.out, set="2_headline_default_pose_posed_path", pose="default_pose", ring3_ms_per_frame=ring, ring3_min_ms_per_frame=ring_best)
    if "3" in sets:
        for k in range(8):
            a = 2 * np.pi * k / 8
            posed(f"orbit_{45 * k}", bunny, rt.Camera.look_at((2 * np.sin(a), 0.4, 2 * np.cos(a)), (0, 0, 0)), "3_orbit")
        for name, path in (("interior", interior_path()), ("interior_hard", interior_hard_path())):
            scene = rt.Scene.load_off(path).build_bvh(0)
            lo, hi = scene.aabbs[0, :3].astype(np.float64), scene.aabbs[1, :3].astype(np.float64)
            c = 0.5 * (lo + hi)
            eye = (c[0] + 0.1 * (hi[0] - lo[0]), lo[1] + 0.35 * (hi[1] - lo[1]), hi[2] - 0.15 * (hi[2] - lo[2]))
            posed(name + "_nave", scene, rt.Camera.look_at(eye, (c[0], lo[1] + 0.4 * (hi[1] - lo[1]), lo[2])), "3_inside")
            posed(name + "_no_camera", scene, None, "3_inside")
    if "4" in sets:
        # ten extents away (the bunny's ground plane reaches 10) with a lens that keeps the model in view: the fast walk;
        # 1e7: beyond what origin_limit can cover -- the exact form (and beyond the primary rays' max_distance: no hits)
        for name, eye, zoom in (("far_10x_fast_walk", (60.0, 20.0, 100.0), 12.0), ("far_1e7_exact_walk", (0.6e7, 0.2e7, 1.0e7), 4.0e5)):
            m = rt.Camera.look_at(eye, (0, 0, 0)).as_array()
            posed(name, bunny, rt.Camera.from_vectors(m[0], m[1], m[2], m[3] * np.float32(zoom)), "4_far")


if __name__ == "__main__":
    main()
