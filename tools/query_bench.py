#!/usr/bin/env python3
"""Ray-query throughput on the bunny (include/rt_hip_query.h): one JSON line per set.

  (a) the 1920x1080 reference camera rays, closest hit (beside: the frame's own time with -a 0, primary pass + finish)
  (b) AO-like rays: the camera hits offset by normal * 1e-5, the 28 directions of the default table around each, occlusion
      with ao_max_distance (beside: the frame's ao_kernel time)
  (c) 4 M uniformly random rays with origins in the scene box: both queries, sorted and unsorted
  (d) the host-memory entry point end to end (wall clock, copies included) for (c)
  (m) multi-hit queries (include/rt_hip_multihit.h) on the rays of (a) and (c): count_hits and k = 1, 4, 16 with every
      output, beside trace_closest on the same rays in the same run (ratio_to_closest: time over the closest hit's)
  (o) ambient-occlusion queries (include/rt_hip_ao.h) at the closest hits of (a), position and smooth normal in image order,
      with the default AO options (UNIFORM): host.ambient_occlusion on device tensors, sorted and sort=False
Device entry points on pre-loaded buffers; the time of a call is rt_last_query_ms (HIP events around sort + walk); the
median of --reps calls after --warmup.

    python3 tools/query_bench.py [--reps 20] [--warmup 3] [--random 4194304] [--sets abcdmo]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import opencl_raytracer_amd as rt  # noqa: E402
import orc  # noqa: E402
import query_oracle as qo  # noqa: E402
from opencl_raytracer_amd.api import RT_QUERY_NO_SORT, _HitArrays, _MultiHitArrays  # noqa: E402
from tools.meshes import bunny_path  # noqa: E402


def timed(host, call, reps, warmup):
    import torch

    for _ in range(warmup):
        call()
    ms = []
    for _ in range(reps):
        call()
        ms.append(host.last_query_ms)
    torch.cuda.synchronize()
    return float(np.median(ms)), float(np.min(ms))


def basis(n):
    """Tangent frame of reference src/intersect_kernel.cl:224-236 (numpy, for measurement only)."""
    h = n.copy()
    a = np.abs(n)
    ix = (a[:, 0] <= a[:, 1]) & (a[:, 0] <= a[:, 2])
    iy = ~ix & (a[:, 1] <= a[:, 0]) & (a[:, 1] <= a[:, 2])
    iz = ~ix & ~iy
    h[ix, 0] = 1.0
    h[iy, 1] = 1.0
    h[iz, 2] = 1.0
    bx = np.cross(h, n)
    bx /= np.linalg.norm(bx, axis=1, keepdims=True)
    bz = np.cross(bx, n)
    bz /= np.linalg.norm(bz, axis=1, keepdims=True)
    return bx.astype(np.float32), bz.astype(np.float32)


def main():
    import torch

    torch.zeros(1, device="cuda:0")  # torch's HIP runtime up BEFORE the library is loaded (as bench.py does)
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--random", type=int, default=4 << 20)
    ap.add_argument("--sets", default="abcdmo", help="which of the sets (a) (b) (c) (d) (m) (o) to run")
    args = ap.parse_args()
    if "b" in args.sets and not set("am") & set(args.sets):
        ap.error("--sets: (b) starts from the camera hits, which (a) or (m) cast")
    lib = rt.load_library()
    dev = torch.device("cuda:0")
    scene = rt.Scene.load_off(bunny_path()).build_bvh(0)
    opt = rt.Options.defaults(width=1920, height=1080, n_super_samples=1)
    host = rt.Host(opt, 0)
    host.upload_scene(scene)

    def frame_ms(enable_ao):
        o = rt.Options.defaults(width=1920, height=1080, n_super_samples=1, enable_ao=enable_ao)
        h = rt.Host(o, 0)
        h.upload_scene(scene)
        k, a = [], []
        for i in range(args.warmup + args.reps):
            h.render()
            if i >= args.warmup:
                k.append(h.last_kernel_ms)
                a.append(h.last_ao_ms)
        h.close()
        return float(np.median(k)), float(np.median(a))

    def device_call(closest, o, d, n, md, flags, out):
        if closest:
            arrays = _HitArrays(*[out[f].data_ptr() if f in out else None for f in qo_fields])
            return lambda: lib.rt_trace_closest_device(host._h, o.data_ptr(), d.data_ptr(), n, md, flags, C.byref(arrays), None)
        return lambda: lib.rt_trace_occluded_device(host._h, o.data_ptr(), d.data_ptr(), n, md, flags, out["hit"].data_ptr(), None)

    qo_fields = ("hit", "distance", "leaf", "barycentric", "position", "normal")

    def outputs(n):
        return {"hit": torch.empty(n, dtype=torch.uint8, device=dev), "distance": torch.empty(n, dtype=torch.float32, device=dev),
                "leaf": torch.empty(n, dtype=torch.uint32, device=dev),
                "barycentric": torch.empty((n, 3), dtype=torch.float32, device=dev),
                "position": torch.empty((n, 3), dtype=torch.float32, device=dev),
                "normal": torch.empty((n, 3), dtype=torch.float32, device=dev)}

    def emit(**kv):
        print(json.dumps(kv), flush=True)

    def multihit_leg(name, o, d, n, out):
        """(m) on rays already on the device: closest hit, then the count alone and k = 1, 4, 16, sorted."""
        closest_ms, _ = timed(host, device_call(True, o, d, n, 100000.0, 0, out), args.reps, args.warmup)
        emit(set="m_" + name, query="closest", rays=n, median_ms=closest_ms, grays_per_s=n / closest_ms / 1e6)
        count = torch.empty(n, dtype=torch.uint32, device=dev)
        for k in (0, 1, 4, 16):
            slots = {"distance": torch.empty((n, k), dtype=torch.float32, device=dev),
                     "leaf": torch.empty((n, k), dtype=torch.uint32, device=dev),
                     "barycentric": torch.empty((n, k, 3), dtype=torch.float32, device=dev),
                     "position": torch.empty((n, k, 3), dtype=torch.float32, device=dev),
                     "normal": torch.empty((n, k, 3), dtype=torch.float32, device=dev)} if k else {}
            arrays = _MultiHitArrays(count.data_ptr(), *[slots[f].data_ptr() if k else None for f in qo_fields[1:]])

            def call(k=k, arrays=arrays):
                rc = lib.rt_trace_multihit_device(host._h, o.data_ptr(), d.data_ptr(), n, 100000.0, k, 0, C.byref(arrays), None)
                assert rc == 0, rc

            med, best = timed(host, call, args.reps, args.warmup)
            c = count.cpu().numpy()
            emit(set="m_" + name, query="count_hits" if k == 0 else f"multihit_k{k}", rays=n, median_ms=med, min_ms=best,
                 grays_per_s=n / med / 1e6, ratio_to_closest=med / closest_ms, mean_count=float(c.mean()), max_count=int(c.max()),
                 share_of_rays_with_more_than_k=float((c > k).mean()))
            del slots

    # (a) camera rays
    p = orc.params_from_options(opt)
    o4, d4 = qo.camera_rays(p)
    n = o4.shape[0]
    to, td = torch.from_numpy(o4).to(dev), torch.from_numpy(d4).to(dev)
    out = outputs(n)
    if "a" in args.sets:
        a0_ms, _ = frame_ms(0)
    for flags, name in ((0, "sorted"), (RT_QUERY_NO_SORT, "unsorted")) if "a" in args.sets else ():
        med, best = timed(host, device_call(True, to, td, n, 100000.0, flags, out), args.reps, args.warmup)
        emit(set="a_camera_closest", order=name, rays=n, median_ms=med, min_ms=best, grays_per_s=n / med / 1e6,
             frame_a0_ms=a0_ms, ratio_to_frame_a0=med / a0_ms)
    if "m" in args.sets:
        multihit_leg("camera", to, td, n, out)
    if "b" in args.sets:
        ao_like_rays(out, dev, opt, host, args, device_call, frame_ms, emit)
    if "o" in args.sets:
        ao_queries(out, to, td, n, host, args, device_call, emit)
    del to, td, out
    random_rays(scene, dev, host, args, device_call, outputs, emit, multihit_leg)
    host.close()


def ao_like_rays(out, dev, opt, host, args, device_call, frame_ms, emit):
    import torch

    # (b) AO-like rays around the camera hits
    hit = out["hit"].cpu().numpy().astype(bool)
    pos, nrm = out["position"].cpu().numpy()[hit], out["normal"].cpu().numpy()[hit]
    table = orc.Oracle().ao_table(orc.params_from_options(opt))[:, :3].astype(np.float32)
    origin = (pos + nrm * np.float32(1e-5)).astype(np.float32)
    bx, bz = basis(nrm)
    dirs = (bx[:, None, :] * table[None, :, 0:1] + nrm[:, None, :] * table[None, :, 1:2] + bz[:, None, :] * table[None, :, 2:3])
    dirs = dirs.reshape(-1, 3).astype(np.float32)
    orig = np.repeat(origin, len(table), axis=0)
    nb = dirs.shape[0]
    to = torch.nn.functional.pad(torch.from_numpy(orig).to(dev), (0, 1)).contiguous()
    td = torch.nn.functional.pad(torch.from_numpy(dirs).to(dev), (0, 1)).contiguous()
    ob = {"hit": torch.empty(nb, dtype=torch.uint8, device=dev)}
    _, ao_ms = frame_ms(1)
    md = orc.kernel_float(opt.ao_max_distance)
    for flags, name in ((0, "sorted"), (RT_QUERY_NO_SORT, "unsorted")):
        med, best = timed(host, device_call(False, to, td, nb, md, flags, ob), args.reps, args.warmup)
        emit(set="b_ao_like_occluded", order=name, rays=nb, directions_per_hit=len(table), median_ms=med, min_ms=best,
             grays_per_s=nb / med / 1e6, frame_ao_kernel_ms=ao_ms, ratio_to_ao_kernel=med / ao_ms if ao_ms else None)
    del to, td, ob


def ao_queries(out, to, td, n, host, args, device_call, emit):
    import torch

    # (o) the fused AO query at the camera's closest hits
    device_call(True, to, td, n, 100000.0, 0, out)()
    torch.cuda.synchronize()
    hit = out["hit"].bool()
    # (N, 4) already, so that a call pads nothing; ready before the first call: the queries run on the host's own stream
    points = torch.nn.functional.pad(out["position"][hit], (0, 1)).contiguous()
    normals = torch.nn.functional.pad(out["normal"][hit], (0, 1)).contiguous()
    torch.cuda.synchronize()
    rays_per_point, _ = host.ao_rays_per_point
    np_, nr = int(points.shape[0]), int(points.shape[0]) * rays_per_point
    for sort, name in ((True, "sorted"), (False, "unsorted")):
        med, best = timed(host, lambda sort=sort: host.ambient_occlusion(points, normals, sort=sort), args.reps, args.warmup)
        emit(set="o_ao_query", order=name, points=np_, rays_per_point=rays_per_point, rays=nr, median_ms=med, min_ms=best,
             grays_per_s=nr / med / 1e6)
    del points, normals


def random_rays(scene, dev, host, args, device_call, outputs, emit, multihit_leg):
    import torch

    if not set("cdm") & set(args.sets):
        return
    # (c) random rays in the scene box
    nr = args.random
    lo, hi = scene.aabbs[0, :3], scene.aabbs[1, :3]
    rng = np.random.default_rng(1)
    o = (lo + rng.random((nr, 3), dtype=np.float32) * (hi - lo)).astype(np.float32)
    d = rng.normal(size=(nr, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o4 = np.zeros((nr, 4), np.float32)
    d4 = np.zeros((nr, 4), np.float32)
    o4[:, :3], d4[:, :3] = o, d
    to, td = torch.from_numpy(o4).to(dev), torch.from_numpy(d4).to(dev)
    out = outputs(nr)
    for closest in (True, False) if "c" in args.sets else ():
        for flags, name in ((0, "sorted"), (RT_QUERY_NO_SORT, "unsorted")):
            med, best = timed(host, device_call(closest, to, td, nr, 100000.0, flags, out), args.reps, args.warmup)
            emit(set="c_random_" + ("closest" if closest else "occluded"), order=name, rays=nr, median_ms=med, min_ms=best,
                 grays_per_s=nr / med / 1e6)
    if "m" in args.sets:
        multihit_leg("random", to, td, nr, out)
    # (d) host memory, end to end
    for closest in (True, False) if "d" in args.sets else ():
        wall = []
        for i in range(2 + 5):
            t0 = time.perf_counter()
            if closest:
                host.trace_closest(o4, d4)
            else:
                host.trace_occluded(o4, d4)
            if i >= 2:
                wall.append((time.perf_counter() - t0) * 1e3)
        emit(set="d_host_memory_" + ("closest" if closest else "occluded"), rays=nr, median_wall_ms=float(np.median(wall)),
             kernels_ms=host.last_query_ms, grays_per_s_end_to_end=nr / float(np.median(wall)) / 1e6)


if __name__ == "__main__":
    main()
