"""The expected values of the instanced directional occlusion queries (include/rt_hip_instance_directional.h) BY COMPOSITION
of what the project has: the ambient-occlusion rays of tests/directional_oracle.c through instance_views_oracle.ao_rays (or
the rays host.ao_rays() wrote out), the instanced walk of tests/instance_oracle.c for every ray's flag, numpy for the packing,
directional_oracle.ordered_sum for `bent`; and the same answer in the float64 reference's terms, for
shading_reference.compare_directional.  No C of its own.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import directional_oracle as do
import instance_oracle as io
import instance_reference as ir
import instance_views_oracle as ivo
import shading_reference as sr
from query_oracle import same_words  # noqa: F401

OUTPUTS = ("ao", "occluded", "mask", "bent")
F1 = np.float32(1.0)


def written_rays(origins, directions):
    """(origins (N * R, 3), directions (N * R, 3)) float32: ray k of point i at i * R + k."""
    origins, directions = np.asarray(origins, np.float32)[:, :3], np.asarray(directions, np.float32)[..., :3]
    per = directions.shape[1]
    return np.ascontiguousarray(np.repeat(origins, per, axis=0)), np.ascontiguousarray(directions.reshape(-1, 3))


def directional(params, arrays, plan, points, normals, seeds=None, rays=None) -> dict:
    """{"mask": uint32 (N, W), "occluded": uint32 (N,), "ao": float32 (N,), "bent": float32 (N, 3), "flags": bool (N, R)}.
    `rays`: (origins, directions) to use instead of the oracle's (the RANDOM method: host.ao_rays())."""
    origins, directions = ivo.ao_rays(params, arrays, points, normals, seeds) if rays is None else rays
    directions = np.asarray(directions, np.float32)[..., :3]
    n, per = directions.shape[0], directions.shape[1]
    o, d = written_rays(origins, directions)
    flags = io.occluded(arrays, plan, o, d, params.ao_max_distance).astype(bool).reshape(n, per)
    occluded = flags.sum(axis=1, dtype=np.uint32)
    with np.errstate(all="ignore"):
        ao = (F1 - occluded.astype(np.float32) / np.float32(ivo.ao_divisor(params, per))).astype(np.float32)
    return {"mask": sr.pack(flags), "occluded": occluded, "ao": ao, "bent": do.ordered_sum(directions, ~flags), "flags": flags}


def reference(scene, transforms, origins, directions, max_distance) -> dict:
    """instance_reference.instanced on the written-out rays, in the form shading_reference.compare_directional takes: a ray is
    judged as that module judges it, a point when all of its rays are; `bent` the float64 sum of the directions as cast over
    the rays the reference finds open."""
    d32 = np.asarray(directions, np.float32)[..., :3]
    n, per = d32.shape[0], d32.shape[1]
    o, d = written_rays(origins, d32)
    multi = ir.instanced(scene, transforms, o, d, max_distance)
    hit, judged = (multi["count"] > 0).reshape(n, per), multi["judged"].reshape(n, per)
    bent = (d32.astype(np.float64) * ~hit[:, :, None]).sum(axis=1)
    return {"hit": hit, "judged": judged, "bent": bent, "rays": per, "occluded": hit.sum(axis=1).astype(np.uint32),
            "point_judged": judged.all(axis=1)}


def lifted_points(arrays, plan, nodes_rays, n: int, lift: float = 0.01):
    """(points, normals) float32 (n, 3): the first n finite hits of the oracle's closest form on `nodes_rays`, each moved
    `lift` along its world normal -- a point ON a surface starts its rays 1e-5 off it, inside the band in which the float64
    reference judges nothing."""
    o, d = nodes_rays
    near = io.closest(arrays, plan, o, d, 1e5)
    at = np.flatnonzero((near["distance"] < np.inf) & np.isfinite(near["normal"]).all(axis=1))[:n]
    normals = near["normal"][at]
    points = (near["position"][at].astype(np.float64) + lift * normals.astype(np.float64)).astype(np.float32)
    return np.ascontiguousarray(points), np.ascontiguousarray(normals)
