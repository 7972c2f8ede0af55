"""A BVH-free float64 reference for the instanced closest-point queries (include/rt_hip_instance_nearest.h).  It shares no
line with the library: every copy's vertices are W v in float64, its vertex normals go through np.linalg.inv of W's linear
part, the copies are MERGED into one mesh, and the merged mesh and the answer -- its (instance, leaf) mapped to a merged face
-- are handed to the plain queries' reference and comparator (tests/distance_reference.py: pair_distances, compare).

MEASURED: the worst scaled difference between the C oracle (tests/instance_nearest_oracle.c) and this reference over the CPU
cases of tests/test_instance_nearest_cpu.py, per check; TOL = 8 x MEASURED, the project's rule.
"""
import numpy as np

import distance_reference as ref

# check -> worst scaled difference measured (tests/test_instance_nearest_cpu.py::test_oracle_against_the_reference prints them)
MEASURED = {
    # (b): `ties` once more, the query at the apex of its sliver (tests/distance_reference.py has the story): the routine is
    # the plain one, and so is its worst case, under every family.
    "distance": 1.01e-5,
    "leaf": 1.2e-7,         # (c)
    "position": 4.2e-7,     # (d)
    "barycentric": 6.0e-8,  # (e)
    "consistency": 1.2e-7,  # (f)
    "normal": 1.7e-7,       # (g): the normal goes through the binary32 inverse (`shear`: entries rounded once, a condition of 8)
}
TOL = {k: 8.0 * v for k, v in MEASURED.items()}


def merged_mesh(vertices, vnormals, faces, world_from_object):
    """(vertices (n V, 3), normals (n V, 3), faces (n F, 3)) of the copies, float64, copy k's block behind copy k - 1's."""
    v = np.asarray(vertices, dtype=np.float64)[:, :3]
    vn = np.asarray(vnormals, dtype=np.float64)[:, :3]
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    W = np.asarray(world_from_object, dtype=np.float64).reshape(-1, 3, 4)
    vs, ns, fs = [], [], []
    for k, w in enumerate(W):
        A, t = w[:, :3], w[:, 3]
        vs.append(v @ A.T + t)
        ns.append(vn @ np.linalg.inv(A))  # transpose(inverse(A)) n, row by row
        fs.append(f + k * len(v))
    return np.concatenate(vs), np.concatenate(ns), np.concatenate(fs)


def pair_distances(points, vertices, faces, world_from_object) -> np.ndarray:
    """float64 (N, n F): the distance from every point to every face of every copy."""
    mv, _, mf = merged_mesh(vertices, vertices, faces, world_from_object)
    return ref.pair_distances(points, mv, mf)


def compare(points, vertices, vnormals, faces, face_of_leaf, world_from_object, max_distance, answer: dict, tol: dict = None, pairs=None) -> dict:
    """Holds `answer` ({"hit", "distance", "leaf", "barycentric", "position", "normal", "instance"}) against the reference:
    distance_reference.compare's checks on the merged mesh, and `instance` 0xFFFFFFFF exactly where nothing was found.
    Returns {"violations": [...], "measured": {check: worst scaled difference}}."""
    mv, mn, mf = merged_mesh(vertices, vnormals, faces, world_from_object)
    face_of_leaf = np.asarray(face_of_leaf, dtype=np.int64)
    leaves, count = len(face_of_leaf), len(np.asarray(world_from_object).reshape(-1, 12))
    merged_face_of_leaf = np.concatenate([face_of_leaf + k * leaves for k in range(count)])  # (F faces = F leaves per copy)
    hit = np.asarray(answer["hit"]).astype(bool)
    instance = np.asarray(answer["instance"]).astype(np.int64)
    violations = []
    if ((instance == 0xFFFFFFFF) != ~hit).any():
        violations.append("(a) `instance` is 0xFFFFFFFF where something was found, or an index where nothing was")
    if (instance[hit] >= count).any():
        violations.append("(c) an instance index beyond the set")
        return {"violations": violations, "measured": {k: 0.0 for k in MEASURED}}
    plain = {k: answer[k] for k in ("hit", "distance", "leaf", "barycentric", "position", "normal")}
    leaf = np.asarray(answer["leaf"]).astype(np.int64)
    plain["leaf"] = np.where(hit & (leaf < leaves), instance * leaves + leaf, 0xFFFFFFFF).astype(np.uint32)
    if (hit & (leaf >= leaves)).any():
        violations.append("(c) a leaf index beyond the scene's leaves")
    held = ref.compare(points, mv, mn, mf, merged_face_of_leaf, max_distance, plain, tol=TOL if tol is None else tol, pairs=pairs)
    return {"violations": violations + held["violations"], "measured": held["measured"]}
