"""ctypes view of tests/instance_nearest_oracle.c (the brute-force CPU oracle of the instanced closest-point queries,
include/rt_hip_instance_nearest.h), compiled on first use with the oracle's flags into a private temporary directory."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from query_oracle import as4, same_words

HERE = os.path.dirname(os.path.abspath(__file__))
NONE = 0xFFFFFFFF
OUTPUTS = ("hit", "distance", "leaf", "barycentric", "position", "normal", "instance")
_LIB = None


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        out = os.path.join(tempfile.mkdtemp(prefix="ocrt_instance_nearest_oracle_"), "libinstance_nearest_oracle.so")
        subprocess.run(["gcc", "-std=gnu11", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-fPIC", "-shared",
                        "-o", out, os.path.join(HERE, "instance_nearest_oracle.c"), "-lm"], check=True)
        L = C.CDLL(out)
        p, u = C.c_void_p, C.c_uint32
        L.ino_closest_points.argtypes = [p, u, p, p, p, p, u, p, u, C.c_float, p, p, p, p, p, p, p]
        L.ino_closest_points.restype = None
        _LIB = L
    return _LIB


def closest_points(leaf_faces, vertices, normals, world_from_object, object_from_world, points, max_distance=np.inf) -> dict:
    """The contract's answer for every point: `leaf_faces` the leaf-ordered faces (3 ids per leaf), `vertices` / `normals`
    (V, 3) or (V, 4), the transforms as given and their inverses by the header's formula ((n, 3, 4) float32 each:
    host.instances() or rt.instance_plan()).  {"hit", "distance", "leaf", "barycentric", "position", "normal", "instance"}."""
    f = np.ascontiguousarray(leaf_faces, dtype=np.uint32).reshape(-1)
    v4, n4, q4 = as4(vertices), as4(normals), as4(points)
    W = np.ascontiguousarray(world_from_object, np.float32).reshape(-1, 12)
    O = np.ascontiguousarray(object_from_world, np.float32).reshape(-1, 12)
    assert W.shape == O.shape and len(W) >= 1
    n = q4.shape[0]
    out = {"hit": np.zeros(n, np.uint8), "distance": np.zeros(n, np.float32), "leaf": np.zeros(n, np.uint32),
           "barycentric": np.zeros((n, 3), np.float32), "position": np.zeros((n, 3), np.float32),
           "normal": np.zeros((n, 3), np.float32), "instance": np.zeros(n, np.uint32)}
    lib().ino_closest_points(f.ctypes.data, f.size // 3, v4.ctypes.data, n4.ctypes.data, W.ctypes.data, O.ctypes.data, len(W),
                             q4.ctypes.data, n, float(max_distance), *[out[k].ctypes.data for k in OUTPUTS])
    return out


def assert_same(got: dict, want: dict, what="") -> None:
    """Every output word of `got` equals the oracle's."""
    for name in got:
        same = same_words(got[name], want[name])
        assert same.all(), (what, name, int((~same).sum()), np.argwhere(~same)[:4].tolist())
