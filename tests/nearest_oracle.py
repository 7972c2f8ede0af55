"""ctypes view of tests/nearest_oracle.c (the brute-force CPU oracle of the closest-point queries, include/rt_hip_nearest.h),
compiled on first use with the oracle's flags into a private temporary directory."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from query_oracle import as4, same_words

HERE = os.path.dirname(os.path.abspath(__file__))
NONE = 0xFFFFFFFF
OUTPUTS = ("hit", "distance", "leaf", "barycentric", "position", "normal")
_LIB = None


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        out = os.path.join(tempfile.mkdtemp(prefix="ocrt_nearest_oracle_"), "libnearest_oracle.so")
        subprocess.run(["gcc", "-std=gnu11", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-fPIC", "-shared",
                        "-o", out, os.path.join(HERE, "nearest_oracle.c"), "-lm"], check=True)
        L = C.CDLL(out)
        p = C.c_void_p
        L.no_closest_points.argtypes = [p, C.c_uint32, p, p, p, C.c_uint32, C.c_float, p, p, p, p, p, p]
        L.no_closest_points.restype = None
        L.no_pair.argtypes = [p, p, C.c_uint32, p, p]
        L.no_pair.restype = None
        _LIB = L
    return _LIB


def closest_points(leaf_faces, vertices, normals, points, max_distance=np.inf) -> dict:
    """The contract's answer for every point: `leaf_faces` the leaf-ordered faces (3 ids per leaf: Scene.sorted_faces),
    `vertices` / `normals` (V, 3) or (V, 4).  {"hit", "distance", "leaf", "barycentric", "position", "normal"}."""
    f = np.ascontiguousarray(leaf_faces, dtype=np.uint32).reshape(-1)
    v4, n4, q4 = as4(vertices), as4(normals), as4(points)
    n = q4.shape[0]
    out = {"hit": np.zeros(n, np.uint8), "distance": np.zeros(n, np.float32), "leaf": np.zeros(n, np.uint32),
           "barycentric": np.zeros((n, 3), np.float32), "position": np.zeros((n, 3), np.float32),
           "normal": np.zeros((n, 3), np.float32)}
    lib().no_closest_points(f.ctypes.data, f.size // 3, v4.ctypes.data, n4.ctypes.data, q4.ctypes.data, n, float(max_distance),
                            *[out[k].ctypes.data for k in OUTPUTS])
    return out


def pair(leaf_faces, vertices, leaf: int, point) -> dict:
    """The per-leaf routine for one (point, leaf) pair: {"s", "t", "position" (3,), "d2"}, float32."""
    f = np.ascontiguousarray(leaf_faces, dtype=np.uint32).reshape(-1)
    v4 = as4(vertices)
    q = np.ascontiguousarray(point, dtype=np.float32)
    out = np.zeros(6, np.float32)
    lib().no_pair(f.ctypes.data, v4.ctypes.data, int(leaf), q.ctypes.data, out.ctypes.data)
    return {"s": out[0], "t": out[1], "position": out[2:5].copy(), "d2": out[5]}


def assert_same(got: dict, want: dict, what: str = "") -> None:
    """Every output word of `got` equals the oracle's."""
    for name in got:
        same = same_words(got[name], want[name])
        assert same.all(), (what, name, int((~same).sum()), np.argwhere(~same)[:4].tolist())
