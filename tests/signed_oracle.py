"""ctypes view of tests/signed_oracle.c (the brute-force CPU oracle of the signed distance queries, include/rt_hip_signed.h),
compiled on first use with the oracle's flags into a private temporary directory."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from query_oracle import as4, same_words

HERE = os.path.dirname(os.path.abspath(__file__))
NONE = 0xFFFFFFFF
RECORD = ("hit", "distance", "leaf", "barycentric", "position", "normal")
OUTPUTS = RECORD + ("feature", "pseudonormal")
FACE, VERTEX_A, VERTEX_B, VERTEX_C, EDGE_AB, EDGE_AC, EDGE_BC, NO_FEATURE = 0, 1, 2, 3, 4, 5, 6, 0xFF
FLAGS = ["-std=gnu11", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-fPIC", "-shared"]
_LIB = None


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        out = os.path.join(tempfile.mkdtemp(prefix="ocrt_signed_oracle_"), "libsigned_oracle.so")
        subprocess.run(["gcc"] + FLAGS + ["-o", out, os.path.join(HERE, "signed_oracle.c"), "-lm"], check=True)
        L = C.CDLL(out)
        p = C.c_void_p
        L.so_table.argtypes = [p, C.c_uint32, p, C.c_uint32, p]
        L.so_table.restype = C.c_int
        L.so_angle.argtypes = [p, p]
        L.so_angle.restype = C.c_float
        L.so_signed_distance.argtypes = [p, C.c_uint32, p, p, p, p, C.c_uint32, C.c_float] + [p] * 8
        L.so_signed_distance.restype = None
        _LIB = L
    return _LIB


def table(leaf_faces, vertices) -> np.ndarray:
    """The sign table of the leaf-ordered faces: float32 (leaves, 6, 4) -- edges AB, AC, BC, vertices A, B, C."""
    f = np.ascontiguousarray(leaf_faces, dtype=np.uint32).reshape(-1)
    v4 = as4(vertices)
    out = np.zeros((f.size // 3, 6, 4), np.float32)
    assert lib().so_table(f.ctypes.data, f.size // 3, v4.ctypes.data, v4.shape[0], out.ctypes.data) == 0
    return out


def angle(a, b) -> np.float32:
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return np.float32(lib().so_angle(a.ctypes.data, b.ctypes.data))


def signed_distance(leaf_faces, vertices, normals, points, max_distance=np.inf, sign_table=None) -> dict:
    """The contract's answer for every point; the arguments are nearest_oracle.closest_points'.  {"hit", "distance" (signed),
    "leaf", "barycentric", "position", "normal", "feature", "pseudonormal" (N, 4)}."""
    f = np.ascontiguousarray(leaf_faces, dtype=np.uint32).reshape(-1)
    v4, n4, q4 = as4(vertices), as4(normals), as4(points)
    t = table(f, v4) if sign_table is None else np.ascontiguousarray(sign_table, np.float32)
    n = q4.shape[0]
    out = {"hit": np.zeros(n, np.uint8), "distance": np.zeros(n, np.float32), "leaf": np.zeros(n, np.uint32),
           "barycentric": np.zeros((n, 3), np.float32), "position": np.zeros((n, 3), np.float32),
           "normal": np.zeros((n, 3), np.float32), "feature": np.zeros(n, np.uint8), "pseudonormal": np.zeros((n, 4), np.float32)}
    lib().so_signed_distance(f.ctypes.data, f.size // 3, v4.ctypes.data, n4.ctypes.data, t.ctypes.data, q4.ctypes.data, n,
                             float(max_distance), *[out[k].ctypes.data for k in OUTPUTS])
    return out


def assert_same(got: dict, want: dict, what: str = "") -> None:
    """Every output word of `got` equals the oracle's."""
    for name in got:
        same = same_words(got[name], want[name])
        assert same.all(), (what, name, int((~same).sum()), np.argwhere(~same)[:4].tolist())
