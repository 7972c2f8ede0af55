"""ctypes view of tests/query_oracle.c (the CPU oracle of the ray queries), compiled on first use with the oracle's
flags into a private temporary directory."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import orc

HERE = os.path.dirname(os.path.abspath(__file__))
NONE = 0xFFFFFFFF
_LIB = None


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        out = os.path.join(tempfile.mkdtemp(prefix="ocrt_query_oracle_"), "libquery_oracle.so")
        subprocess.run(["gcc", "-std=gnu11", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-fPIC", "-shared",
                        "-o", out, os.path.join(HERE, "query_oracle.c"), "-lm"], check=True)
        L = C.CDLL(out)
        P, S, p = C.POINTER(orc.OrcParams), C.POINTER(orc.OrcScene), C.c_void_p
        L.qo_closest.argtypes = [S, p, p, C.c_uint32, C.c_float, p, p, p, p, p, p]
        L.qo_any.argtypes = [S, p, p, C.c_uint32, C.c_float, p]
        L.qo_camera_rays.argtypes = [P, p, p]
        L.qo_shade.argtypes = [p, p, p, C.c_uint32, C.c_int, p]
        for f in (L.qo_closest, L.qo_any, L.qo_camera_rays, L.qo_shade):
            f.restype = None
        _LIB = L
    return _LIB


def as4(a) -> np.ndarray:
    a = np.asarray(a, dtype=np.float32)
    if a.shape[1] == 4:
        return np.ascontiguousarray(a)
    out = np.zeros((a.shape[0], 4), dtype=np.float32)
    out[:, :3] = a
    return out


def closest(arrays, origins, directions, max_distance: float) -> dict:
    o4, d4 = as4(origins), as4(directions)
    n = o4.shape[0]
    out = {"hit": np.zeros(n, np.uint8), "distance": np.zeros(n, np.float32), "leaf": np.zeros(n, np.uint32),
           "barycentric": np.zeros((n, 3), np.float32), "position": np.zeros((n, 3), np.float32),
           "normal": np.zeros((n, 3), np.float32)}
    sc = arrays.c_struct()
    lib().qo_closest(C.byref(sc), o4.ctypes.data, d4.ctypes.data, n, float(max_distance),
                     *[out[k].ctypes.data for k in ("hit", "distance", "leaf", "barycentric", "position", "normal")])
    return out


def occluded(arrays, origins, directions, max_distance: float) -> np.ndarray:
    o4, d4 = as4(origins), as4(directions)
    out = np.zeros(o4.shape[0], np.uint8)
    sc = arrays.c_struct()
    lib().qo_any(C.byref(sc), o4.ctypes.data, d4.ctypes.data, o4.shape[0], float(max_distance), out.ctypes.data)
    return out


def camera_rays(params):
    n = params.width * params.height
    o4, d4 = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    lib().qo_camera_rays(C.byref(params), o4.ctypes.data, d4.ctypes.data)
    return o4, d4


def shade(hit, normal, directions, shading: bool) -> np.ndarray:
    d4 = as4(directions)
    hit = np.ascontiguousarray(hit, np.uint8)
    normal = np.ascontiguousarray(normal, np.float32)
    out = np.zeros(d4.shape[0], np.float32)
    lib().qo_shade(hit.ctypes.data, normal.ctypes.data, d4.ctypes.data, d4.shape[0], int(bool(shading)), out.ctypes.data)
    return out


def same_words(a, b) -> np.ndarray:
    """Elementwise: the same bits, or both NaN (a NaN's payload is the platform's)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    return a == b
