"""ctypes view of tests/segment_oracle.c (the CPU oracle of the segment queries, include/rt_hip_segment.h), compiled on first
use with the oracle's flags into a private temporary directory."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import orc
from query_oracle import NONE, as4, same_words  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("hit", "distance", "leaf", "barycentric", "position", "normal")
_LIB = None


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        out = os.path.join(tempfile.mkdtemp(prefix="ocrt_segment_oracle_"), "libsegment_oracle.so")
        subprocess.run(["gcc", "-std=gnu11", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-fPIC", "-shared",
                        "-o", out, os.path.join(HERE, "segment_oracle.c"), "-lm"], check=True)
        L = C.CDLL(out)
        S, p, u, f = C.POINTER(orc.OrcScene), C.c_void_p, C.c_uint32, C.c_float
        L.so_closest.argtypes = [S, p, p, u, f, f, p, p, p, p, p, p]
        L.so_occluded.argtypes = [S, p, p, u, f, f, p]
        L.so_visibility.argtypes = [S, p, u, p, u, f, f, p, p]
        for fn in (L.so_closest, L.so_occluded, L.so_visibility):
            fn.restype = None
        _LIB = L
    return _LIB


def closest(arrays, a, b, interval) -> dict:
    a4, b4 = as4(a), as4(b)
    n = a4.shape[0]
    out = {"hit": np.zeros(n, np.uint8), "distance": np.zeros(n, np.float32), "leaf": np.zeros(n, np.uint32),
           "barycentric": np.zeros((n, 3), np.float32), "position": np.zeros((n, 3), np.float32),
           "normal": np.zeros((n, 3), np.float32)}
    sc = arrays.c_struct()
    lib().so_closest(C.byref(sc), a4.ctypes.data, b4.ctypes.data, n, float(interval[0]), float(interval[1]),
                     *[out[k].ctypes.data for k in FIELDS])
    return out


def occluded(arrays, a, b, interval) -> np.ndarray:
    a4, b4 = as4(a), as4(b)
    out = np.zeros(a4.shape[0], np.uint8)
    sc = arrays.c_struct()
    lib().so_occluded(C.byref(sc), a4.ctypes.data, b4.ctypes.data, a4.shape[0], float(interval[0]), float(interval[1]), out.ctypes.data)
    return out


def visibility(arrays, points, targets, interval) -> dict:
    p4, t4 = as4(points), as4(targets)
    np_, nt = p4.shape[0], t4.shape[0]
    out = {"mask": np.zeros((np_, (nt + 31) // 32), np.uint32), "count": np.zeros(np_, np.uint32)}
    sc = arrays.c_struct()
    lib().so_visibility(C.byref(sc), p4.ctypes.data, np_, t4.ctypes.data, nt, float(interval[0]), float(interval[1]),
                        out["mask"].ctypes.data, out["count"].ctypes.data)
    return out


def assert_same(got: dict, want: dict, what="") -> None:
    for f in got:
        ok = same_words(got[f], want[f])
        assert ok.all(), (what, f, int((~ok).sum()), np.argwhere(~ok)[:5].tolist())
