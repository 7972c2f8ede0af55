"""ctypes view of tests/instance_oracle.c (the CPU oracle of the instanced ray queries, include/rt_hip_instances.h),
compiled on first use with the oracle's flags into a private temporary directory."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import orc
from query_oracle import NONE, as4, same_words  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("hit", "distance", "leaf", "barycentric", "position", "normal", "instance")
_LIB = None


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        out = os.path.join(tempfile.mkdtemp(prefix="ocrt_instance_oracle_"), "libinstance_oracle.so")
        subprocess.run(["gcc", "-std=gnu11", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-fPIC", "-shared",
                        "-o", out, os.path.join(HERE, "instance_oracle.c"), "-lm"], check=True)
        L = C.CDLL(out)
        S, p, u, f = C.POINTER(orc.OrcScene), C.c_void_p, C.c_uint32, C.c_float
        L.io_closest.argtypes = [S, p, u, p, p, p, u, f, p, p, p, p, p, p, p]
        L.io_occluded.argtypes = [S, p, u, p, p, p, u, f, p]
        for fn in (L.io_closest, L.io_occluded):
            fn.restype = None
        _LIB = L
    return _LIB


def _plan(plan):
    """(nodes, O) of a plan -- host.instances() or rt.instance_plan() -- as contiguous arrays."""
    nodes = np.ascontiguousarray(plan["nodes"])
    inverse = np.ascontiguousarray(plan["object_from_world"], np.float32)
    assert nodes.dtype.itemsize == 32 and len(nodes) == 2 * len(inverse) - 1
    return nodes, inverse


def closest(arrays, plan, origins, directions, max_distance) -> dict:
    nodes, inverse = _plan(plan)
    o4, d4 = as4(origins), as4(directions)
    n = o4.shape[0]
    out = {"hit": np.zeros(n, np.uint8), "distance": np.zeros(n, np.float32), "leaf": np.zeros(n, np.uint32),
           "barycentric": np.zeros((n, 3), np.float32), "position": np.zeros((n, 3), np.float32),
           "normal": np.zeros((n, 3), np.float32), "instance": np.zeros(n, np.uint32)}
    sc = arrays.c_struct()
    lib().io_closest(C.byref(sc), nodes.ctypes.data, len(nodes), inverse.ctypes.data, o4.ctypes.data, d4.ctypes.data, n,
                     float(max_distance), *[out[k].ctypes.data for k in FIELDS])
    return out


def occluded(arrays, plan, origins, directions, max_distance) -> np.ndarray:
    nodes, inverse = _plan(plan)
    o4, d4 = as4(origins), as4(directions)
    out = np.zeros(o4.shape[0], np.uint8)
    sc = arrays.c_struct()
    lib().io_occluded(C.byref(sc), nodes.ctypes.data, len(nodes), inverse.ctypes.data, o4.ctypes.data, d4.ctypes.data, o4.shape[0],
                      float(max_distance), out.ctypes.data)
    return out


def assert_same(got: dict, want: dict, what="") -> None:
    for f in got:
        ok = same_words(got[f], want[f])
        assert ok.all(), (what, f, int((~ok).sum()), np.argwhere(~ok)[:5].tolist())
