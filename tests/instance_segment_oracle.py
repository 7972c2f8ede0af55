"""ctypes view of tests/instance_segment_oracle.c (the CPU oracle of the instanced segment queries,
include/rt_hip_instance_segments.h), compiled on first use with the oracle's flags into a private temporary directory.
Pair forms only: the mask form's expectation is `mask_of`, the occluded form on the pairs written out."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import orc
import segment_cases
from query_oracle import NONE, as4, same_words  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("hit", "distance", "leaf", "barycentric", "position", "normal", "instance")
_LIB = None


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        out = os.path.join(tempfile.mkdtemp(prefix="ocrt_instance_segment_oracle_"), "libinstance_segment_oracle.so")
        subprocess.run(["gcc", "-std=gnu11", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-fPIC", "-shared",
                        "-o", out, os.path.join(HERE, "instance_segment_oracle.c"), "-lm"], check=True)
        L = C.CDLL(out)
        S, p, u, f = C.POINTER(orc.OrcScene), C.c_void_p, C.c_uint32, C.c_float
        L.iso_closest.argtypes = [S, p, u, p, p, p, u, f, f, p, p, p, p, p, p, p]
        L.iso_occluded.argtypes = [S, p, u, p, p, p, u, f, f, p]
        for fn in (L.iso_closest, L.iso_occluded):
            fn.restype = None
        _LIB = L
    return _LIB


def _plan(plan):
    """(nodes, O) of a plan -- host.instances() or rt.instance_plan() -- as contiguous arrays."""
    nodes = np.ascontiguousarray(plan["nodes"])
    inverse = np.ascontiguousarray(plan["object_from_world"], np.float32)
    assert nodes.dtype.itemsize == 32 and len(nodes) == 2 * len(inverse) - 1
    return nodes, inverse


def closest(arrays, plan, a, b, interval) -> dict:
    nodes, inverse = _plan(plan)
    a4, b4 = as4(a), as4(b)
    n = a4.shape[0]
    out = {"hit": np.zeros(n, np.uint8), "distance": np.zeros(n, np.float32), "leaf": np.zeros(n, np.uint32),
           "barycentric": np.zeros((n, 3), np.float32), "position": np.zeros((n, 3), np.float32),
           "normal": np.zeros((n, 3), np.float32), "instance": np.zeros(n, np.uint32)}
    sc = arrays.c_struct()
    lib().iso_closest(C.byref(sc), nodes.ctypes.data, len(nodes), inverse.ctypes.data, a4.ctypes.data, b4.ctypes.data, n,
                      float(interval[0]), float(interval[1]), *[out[k].ctypes.data for k in FIELDS])
    return out


def occluded(arrays, plan, a, b, interval) -> np.ndarray:
    nodes, inverse = _plan(plan)
    a4, b4 = as4(a), as4(b)
    out = np.zeros(a4.shape[0], np.uint8)
    sc = arrays.c_struct()
    lib().iso_occluded(C.byref(sc), nodes.ctypes.data, len(nodes), inverse.ctypes.data, a4.ctypes.data, b4.ctypes.data, a4.shape[0],
                       float(interval[0]), float(interval[1]), out.ctypes.data)
    return out


def mask_of(arrays, plan, points, targets, interval) -> dict:
    """The mask form's expectation, derived from the occluded pair form on segment_cases.pairs_of(points, targets):
    {"mask": uint32 (P, W), "count": uint32 (P,), "flags": bool (P, T)}."""
    p, t = np.asarray(points), np.asarray(targets)
    flags = np.zeros((len(p), len(t)), bool)
    if len(p) and len(t):
        pa, pb = segment_cases.pairs_of(p, t)
        flags = occluded(arrays, plan, pa, pb, interval).reshape(len(p), len(t)).astype(bool)
    words = (len(t) + 31) // 32
    padded = np.zeros((len(p), words * 32), np.uint8)
    padded[:, :len(t)] = flags
    mask = np.packbits(padded.reshape(len(p), words, 32), axis=-1, bitorder="little").view(np.uint32).reshape(len(p), words)
    return {"mask": np.ascontiguousarray(mask), "count": flags.sum(axis=1).astype(np.uint32), "flags": flags}


def assert_same(got: dict, want: dict, what="") -> None:
    for f in got:
        ok = same_words(got[f], want[f])
        assert ok.all(), (what, f, int((~ok).sum()), np.argwhere(~ok)[:5].tolist())
