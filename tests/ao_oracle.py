"""ctypes view of tests/ao_oracle.c (the CPU oracle of the ambient-occlusion queries), compiled on first use with the
oracle's flags into a private temporary directory."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import orc
from query_oracle import as4

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        out = os.path.join(tempfile.mkdtemp(prefix="ocrt_ao_oracle_"), "libao_oracle.so")
        subprocess.run(["gcc", "-std=gnu11", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-fPIC", "-shared",
                        "-o", out, os.path.join(HERE, "ao_oracle.c"), "-lm"], check=True)
        L = C.CDLL(out)
        P, S, p = C.POINTER(orc.OrcParams), C.POINTER(orc.OrcScene), C.c_void_p
        L.aoo_ambient_occlusion.argtypes = [P, S, p, p, p, C.c_uint32, p, p]
        L.aoo_ambient_occlusion.restype = C.c_uint32
        _LIB = L
    return _LIB


def ambient_occlusion(params, arrays, points, normals, seeds=None) -> dict:
    """The oracle's ambient_occlusion at every point: {"ao": float32 (N,), "occluded": uint32 (N,), "rays": per point}.
    `params`: orc.OrcParams (ao_method, ao_num_samples, angles, ao_max_distance); seeds None: the point's index."""
    p4, n4 = as4(points), as4(normals)
    n = p4.shape[0]
    assert n4.shape[0] == n
    if seeds is not None:
        seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
        assert seeds.shape == (n,)
    ao, hits = np.zeros(n, np.float32), np.zeros(n, np.uint32)
    sc = arrays.c_struct()
    rays = lib().aoo_ambient_occlusion(C.byref(params), C.byref(sc), p4.ctypes.data, n4.ctypes.data,
                                       seeds.ctypes.data if seeds is not None else None, n, ao.ctypes.data, hits.ctypes.data)
    assert rays > 0, "ao oracle: no direction table"
    return {"ao": ao, "occluded": hits, "rays": int(rays)}
