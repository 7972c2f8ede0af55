"""ctypes view of tests/directional_oracle.c (the CPU oracle of the directional occlusion queries), compiled on first use
with the oracle's flags into a private temporary directory."""
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
        out = os.path.join(tempfile.mkdtemp(prefix="ocrt_directional_oracle_"), "libdirectional_oracle.so")
        subprocess.run(["gcc", "-std=gnu11", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-fPIC", "-shared",
                        "-o", out, os.path.join(HERE, "directional_oracle.c"), "-lm"], check=True)
        L = C.CDLL(out)
        P, S, p = C.POINTER(orc.OrcParams), C.POINTER(orc.OrcScene), C.c_void_p
        L.dro_rays_per_point.argtypes = [P]
        L.dro_rays_per_point.restype = C.c_uint32
        L.dro_directional.argtypes = [P, S, p, p, p, C.c_uint32, p, p, p, p]
        L.dro_directional.restype = C.c_uint32
        _LIB = L
    return _LIB


def directional(params, arrays, points, normals, seeds=None) -> dict:
    """Per point what the oracle's ambient_occlusion casts and finds: {"rays": R, "origins": float32 (N, 3), "directions":
    float32 (N, R, 3), "mask": uint32 (N, ceil(R / 32)), "bent": float32 (N, 3), and -- made of the mask as the contract
    says -- "occluded": uint32 (N,), "ao": float32 (N,)}.  `params`: orc.OrcParams; seeds None: the point's index."""
    p4, n4 = as4(points), as4(normals)
    n = p4.shape[0]
    assert n4.shape[0] == n
    if seeds is not None:
        seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
        assert seeds.shape == (n,)
    rays = int(lib().dro_rays_per_point(C.byref(params)))
    assert rays > 0, "directional oracle: no direction table"
    words = (rays + 31) // 32
    origins, dirs = np.zeros((n, 3), np.float32), np.zeros((n, rays, 3), np.float32)
    mask, bent = np.zeros((n, words), np.uint32), np.zeros((n, 3), np.float32)
    sc = arrays.c_struct()
    got = lib().dro_directional(C.byref(params), C.byref(sc), p4.ctypes.data, n4.ctypes.data,
                                seeds.ctypes.data if seeds is not None else None, n, origins.ctypes.data, dirs.ctypes.data,
                                mask.ctypes.data, bent.ctypes.data)
    assert got == rays, (got, rays)
    occluded = popcount(mask)
    divisor = rays if params.ao_method == 0 else params.ao_num_samples + 1
    ao = np.float32(1.0) - occluded.astype(np.float32) / np.float32(divisor)
    return {"rays": rays, "origins": origins, "directions": dirs, "mask": mask, "bent": bent, "occluded": occluded,
            "ao": ao.astype(np.float32)}


def popcount(mask: np.ndarray) -> np.ndarray:
    """Set bits per row of uint32 (N, W): uint32 (N,)."""
    return np.unpackbits(np.ascontiguousarray(mask).view(np.uint8), axis=1).sum(axis=1, dtype=np.uint32)


def ordered_sum(directions: np.ndarray, open_rays: np.ndarray) -> np.ndarray:
    """float32 (N, 3): starting from +0, b = b + directions[:, k] for k = 0, 1, ... over the rays with open_rays[:, k]."""
    b = np.zeros((directions.shape[0], 3), np.float32)
    with np.errstate(all="ignore"):
        for k in range(directions.shape[1]):
            b = np.where(open_rays[:, k, None], b + directions[:, k, :3], b).astype(np.float32)
    return b
