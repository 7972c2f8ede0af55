"""ctypes view of tests/layers_oracle.c (the CPU oracle of the frame layers), compiled on first use with the oracle's
flags into a private temporary directory."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import orc
from camera_oracle import pose_array

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

# name -> (dtype, values per sub-pixel), in the order of lo_layers (and of rt_layer_arrays)
LAYERS = (("hit", np.uint8, 1), ("distance", np.float32, 1), ("leaf", np.uint32, 1), ("barycentric", np.float32, 3),
          ("position", np.float32, 3), ("normal", np.float32, 3), ("direction", np.float32, 3), ("shade", np.float32, 1),
          ("ao", np.float32, 1), ("value", np.float32, 1))
NAMES = tuple(name for name, _, _ in LAYERS)
RECORD = NAMES[:6]


class _Layers(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in NAMES]


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        out = os.path.join(tempfile.mkdtemp(prefix="ocrt_layers_oracle_"), "liblayers_oracle.so")
        subprocess.run(["gcc", "-std=gnu11", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-fPIC", "-shared",
                        "-o", out, os.path.join(HERE, "layers_oracle.c"), "-lm"], check=True)
        L = C.CDLL(out)
        L.lo_render.restype = C.c_int
        L.lo_render.argtypes = [C.POINTER(orc.OrcParams), C.POINTER(orc.OrcScene), C.c_void_p, C.POINTER(_Layers)]
        _LIB = L
    return _LIB


def render(params: orc.OrcParams, arrays: orc.SceneArrays, pose=None) -> dict:
    """Every layer of the frame, {name: (H, W) or (H, W, 3)}; pose None: the reference's camera (a host without a pose)."""
    h, w = params.height, params.width
    out = {name: np.zeros((h, w) + ((per,) if per > 1 else ()), dtype=dtype) for name, dtype, per in LAYERS}
    p = None if pose is None else pose_array(pose)
    sc = arrays.c_struct()
    layers = _Layers(*[out[name].ctypes.data for name in NAMES])
    with np.errstate(all="ignore"):
        used = lib().lo_render(C.byref(params), C.byref(sc), None if p is None else p.ctypes.data, C.byref(layers))
    if used < 0:
        raise RuntimeError("layers oracle: AO direction table too large")
    return out


def same_words(a, b) -> np.ndarray:
    """Elementwise: the same bits, or both NaN (a NaN's payload is the platform's)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    return a == b
