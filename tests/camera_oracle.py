"""ctypes view of tests/camera_oracle.c (the CPU oracle of the posed camera), compiled on first use with the oracle's
flags into a private temporary directory."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import orc

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

DEFAULT_POSE = np.array([[0, 0, 2], [1, 0, 0], [0, 1, 0], [0, 0, -1]], dtype=np.float32)


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        out = os.path.join(tempfile.mkdtemp(prefix="ocrt_camera_oracle_"), "libcamera_oracle.so")
        subprocess.run(["gcc", "-std=gnu11", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-fPIC", "-shared",
                        "-o", out, os.path.join(HERE, "camera_oracle.c"), "-lm"], check=True)
        L = C.CDLL(out)
        L.co_render.restype = C.c_int
        L.co_render.argtypes = [C.POINTER(orc.OrcParams), C.POINTER(orc.OrcScene), C.c_void_p, C.c_void_p, C.POINTER(orc.OrcCounters)]
        _LIB = L
    return _LIB


def pose_array(pose) -> np.ndarray:
    """(4, 3) float32 -- eye, right, up, forward -- from such an array or from an opencl_raytracer_amd.Camera."""
    if hasattr(pose, "as_array"):
        pose = pose.as_array()
    a = np.ascontiguousarray(pose, dtype=np.float32)
    assert a.shape == (4, 3)
    return a


def render(params: orc.OrcParams, arrays: orc.SceneArrays, pose):
    """The frame from that pose: (float image H x W, counters dict)."""
    p = pose_array(pose)
    image = np.zeros((params.height, params.width), dtype=np.float32)
    counters = orc.OrcCounters()
    sc = arrays.c_struct()
    with np.errstate(all="ignore"):
        used = lib().co_render(C.byref(params), C.byref(sc), p.ctypes.data, image.ctypes.data, C.byref(counters))
    if used < 0:
        raise RuntimeError("camera oracle: AO direction table too large")
    return image, {k: int(getattr(counters, k)) for k, _ in orc.OrcCounters._fields_}
