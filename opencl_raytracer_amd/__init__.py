"""MI355X-native ray-casting path behind the reference's render-host API.

The product is native code: ``csrc/`` builds ``lib/libocrt_hip.so`` (C ABI of
``include/rt_hip.h`` + the C++ ``HipHost`` class + gfx950 kernels) and the
``bin/render`` CLI.  This package is only the thin ctypes view of that C ABI
used by the tests and ``bench.py``; it contains no compute and no fallback --
if the shared library is missing, importing :mod:`opencl_raytracer_amd.api`
raises.
"""
from .api import (  # noqa: F401
    DIRECTIONAL_OUTPUTS,
    INSTANCE_MULTIHIT_OUTPUTS,
    INSTANCE_NODE,
    INSTANCE_OUTPUTS,
    INSTANCE_VIEW_OUTPUTS,
    LAYER_OUTPUTS,
    NEAREST_OUTPUTS,
    SIGNED_OUTPUTS,
    FEATURES,
    SIGN_RECORD,
    SEGMENT_INTERVAL,
    SEGMENT_OUTPUTS,
    VIEW_OUTPUTS,
    VISIBILITY_OUTPUTS,
    Camera,
    FrameRing,
    Host,
    Options,
    RtError,
    Scene,
    device_count,
    lib_path,
    load_library,
    node_test_forms,
    partition_rows,
    pgm_bytes,
    rccl_available,
    rccl_unique_id,
    instance_plan,
    instance_plan_lbvh,
    resize_cpu,
    unpack_ao_mask,
    unpack_visibility_mask,
)
