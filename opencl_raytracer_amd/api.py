"""ctypes binding of include/rt_hip.h, rt_hip_ring.h, rt_hip_debug.h, rt_hip_query.h, rt_hip_multihit.h, rt_hip_ao.h,
rt_hip_nearest.h, rt_hip_segment.h, rt_hip_instances.h, rt_hip_instance_build.h, rt_hip_instance_segments.h, rt_hip_instance_views.h, rt_hip_instance_multihit.h, rt_hip_instance_directional.h, rt_hip_directional.h, rt_hip_layers.h, rt_hip_views.h, rt_hip_update.h and rt_hip_camera.h (see those headers
for the contract)."""
from __future__ import annotations

import ctypes as C
import weakref
import os
import sys
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


def lib_path() -> str:
    """lib/libocrt_hip.so; OCRT_LIB_DIR (debug knob) names another directory of this package holding a build of
    the same library, e.g. lib_stamps for the instrumented one (make EXTRA_DEFS=-DOCRT_STAMPS LIBDIR=...)."""
    return os.path.join(_HERE, os.environ.get("OCRT_LIB_DIR", "lib"), "libocrt_hip.so")


class RtError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"[rt {code}] {message}")
        self.code = code
        self.message = message


RT_E_INVALID, RT_E_NO_DEVICE, RT_E_DEVICE, RT_E_STATE, RT_E_IO = -1, -2, -3, -4, -5


class Options(C.Structure):
    """rt_options == RayTracer::Options (reference include/ray_tracer.h:17-30)."""

    _fields_ = [
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("focal_length", C.c_float),
        ("n_super_samples", C.c_uint32),
        ("enable_shading", C.c_int32),
        ("enable_ao", C.c_int32),
        ("ao_max_distance", C.c_float),
        ("ao_num_samples", C.c_uint32),
        ("ao_method", C.c_int32),
        ("ao_alpha_min", C.c_int32),
        ("ao_alpha_max", C.c_int32),
        ("bvh_method", C.c_int32),
    ]

    @classmethod
    def defaults(cls, **overrides) -> "Options":
        o = cls()
        load_library().rt_options_default(C.byref(o))
        for k, v in overrides.items():
            if not hasattr(o, k):
                raise AttributeError(k)
            setattr(o, k, v)
        # the CLI's rule: AO is on iff the sample count is non-zero (reference src/render.cc:42)
        if "ao_num_samples" in overrides and "enable_ao" not in overrides:
            o.enable_ao = int(o.ao_num_samples != 0)
        return o

    @property
    def total_width(self) -> int:
        return load_library().rt_total_width(C.byref(self))

    @property
    def total_height(self) -> int:
        return load_library().rt_total_height(C.byref(self))


class _Stats(C.Structure):
    _fields_ = [
        ("primary_rays", C.c_uint64),
        ("primary_hits", C.c_uint64),
        ("ao_rays", C.c_uint64),
        ("ao_occluded", C.c_uint64),
    ]


class Camera(C.Structure):
    """rt_camera (include/rt_hip_camera.h): eye, right, up, forward -- four float triples, used as given."""

    _fields_ = [("eye", C.c_float * 3), ("right", C.c_float * 3), ("up", C.c_float * 3), ("forward", C.c_float * 3)]

    @classmethod
    def default(cls) -> "Camera":
        """The reference's camera: eye (0, 0, 2), right (1, 0, 0), up (0, 1, 0), forward (0, 0, -1)."""
        c = cls()
        load_library().rt_camera_default(C.byref(c))
        return c

    @classmethod
    def look_at(cls, eye, target, up=(0.0, 1.0, 0.0)) -> "Camera":
        """An orthonormal, right-handed pose at `eye` looking at `target` (rt_camera_look_at); RtError -1 where there is none."""
        c = cls()
        _check(load_library().rt_camera_look_at((C.c_float * 3)(*eye), (C.c_float * 3)(*target), (C.c_float * 3)(*up), C.byref(c)))
        return c

    @classmethod
    def from_vectors(cls, eye, right, up, forward) -> "Camera":
        """The four triples as given (float32): nothing is normalised or checked."""
        c = cls()
        for name, v in (("eye", eye), ("right", right), ("up", up), ("forward", forward)):
            setattr(c, name, (C.c_float * 3)(*np.asarray(v, dtype=np.float32).tolist()))
        return c

    def as_array(self) -> np.ndarray:
        """(4, 3) float32: eye, right, up, forward."""
        return np.frombuffer(bytes(self), dtype=np.float32).reshape(4, 3).copy()


_LIB: Optional[C.CDLL] = None

# name -> (restype, argtypes); also the list tests check against the header.
_SIGNATURES = {
    "rt_last_error": (C.c_char_p, []),
    "rt_last_error_code": (C.c_int, []),
    "rt_options_default": (None, [C.POINTER(Options)]),
    "rt_total_width": (C.c_uint32, [C.POINTER(Options)]),
    "rt_total_height": (C.c_uint32, [C.POINTER(Options)]),
    "rt_resize_cpu": (C.c_int, [C.POINTER(Options), C.c_void_p, C.c_void_p]),
    "rt_scene_load_off": (C.c_void_p, [C.c_char_p]),
    "rt_scene_from_arrays": (C.c_void_p, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]),
    "rt_scene_free": (None, [C.c_void_p]),
    "rt_scene_num_vertices": (C.c_uint32, [C.c_void_p]),
    "rt_scene_num_faces": (C.c_uint32, [C.c_void_p]),
    "rt_scene_build_bvh": (C.c_int, [C.c_void_p, C.c_int]),
    "rt_scene_num_nodes": (C.c_uint32, [C.c_void_p]),
    "rt_scene_vertices": (C.c_void_p, [C.c_void_p]),
    "rt_scene_vnormals": (C.c_void_p, [C.c_void_p]),
    "rt_scene_faces": (C.c_void_p, [C.c_void_p]),
    "rt_scene_nodes": (C.c_void_p, [C.c_void_p]),
    "rt_scene_aabbs": (C.c_void_p, [C.c_void_p]),
    "rt_scene_triangles": (C.c_void_p, [C.c_void_p]),
    "rt_scene_sorted_faces": (C.c_void_p, [C.c_void_p]),
    "rt_create": (C.c_void_p, [C.POINTER(Options)]),
    "rt_create_on": (C.c_void_p, [C.POINTER(Options), C.c_int, C.c_uint32, C.c_uint32]),
    "rt_destroy": (None, [C.c_void_p]),
    "rt_upload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                            C.c_uint32, C.c_void_p]),
    "rt_upload_scene": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rt_render": (C.c_int, [C.c_void_p]),
    "rt_render_async": (C.c_int, [C.c_void_p]),
    "rt_sync": (C.c_int, [C.c_void_p]),
    "rt_download": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rt_download_u8": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rt_local_rows": (C.c_uint32, [C.c_void_p]),
    "rt_download_u8_local": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rt_local_to_global_row": (C.c_uint32, [C.c_void_p, C.c_uint32]),
    "rt_partition_local_rows": (C.c_uint32, [C.POINTER(Options), C.c_uint32, C.c_uint32]),
    "rt_partition_global_row": (C.c_uint32, [C.POINTER(Options), C.c_uint32, C.c_uint32, C.c_uint32]),
    "rt_resize_into_device": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rt_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rt_use_private_stream": (C.c_int, [C.c_void_p]),
    "rt_get_stream": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "rt_set_device_share": (C.c_int, [C.c_void_p, C.c_uint]),
    "rt_expect_frames": (C.c_int, [C.c_void_p, C.c_uint64]),
    "rt_get_stats": (C.c_int, [C.c_void_p, C.POINTER(_Stats)]),
    "rt_last_kernel_ms": (C.c_float, [C.c_void_p]),
    "rt_total_kernel_ms": (C.c_double, [C.c_void_p]),
    "rt_last_ao_ms": (C.c_float, [C.c_void_p]),
    "rt_total_ao_ms": (C.c_double, [C.c_void_p]),
    "rt_kernel_launches": (C.c_uint64, [C.c_void_p]),
    "rt_reset_timers": (None, [C.c_void_p]),
    "rt_ring_create": (C.c_void_p, [C.POINTER(Options), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32]),
    "rt_ring_destroy": (None, [C.c_void_p]),
    "rt_ring_upload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                 C.c_uint32, C.c_void_p]),
    "rt_ring_upload_scene": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rt_ring_device_bytes": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "rt_ring_set_gather_timeout": (C.c_int, [C.c_void_p, C.c_double]),
    "rt_ring_rccl_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "rt_ring_set_calibration": (C.c_int, [C.c_void_p, C.c_int]),
    "rt_ring_calibration": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "rt_set_ao_prefetch": (C.c_int, [C.c_void_p, C.c_int]),
    "rt_walk_entries": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_double),
                        C.POINTER(C.c_double)]),
    "rt_ring_size": (C.c_uint32, [C.c_void_p]),
    "rt_ring_slots": (C.c_uint32, [C.c_void_p]),
    "rt_ring_local_rows": (C.c_uint32, [C.c_void_p]),
    "rt_ring_in_flight": (C.c_uint32, [C.c_void_p]),
    "rt_ring_host": (C.c_void_p, [C.c_void_p, C.c_uint32]),
    "rt_ring_set_graph_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "rt_ring_set_pacing": (C.c_int, [C.c_void_p, C.c_float]),
    "rt_ring_bind_output": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "rt_ring_submit": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "rt_ring_collect": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_void_p)]),
    "rt_ring_collect_into_device": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rt_ring_step": (C.c_int, [C.c_void_p]),
    "rt_ring_run": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rt_ring_drain": (C.c_int, [C.c_void_p]),
    "rt_ring_last_image_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "rt_ring_download_last": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rt_ring_reset_clock": (C.c_int, [C.c_void_p]),
    "rt_ring_keep_frame_times": (C.c_int, [C.c_void_p, C.c_int]),
    "rt_ring_frame_times": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_float)]),
    "rt_ring_timers": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_double),
                                 C.POINTER(C.c_uint64)]),
    "rt_ring_reset_timers": (None, [C.c_void_p]),
    "rt_ring_cpu_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                    C.POINTER(C.c_uint64)]),
    "rt_rccl_available": (C.c_int, []),
    "rt_rccl_unique_id": (C.c_int, [C.c_void_p]),
    "rt_ring_attach_rccl": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rt_ring_rccl_self_test": (C.c_int, [C.c_void_p]),
    "rt_print_info": (None, []),
    "rt_device_count": (C.c_int, []),
    # include/rt_hip_debug.h
    "rt_debug_measure_tile_costs": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int]),
    "rt_debug_set_order_policy": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_float]),
    "rt_debug_set_primary_split": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rt_debug_tile_order_slots": (C.c_uint32, [C.c_void_p]),
    "rt_debug_tiles": (C.c_uint32, [C.c_void_p]),
    "rt_debug_tile_order": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_debug_set_tile_order": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "rt_debug_split_tiles": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rt_debug_set_cheap_claims": (C.c_int, [C.c_void_p, C.c_float]),
    "rt_debug_cheap_tiles": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rt_debug_prune_facts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_debug_walk_interval_ends": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rt_debug_poison_hit_list": (C.c_int, [C.c_void_p]),
    "rt_debug_node_test_forms": (C.c_int, [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]),
    "rt_debug_set_views_chunk": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rt_debug_last_views": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    # include/rt_hip_query.h
    "rt_trace_closest": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.c_void_p]),
    "rt_trace_occluded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.c_void_p]),
    "rt_trace_closest_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.c_void_p,
                                          C.c_void_p]),
    "rt_trace_occluded_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.c_void_p,
                                           C.c_void_p]),
    "rt_last_query_ms": (C.c_float, [C.c_void_p]),
    # include/rt_hip_segment.h
    "rt_segments_occluded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_uint32, C.c_void_p]),
    "rt_segments_closest": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_uint32, C.c_void_p]),
    "rt_segments_occluded_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_uint32,
                                              C.c_void_p, C.c_void_p]),
    "rt_segments_closest_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_uint32,
                                             C.c_void_p, C.c_void_p]),
    "rt_visibility_masks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_uint32,
                                      C.c_void_p]),
    "rt_visibility_masks_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_float, C.c_float,
                                             C.c_uint32, C.c_void_p, C.c_void_p]),
    # include/rt_hip_instance_segments.h
    "rt_instances_segments_occluded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_uint32,
                                                 C.c_void_p]),
    "rt_instances_segments_closest": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_uint32,
                                                C.c_void_p]),
    "rt_instances_segments_occluded_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_uint32,
                                                        C.c_void_p, C.c_void_p]),
    "rt_instances_segments_closest_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_uint32,
                                                       C.c_void_p, C.c_void_p]),
    "rt_instances_visibility_masks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_float, C.c_float,
                                                C.c_uint32, C.c_void_p]),
    "rt_instances_visibility_masks_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_float, C.c_float,
                                                       C.c_uint32, C.c_void_p, C.c_void_p]),
    # include/rt_hip_instances.h
    "rt_set_instances": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "rt_instance_count": (C.c_uint32, [C.c_void_p]),
    "rt_instance_node_count": (C.c_uint32, [C.c_void_p]),
    "rt_instances_object_from_world": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rt_instance_nodes": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rt_trace_instances_closest": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.c_void_p]),
    "rt_trace_instances_occluded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.c_void_p]),
    "rt_trace_instances_closest_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.c_void_p,
                                                    C.c_void_p]),
    "rt_trace_instances_occluded_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.c_void_p,
                                                     C.c_void_p]),
    "rt_instance_plan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    # include/rt_hip_instance_build.h
    "rt_build_instances_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "rt_build_instances": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "rt_instances_world_from_object": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rt_instance_bounds": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rt_last_instance_build_ms": (C.c_float, [C.c_void_p]),
    "rt_instance_plan_lbvh": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    # include/rt_hip_nearest.h
    "rt_closest_points": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.c_void_p]),
    "rt_closest_points_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p]),
    "rt_signed_distance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.c_void_p]),
    "rt_signed_distance_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p]),
    "rt_signed_distance_grid": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    "rt_signed_distance_grid_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p,
                                                 C.c_void_p]),
    "rt_prepare_signed_distance": (C.c_int, [C.c_void_p]),
    "rt_last_sign_build_ms": (C.c_float, [C.c_void_p]),
    "rt_debug_sign_table": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rt_instances_closest_points": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.c_void_p]),
    "rt_instances_closest_points_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p]),
    "rt_debug_set_nearest_walk": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rt_debug_last_nearest_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    # include/rt_hip_multihit.h
    "rt_trace_multihit":(C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p]),
    "rt_trace_multihit_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.c_uint32,
                                           C.c_void_p, C.c_void_p]),
    # include/rt_hip_ao.h
    "rt_ao_rays_per_point": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "rt_trace_ao": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "rt_trace_ao_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    # include/rt_hip_instance_multihit.h
    "rt_trace_instances_multihit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.c_uint32,
                                              C.c_void_p]),
    "rt_trace_instances_multihit_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32, C.c_uint32,
                                                     C.c_void_p, C.c_void_p]),
    # include/rt_hip_instance_directional.h
    "rt_trace_instances_ao_directional": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "rt_trace_instances_ao_directional_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                                           C.c_void_p, C.c_void_p]),
    # include/rt_hip_directional.h
    "rt_ao_mask_words": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "rt_trace_ao_directional": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "rt_trace_ao_directional_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                                 C.c_void_p]),
    "rt_ao_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "rt_ao_rays_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    # include/rt_hip_layers.h
    "rt_render_layers": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rt_render_layers_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    # include/rt_hip_views.h
    "rt_render_views": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "rt_render_views_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    # include/rt_hip_instance_views.h
    "rt_trace_instances_ao": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "rt_trace_instances_ao_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                               C.c_void_p, C.c_void_p]),
    "rt_render_instance_views": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "rt_render_instance_views_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    # include/rt_hip_update.h
    "rt_update_vertices":(C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    "rt_update_vertices_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "rt_scene_refit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "rt_last_update_ms": (C.c_float, [C.c_void_p]),
    # include/rt_hip_build.h
    "rt_build_scene": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]),
    "rt_build_scene_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]),
    "rt_built_faces": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rt_scene_build_lbvh": (C.c_int, [C.c_void_p]),
    "rt_last_build_ms": (C.c_float, [C.c_void_p]),
    "rt_debug_last_build_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "rt_debug_set_refit_group": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rt_debug_refit_schedule": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "rt_debug_record_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "rt_debug_download_records": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # include/rt_hip_camera.h
    "rt_camera_default": (None, [C.POINTER(Camera)]),
    "rt_camera_look_at": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(Camera)]),
    "rt_set_camera": (C.c_int, [C.c_void_p, C.POINTER(Camera)]),
    "rt_get_camera": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(C.c_int)]),
    "rt_ring_set_camera": (C.c_int, [C.c_void_p, C.POINTER(Camera)]),
}


class _HitArrays(C.Structure):
    """rt_hit_arrays (include/rt_hip_query.h)."""
    _fields_ = [("hit", C.c_void_p), ("distance", C.c_void_p), ("leaf", C.c_void_p), ("barycentric", C.c_void_p),
                ("position", C.c_void_p), ("normal", C.c_void_p)]


class _MultiHitArrays(C.Structure):
    """rt_multihit_arrays (include/rt_hip_multihit.h)."""
    _fields_ = [("count", C.c_void_p), ("distance", C.c_void_p), ("leaf", C.c_void_p), ("barycentric", C.c_void_p),
                ("position", C.c_void_p), ("normal", C.c_void_p)]


class _DirectionalArrays(C.Structure):
    """rt_ao_directional_arrays (include/rt_hip_directional.h)."""
    _fields_ = [("ao", C.c_void_p), ("occluded", C.c_void_p), ("mask", C.c_void_p), ("bent", C.c_void_p)]


class _InstanceHitArrays(C.Structure):
    """rt_instance_hit_arrays (include/rt_hip_instances.h)."""
    _fields_ = [("record", _HitArrays), ("instance", C.c_void_p)]


class _SignedArrays(C.Structure):
    """rt_signed_arrays (include/rt_hip_signed.h)."""
    _fields_ = [("hit", _HitArrays), ("feature", C.c_void_p), ("pseudonormal4", C.c_void_p)]


class _InstanceMultiHitArrays(C.Structure):
    """rt_instance_multihit_arrays (include/rt_hip_instance_multihit.h)."""
    _fields_ = [("slots", _MultiHitArrays), ("instance", C.c_void_p)]


class _VisibilityArrays(C.Structure):
    """rt_visibility_arrays (include/rt_hip_segment.h)."""
    _fields_ = [("mask", C.c_void_p), ("count", C.c_void_p)]


class _LayerArrays(C.Structure):
    """rt_layer_arrays (include/rt_hip_layers.h)."""
    _fields_ = _HitArrays._fields_ + [("direction", C.c_void_p), ("shade", C.c_void_p), ("ao", C.c_void_p), ("value", C.c_void_p)]


class _ViewArrays(C.Structure):
    """rt_view_arrays (include/rt_hip_views.h)."""
    _fields_ = [("layers", _LayerArrays), ("image", C.c_void_p)]


class _InstanceViewArrays(C.Structure):
    """rt_instance_view_arrays (include/rt_hip_instance_views.h)."""
    _fields_ = [("views", _ViewArrays), ("instance", C.c_void_p)]


RT_QUERY_NO_SORT = 1
# the records of a scene on the device (csrc/device_types.h: NodeRec, TriRec, ShadeRec), as Host.records() returns them
NODE_RECORD = np.dtype([("lo", np.float32, 3), ("skip", np.uint32), ("hi", np.float32, 3), ("leaf", np.uint32)])
TRI_RECORD = np.dtype([("lo", np.float32, 3), ("pad0", np.float32), ("hi", np.float32, 3), ("inv_d", np.float32), ("ta", np.float32, 3),
                       ("u", np.float32, 3), ("v", np.float32, 3), ("n", np.float32, 3), ("uu", np.float32), ("uv", np.float32),
                       ("vv", np.float32), ("D", np.float32)])
SHADE_RECORD = np.dtype([("n0", np.float32, 4), ("n1", np.float32, 4), ("n2", np.float32, 4)])
assert (NODE_RECORD.itemsize, TRI_RECORD.itemsize, SHADE_RECORD.itemsize) == (32, 96, 48)
RT_MULTIHIT_MAX_K = 16
MULTIHIT_OUTPUTS = ("count", "distance", "leaf", "barycentric", "position", "normal")
QUERY_OUTPUTS = ("hit", "distance", "leaf", "barycentric", "position", "normal")
NEAREST_OUTPUTS = QUERY_OUTPUTS  # closest-point queries: "hit" is `found`
# signed distance queries: the record with `distance` signed, the feature code (FEATURES) and the pseudonormal with g behind it
SIGNED_OUTPUTS = QUERY_OUTPUTS + ("feature", "pseudonormal")
FEATURES = ("face", "vertex A", "vertex B", "vertex C", "edge AB", "edge AC", "edge BC")
SIGN_RECORD = np.dtype([("edge", np.float32, (3, 4)), ("vertex", np.float32, (3, 4))])  # a leaf of Host.sign_table()
INSTANCE_MULTIHIT_OUTPUTS = MULTIHIT_OUTPUTS + ("instance",)  # instanced multi-hit queries: the copy of every slot beside it
INSTANCE_OUTPUTS = QUERY_OUTPUTS + ("instance",)  # instanced ray queries: the record and the instance it lies in
RT_INSTANCES_MAX = 1 << 20
# the record of a top-level tree (include/rt_hip_instances.h): the node record the exact walk reads
INSTANCE_NODE = np.dtype([("lo", np.float32, 3), ("skip", np.uint32), ("hi", np.float32, 3), ("leaf", np.uint32)])
SEGMENT_OUTPUTS = QUERY_OUTPUTS  # segment queries, the closest form: "hit" is "the segment has a blocker"
VISIBILITY_OUTPUTS = ("mask", "count")
SEGMENT_INTERVAL = (1e-4, 1 - 1e-4)  # the default (t_lo, t_hi) of the segment queries, fractions of the segment
AO_OUTPUTS = ("ao", "occluded")
DIRECTIONAL_OUTPUTS = ("ao", "occluded", "mask", "bent")
LAYER_OUTPUTS = QUERY_OUTPUTS + ("direction", "shade", "ao", "value")
VIEW_OUTPUTS = LAYER_OUTPUTS + ("image",)
INSTANCE_VIEW_OUTPUTS = VIEW_OUTPUTS + ("instance",)  # instanced views: the copy a sub-pixel's record lies in
# per output of any query: numpy dtype, values per record.  The first four are one value per ray or point; the others are
# the fields of a hit record: one record per ray (closest hit) or k of them (multi-hit).
_OUTPUT_LAYOUT = {"hit": (np.uint8, 1), "count": (np.uint32, 1), "ao": (np.float32, 1), "occluded": (np.uint32, 1),
                  "distance": (np.float32, 1), "leaf": (np.uint32, 1), "barycentric": (np.float32, 3), "position": (np.float32, 3),
                  "normal": (np.float32, 3), "direction": (np.float32, 3), "shade": (np.float32, 1), "value": (np.float32, 1),
                  "bent": (np.float32, 3), "instance": (np.uint32, 1), "feature": (np.uint8, 1), "pseudonormal": (np.float32, 4)}
_RECORD_FIELDS = ("distance", "leaf", "barycentric", "position", "normal")


def _known(outputs, legal: tuple) -> tuple:
    """`outputs` as a tuple, every name of it one of `legal`."""
    outputs = tuple(outputs)
    unknown = [o for o in outputs if o not in legal]
    if unknown:
        raise ValueError(f"unknown outputs {unknown}; choose from {legal}")
    return outputs


# How an instanced family's output structure is made of its pointers: the plain family's, and "instance" behind them.
def _instance_hits(*at):
    return _InstanceHitArrays(_HitArrays(*at[:-1]), at[-1])


def _instance_multihits(*at):
    return _InstanceMultiHitArrays(_MultiHitArrays(*at[:-1]), at[-1])


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _rays4_numpy(a, what: str) -> np.ndarray:
    if not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.ndim != 2 or a.shape[1] not in (3, 4):
        raise ValueError(f"{what}: expected a float32 array of shape (N, 3) or (N, 4)")
    if a.shape[1] == 4:
        return np.ascontiguousarray(a)
    out = np.zeros((a.shape[0], 4), dtype=np.float32)
    out[:, :3] = a
    return out


def _rays4_torch(t, what: str):
    import torch

    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] not in (3, 4):
        raise ValueError(f"{what}: expected a float32 tensor of shape (N, 3) or (N, 4)")
    if not t.is_contiguous():
        raise ValueError(f"{what}: the tensor must be contiguous")
    if t.device.type != "cuda":
        raise ValueError(f"{what}: the tensor must be on the host's GPU")
    if t.shape[1] == 4:
        return t
    return torch.nn.functional.pad(t, (0, 1))  # (N, 4), on the device, stream-ordered


class _QueryArrays:
    """The arrays of one query call: the two (N, 3) / (N, 4) inputs padded to (N, 4), the outputs made from
    _OUTPUT_LAYOUT, their addresses, and the call itself.  numpy arrays in host memory go to the library's blocking entry
    points; torch tensors on the host's GPU go to its *_device entry points, enqueued on torch.cuda.current_stream()
    without waiting.  The inputs a, b (and `also`, if given) must be of one kind."""

    def __init__(self, a, b, names, items: str, also=None):
        given = [a] + ([] if b is None else [b]) + ([] if also is None else [also])
        self.torch = any(_is_torch(x) for x in given)
        if self.torch and not all(_is_torch(x) for x in given):
            both = "all" if len(names) > 2 else "both"
            raise ValueError(f"{', '.join(names[:-1])} and {names[-1]} must {both} be torch tensors or {both} numpy arrays")
        pad = _rays4_torch if self.torch else _rays4_numpy
        self.a = pad(a, names[0])
        self.b = self.a if b is None else pad(b, names[1])  # (b None: a query of points alone, closest_points)
        self.inputs = (self.a,) if b is None else (self.a, self.b)
        if self.a.shape[0] != self.b.shape[0] or (self.torch and self.a.device != self.b.device):
            raise ValueError(f"{names[0]} and {names[1]} must hold the same number of {items}"
                             + (" on the same device" if self.torch else ""))
        self.n = int(self.a.shape[0])
        self.suffix, self.stream, self.padded = "", (), []
        if self.torch:
            import torch

            self.current = torch.cuda.current_stream(self.a.device)
            self.suffix, self.stream = "_device", (self.current.cuda_stream,)
            self.padded = [t for t, was in ((self.a, a), (self.b, b)) if was is not None and t is not was]

    def ptr(self, x) -> int:
        return x.data_ptr() if self.torch else x.ctypes.data

    def seeds(self, seeds):
        """The uint32 (N,) seeds of an ambient-occlusion call, checked."""
        if self.torch:
            import torch

            if seeds.dtype not in (torch.uint32, torch.int32) or seeds.dim() != 1 or seeds.shape[0] != self.n:
                raise ValueError("seeds: expected a uint32 tensor of shape (N,)")
            if not seeds.is_contiguous() or seeds.device != self.a.device:
                raise ValueError("seeds: the tensor must be contiguous and on the points' device")
            return seeds
        if not isinstance(seeds, np.ndarray) or seeds.dtype != np.uint32 or seeds.shape != (self.n,):
            raise ValueError("seeds: expected a uint32 array of shape (N,)")
        return np.ascontiguousarray(seeds)

    def outputs(self, names, k=None, shapes=None) -> dict:
        """{name: (N,) or (N, 3)}; with k the fields of a hit record are (N, k) or (N, k, 3).  `shapes`: {name: (dtype, what
        follows N in the shape)} for outputs whose layout depends on the host's options."""
        out = {}
        for name in names:
            if shapes and name in shapes:
                dtype, shape = shapes[name][0], (self.n,) + tuple(shapes[name][1])
            else:
                dtype, per = _OUTPUT_LAYOUT[name]
                slots = (k,) if k is not None and name in _RECORD_FIELDS else ()
                shape = (self.n,) + slots + ((per,) if per > 1 else ())
            if self.torch:
                import torch

                out[name] = torch.empty(shape, dtype=getattr(torch, np.dtype(dtype).name), device=self.a.device)
            else:
                out[name] = np.empty(shape, dtype=dtype)
        return out

    def pointers(self, out: dict, names, name_empty: bool = False) -> list:
        """The addresses of the outputs in the order of `names`; None: not asked for, or the call has nothing to work on
        (N = 0).  name_empty: an array is named even where it holds nothing -- N = 0, or a slot array with k = 0 --, so
        that the library says what is wrong with the call, as it would for a caller in C."""
        if name_empty:
            return [self.ptr(out[name]) or 4 if name in out else None for name in names]
        return [self.ptr(out[name]) if name in out and self.n else None for name in names]

    def call(self, h, function: str, *args) -> None:
        """function(h, the two inputs -- or the one --, *args) -- or function_device(..., the current stream)."""
        _check(getattr(load_library(), function + self.suffix)(h, *(self.ptr(x) for x in self.inputs), *args, *self.stream))
        for t in self.padded:  # (the padded copies must live until the kernels have read them)
            t.record_stream(self.current)


def unpack_ao_mask(mask, rays: int):
    """The (N, W) uint32 mask rows of directional_occlusion as booleans: (N, rays), [i, k] True iff ray k of point i was
    blocked.  numpy in, numpy out; torch in, torch out on the same device."""
    rays = int(rays)
    if mask.ndim != 2 or rays < 0 or rays > 32 * int(mask.shape[1]):
        raise ValueError("mask: expected (N, W) rows with W >= ceil(rays / 32)")
    k = np.arange(rays)
    if _is_torch(mask):
        import torch

        if mask.dtype not in (torch.uint32, torch.int32):
            raise ValueError("mask: expected uint32 words")
        words = mask.view(torch.int32)[:, torch.from_numpy(k >> 5).to(mask.device)]
        return ((words >> torch.from_numpy((k & 31).astype(np.int32)).to(mask.device)) & 1).to(torch.bool)
    if not isinstance(mask, np.ndarray) or mask.dtype != np.uint32:
        raise ValueError("mask: expected uint32 words")
    return ((mask[:, k >> 5] >> (k & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)


def unpack_visibility_mask(mask, targets: int):
    """The (P, W) uint32 mask rows of Host.visibility as booleans: (P, targets), [i, j] True iff the segment from point i to
    target j is OCCLUDED.  numpy in, numpy out; torch in, torch out on the same device."""
    return unpack_ao_mask(mask, targets)  # (the same layout: bit j & 31 of word j >> 5)


def _transforms12(transforms) -> np.ndarray:
    t = np.asarray(transforms)
    if t.dtype != np.float32 or t.ndim != 3 or t.shape[1:] != (3, 4):
        raise ValueError("transforms: expected a float32 array of shape (n, 3, 4), the rows of [A | t]")
    return np.ascontiguousarray(t)


def instance_plan(root_lo, root_hi, transforms) -> dict:
    """The planner of an instance set alone (rt_instance_plan, include/rt_hip_instances.h; host only, no device):
    {"object_from_world": float32 (n, 3, 4), "nodes": INSTANCE_NODE (2n - 1,)} for a scene whose root box is
    (root_lo, root_hi).  RtError -1 for a refused transform."""
    w = _transforms12(transforms)
    lo, hi = np.ascontiguousarray(root_lo, np.float32).reshape(3), np.ascontiguousarray(root_hi, np.float32).reshape(3)
    n = int(w.shape[0])
    inverse, nodes = np.zeros((n, 3, 4), np.float32), np.zeros(max(2 * n - 1, 0), INSTANCE_NODE)
    rc = load_library().rt_instance_plan(lo.ctypes.data, hi.ctypes.data, w.ctypes.data, n, inverse.ctypes.data, nodes.ctypes.data)
    if rc != 0:
        raise RtError(rc, "rt_instance_plan: no transforms, too many, or a refused transform")
    return {"object_from_world": inverse, "nodes": nodes}


def instance_plan_lbvh(root_lo, root_hi, transforms) -> dict:
    """What a device-side instance build makes, restated on the host (rt_instance_plan_lbvh,
    include/rt_hip_instance_build.h; no device): {"object_from_world": float32 (n, 3, 4), "nodes": INSTANCE_NODE (2n - 1,),
    the radix tree over the leaf boxes' Morton keys, "bounds": float32 (n, 4), the closest-point walk's} for a scene whose
    root box is (root_lo, root_hi).  RtError -1 for a refused transform."""
    w = _transforms12(transforms)
    lo, hi = np.ascontiguousarray(root_lo, np.float32).reshape(3), np.ascontiguousarray(root_hi, np.float32).reshape(3)
    n = int(w.shape[0])
    inverse, nodes, bounds = np.zeros((n, 3, 4), np.float32), np.zeros(max(2 * n - 1, 0), INSTANCE_NODE), np.zeros((n, 4), np.float32)
    rc = load_library().rt_instance_plan_lbvh(lo.ctypes.data, hi.ctypes.data, w.ctypes.data, n, inverse.ctypes.data, nodes.ctypes.data,
                                              bounds.ctypes.data)
    if rc != 0:
        raise RtError(rc, "rt_instance_plan_lbvh: no transforms, too many, or a refused transform")
    return {"object_from_world": inverse, "nodes": nodes, "bounds": bounds}


def load_library() -> C.CDLL:
    """Loads lib/libocrt_hip.so; raises if it has not been built (no fallback)."""
    global _LIB
    if _LIB is None:
        path = lib_path()
        if not os.path.exists(path):
            raise ImportError(
                f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C opencl_raytracer_amd/csrc`). There is no CPU fallback."
            )
        lib = C.CDLL(path)
        for name, (restype, argtypes) in _SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:
                # an OLDER build of the library loaded on purpose for an A/B run (OCRT_LIB_DIR + OCRT_ALLOW_OLD_LIB=1, set by
                # the A/B tools): it may lack the newest entry points, which such a run does not call.  Every other library
                # -- the product one, and one that OCRT_LIB_DIR merely locates -- must export every one of them.
                if os.environ.get("OCRT_LIB_DIR") and os.environ.get("OCRT_ALLOW_OLD_LIB") == "1":
                    print(f"opencl_raytracer_amd: {path} lacks {name} (OCRT_ALLOW_OLD_LIB=1: skipped)", file=sys.stderr)
                    continue
                raise
            fn.restype = restype
            fn.argtypes = argtypes
        _LIB = lib
    return _LIB


def _check(rc: int) -> None:
    if rc != 0:
        lib = load_library()
        raise RtError(rc, lib.rt_last_error().decode("utf-8", "replace"))


def _raise_last() -> None:
    lib = load_library()
    raise RtError(lib.rt_last_error_code(), lib.rt_last_error().decode("utf-8", "replace"))


def device_count() -> int:
    return load_library().rt_device_count()


def node_test_forms(records: np.ndarray, rays: np.ndarray, device: int = 0) -> np.ndarray:
    """The any-hit walk's node test in its two forms on the device (include/rt_hip_debug.h, rt_debug_node_test_forms):
    `records` (B, 8) float32 centre / half-extent records, `rays` (R, 6) float32 walk rays, R a multiple of 64.  Returns
    (R, B, 9) uint32: near, far (bit patterns) and the decision of the old form, of the new form on node a's registers, of
    the new form on node b's."""
    records = np.ascontiguousarray(records, dtype=np.float32)
    rays = np.ascontiguousarray(rays, dtype=np.float32)
    if records.ndim != 2 or records.shape[1] != 8 or rays.ndim != 2 or rays.shape[1] != 6:
        raise ValueError("node_test_forms: expected (B, 8) records and (R, 6) rays")
    out = np.empty((rays.shape[0], records.shape[0], 9), dtype=np.uint32)
    _check(load_library().rt_debug_node_test_forms(int(device), records.ctypes.data, records.shape[0], rays.ctypes.data,
                                                   rays.shape[0], out.ctypes.data))
    return out


def _view(ptr: int, count: int, dtype) -> np.ndarray:
    if count == 0:
        return np.zeros(0, dtype=dtype)
    ctype = {np.uint32: C.c_uint32, np.float32: C.c_float}[dtype]
    arr = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(count,))
    return arr.copy()


class Scene:
    """CPU-side mesh + BVH: load_off_mesh / compute_vertex_normals / BVH::buildBVH."""

    def __init__(self, handle: int):
        self._h = handle

    @classmethod
    def load_off(cls, path: str) -> "Scene":
        h = load_library().rt_scene_load_off(os.fsencode(path))
        if not h:
            _raise_last()
        return cls(h)

    @classmethod
    def from_arrays(cls, vertices: np.ndarray, faces: np.ndarray) -> "Scene":
        v = np.ascontiguousarray(vertices, dtype=np.float32)
        if v.ndim != 2 or v.shape[1] not in (3, 4):
            raise ValueError("vertices must be (V,3) or (V,4)")
        if v.shape[1] == 3:
            v = np.concatenate([v, np.zeros((v.shape[0], 1), np.float32)], axis=1)
        v = np.ascontiguousarray(v)
        f = np.ascontiguousarray(faces, dtype=np.uint32).reshape(-1)
        h = load_library().rt_scene_from_arrays(v.ctypes.data, v.shape[0], f.ctypes.data, f.size // 3)
        if not h:
            _raise_last()
        return cls(h)

    def close(self) -> None:
        if self._h:
            load_library().rt_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def build_bvh(self, method: int = 0) -> "Scene":
        _check(load_library().rt_scene_build_bvh(self._h, int(method)))
        return self

    def build_lbvh(self) -> "Scene":
        """The tree a device-side build makes (include/rt_hip_build.h, rt_scene_build_lbvh), on the CPU: Morton keys of the
        leaf boxes' centres, the stable order by key, the binary radix tree over them in pre-order, boxes by the refit rule.
        nodes, aabbs, triangles and sorted_faces as build_bvh leaves them; upload_scene takes the scene like any other."""
        _check(load_library().rt_scene_build_lbvh(self._h))
        return self

    @property
    def num_vertices(self) -> int:
        return load_library().rt_scene_num_vertices(self._h)

    @property
    def num_faces(self) -> int:
        return load_library().rt_scene_num_faces(self._h)

    @property
    def num_nodes(self) -> int:
        return load_library().rt_scene_num_nodes(self._h)

    def _arr(self, getter: str, count: int, dtype):
        return _view(getattr(load_library(), getter)(self._h), count, dtype)

    @property
    def vertices(self) -> np.ndarray:
        return self._arr("rt_scene_vertices", 4 * self.num_vertices, np.float32).reshape(-1, 4)

    @property
    def vnormals(self) -> np.ndarray:
        return self._arr("rt_scene_vnormals", 4 * self.num_vertices, np.float32).reshape(-1, 4)

    @property
    def faces(self) -> np.ndarray:
        return self._arr("rt_scene_faces", 3 * self.num_faces, np.uint32)

    @property
    def nodes(self) -> np.ndarray:
        return self._arr("rt_scene_nodes", self.num_nodes, np.uint32)

    @property
    def aabbs(self) -> np.ndarray:
        return self._arr("rt_scene_aabbs", 8 * self.num_nodes, np.float32).reshape(-1, 4)

    @property
    def triangles(self) -> np.ndarray:
        return self._arr("rt_scene_triangles", self.num_faces if self.num_nodes else 0, np.uint32)

    @property
    def sorted_faces(self) -> np.ndarray:
        return self._arr("rt_scene_sorted_faces", 3 * self.num_faces if self.num_nodes else 0, np.uint32)

    def refit(self, vertices) -> "Scene":
        """New vertex positions for the same faces (include/rt_hip_update.h, rt_scene_refit): `vertices` (V, 3) or (V, 4)
        float32 replaces every position, `vnormals` is recomputed, `aabbs` is refitted by the refit rule; nodes, triangles,
        faces and sorted_faces stay.  RtError -1 for another vertex count and for coordinates that are not finite or
        exceed 1e37.  What Host.update_vertices does to the scene on the device, on the CPU arrays."""
        v = _rays4_numpy(np.asarray(vertices), "vertices")
        _check(load_library().rt_scene_refit(self._h, v.ctypes.data, v.shape[0]))
        return self

    def refit_schedule(self, group_nodes: int = 0, packed_tree: bool = False) -> dict:
        """The schedule by which an update refits the inner boxes (include/rt_hip_debug.h, rt_debug_refit_schedule):
        {"skips": (N,), "entries": (E, 4) node / first child reference / children / round, "children": (C,), "groups":
        (G, 4) first entry / entries / rounds / pass, "passes", "group_nodes": S as used}, all uint32."""
        lib, counts = load_library(), (C.c_uint32 * 6)()
        _check(lib.rt_debug_refit_schedule(self._h, int(group_nodes), int(packed_tree), counts, None, None, None, None))
        skips, entries = np.zeros(counts[0], np.uint32), np.zeros((counts[1], 4), np.uint32)
        children, groups = np.zeros(counts[2], np.uint32), np.zeros((counts[3], 4), np.uint32)
        _check(lib.rt_debug_refit_schedule(self._h, int(group_nodes), int(packed_tree), counts, skips.ctypes.data, entries.ctypes.data,
                                           children.ctypes.data, groups.ctypes.data))
        return {"skips": skips, "entries": entries, "children": children, "groups": groups, "passes": int(counts[4]),
                "group_nodes": int(counts[5])}

    def face_of_leaf(self, leaf=None) -> np.ndarray:
        """The file-order face a query's `leaf` index stands for (rt_scene_triangles, include/rt_hip_query.h); without an
        argument the whole map.  Leaves of 0xFFFFFFFF (no hit) map to 0xFFFFFFFF."""
        faces = self.triangles
        if leaf is None:
            return faces
        leaf = np.asarray(leaf, dtype=np.uint32)
        miss = leaf == 0xFFFFFFFF
        return np.where(miss, np.uint32(0xFFFFFFFF), faces[np.where(miss, 0, leaf)]).astype(np.uint32)


class Host:
    """One render host == one OpenCLHost of the reference (ctor/upload/()/download)."""

    def __init__(self, options: Options, device: int = -1, rank: int = 0, nranks: int = 1):
        self.options, self._device = options, int(device)
        self._h = load_library().rt_create_on(C.byref(options), device, rank, nranks)
        if not self._h:
            _raise_last()

    @classmethod
    def _borrowed(cls, options: Options, handle: int, owner=None) -> "Host":
        """A view of a host that `owner` (a FrameRing) owns: it keeps the owner alive, and the owner's close() takes the
        handle away (`_h = None`: every later call then fails with RtError / returns 0 instead of touching freed memory)."""
        h = cls.__new__(cls)
        h.options, h._h, h._owned, h._owner = options, handle, False, owner
        return h

    def close(self) -> None:
        if getattr(self, "_h", None):
            if getattr(self, "_owned", True):
                load_library().rt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, faces, nodes, aabbs, vertices, vnormals) -> None:
        f = np.ascontiguousarray(faces, dtype=np.uint32).reshape(-1)
        n = np.ascontiguousarray(nodes, dtype=np.uint32).reshape(-1)
        a = np.ascontiguousarray(aabbs, dtype=np.float32).reshape(-1, 4)
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 4)
        vn = np.ascontiguousarray(vnormals, dtype=np.float32).reshape(-1, 4)
        if a.shape[0] != 2 * n.size:
            raise RtError(RT_E_INVALID, "aabbs must hold a (min,max) pair per node")
        if vn.shape[0] != v.shape[0]:
            raise RtError(RT_E_INVALID, "one normal per vertex expected")
        _check(load_library().rt_upload(self._h, f.ctypes.data, f.size // 3, n.ctypes.data, n.size, a.ctypes.data,
                                        v.ctypes.data, v.shape[0], vn.ctypes.data))

    def upload_scene(self, scene: Scene) -> None:
        _check(load_library().rt_upload_scene(self._h, scene._h))

    def set_camera(self, camera: Camera) -> None:
        """Gives the host its pose (include/rt_hip_camera.h, rt_set_camera): before the upload only, RtError -4 afterwards
        and on the hosts of a frame ring."""
        _check(load_library().rt_set_camera(self._h, C.byref(camera)))

    def camera(self) -> Camera:
        """The host's pose -- the reference's camera if none was set (`camera_is_set`)."""
        c = Camera()
        _check(load_library().rt_get_camera(self._h, C.byref(c), None))
        return c

    @property
    def camera_is_set(self) -> bool:
        c, flag = Camera(), C.c_int()
        _check(load_library().rt_get_camera(self._h, C.byref(c), C.byref(flag)))
        return bool(flag.value)

    def render(self) -> None:
        _check(load_library().rt_render(self._h))

    __call__ = render

    def render_async(self) -> None:
        _check(load_library().rt_render_async(self._h))

    def sync(self) -> None:
        _check(load_library().rt_sync(self._h))

    def download(self) -> np.ndarray:
        img = np.empty((self.options.total_height, self.options.total_width), dtype=np.float32)
        _check(load_library().rt_download(self._h, img.ctypes.data))
        return img

    def download_u8(self) -> np.ndarray:
        img = np.empty((self.options.height, self.options.width), dtype=np.uint8)
        _check(load_library().rt_download_u8(self._h, img.ctypes.data))
        return img

    @property
    def local_rows(self) -> int:
        return load_library().rt_local_rows(self._h)

    def local_to_global_rows(self) -> np.ndarray:
        lib = load_library()
        return np.array([lib.rt_local_to_global_row(self._h, j) for j in range(self.local_rows)], dtype=np.int64)

    def download_u8_local(self) -> np.ndarray:
        rows = np.empty((self.local_rows, self.options.width), dtype=np.uint8)
        _check(load_library().rt_download_u8_local(self._h, rows.ctypes.data))
        return rows

    def resize_into_device(self, device_ptr: int) -> None:
        _check(load_library().rt_resize_into_device(self._h, device_ptr))

    def set_stream(self, hip_stream: int) -> None:
        _check(load_library().rt_set_stream(self._h, hip_stream))

    def use_private_stream(self) -> None:
        _check(load_library().rt_use_private_stream(self._h))

    def set_device_share(self, hosts: int) -> None:
        """`hosts` of them (this one included) take frames in turn on this GPU."""
        _check(load_library().rt_set_device_share(self._h, int(hosts)))

    @property
    def stream_handle(self) -> int:
        """The hipStream_t (as an integer) this host enqueues on."""
        p = C.c_void_p()
        _check(load_library().rt_get_stream(self._h, C.byref(p)))
        return int(p.value or 0)

    def set_ao_prefetch(self, on: bool) -> None:
        """Which form of the AO pass's node loop this host launches (include/rt_hip_debug.h, rt_set_ao_prefetch); same results."""
        _check(load_library().rt_set_ao_prefetch(self._h, int(on)))

    def poison_hit_list(self) -> None:
        """Test aid (include/rt_hip_debug.h): overwrites the hit list and the occlusion counts with 0xFF between frames."""
        _check(load_library().rt_debug_poison_hit_list(self._h))

    def expect_frames(self, frames: int) -> None:
        """Announces a stream of frames (include/rt_hip.h, rt_expect_frames): uploads then prepare the walk intervals."""
        _check(load_library().rt_expect_frames(self._h, int(frames)))

    def measure_tile_costs(self, frames: int = 2, reorder: bool = True) -> None:
        """Measures what the tiles' AO packets cost (include/rt_hip_debug.h) and, with `reorder`, claims them by that."""
        _check(load_library().rt_debug_measure_tile_costs(self._h, int(frames), int(reorder)))

    def set_primary_split(self, above: int) -> None:
        """Primary pass: tiles of cost class `above` or more are cast in quarters (DeviceRenderer::setPrimarySplit; 0: none)."""
        _check(load_library().rt_debug_set_primary_split(self._h, int(above)))

    def set_order_policy(self, heavy: float, runway: float, split_above: float = -1.0) -> None:
        """How orders are made from measured costs (DeviceRenderer::orderByMeasuredCost); re-orders if costs have been measured."""
        _check(load_library().rt_debug_set_order_policy(self._h, float(heavy), float(runway), float(split_above)))

    def tile_order(self) -> dict:
        """The AO pass's claim order: list (eight segments), 8 x 3 constants, tile words, measured costs per tile."""
        lib = load_library()
        slots, tiles = lib.rt_debug_tile_order_slots(self._h), lib.rt_debug_tiles(self._h)
        order, constants = np.zeros(slots, np.uint32), np.zeros(24, np.uint32)
        words, costs = np.zeros(tiles, np.uint32), np.zeros(tiles, np.float32)
        _check(lib.rt_debug_tile_order(self._h, order.ctypes.data, constants.ctypes.data, words.ctypes.data, costs.ctypes.data))
        return {"order": order, "constants": constants.reshape(8, 3), "words": words, "costs": costs}

    def set_tile_order(self, order, constants) -> None:
        order = np.ascontiguousarray(order, np.uint32)
        constants = np.ascontiguousarray(constants, np.uint32).reshape(24)
        _check(load_library().rt_debug_set_tile_order(self._h, order.ctypes.data, len(order), constants.ctypes.data))

    def split_tiles(self) -> np.ndarray:
        """Per XCD group, the tiles at the head of its list that the AO pass claims half a tile at a time
        (include/rt_hip_debug.h, rt_debug_split_tiles)."""
        out = np.zeros(8, np.uint32)
        _check(load_library().rt_debug_split_tiles(self._h, out.ctypes.data))
        return out

    def set_cheap_claims(self, cheap_below: float) -> None:
        """The boundary of the lists' cheap suffix in reference costs (include/rt_hip_debug.h, rt_debug_set_cheap_claims):
        0 turns the region off, a huge value puts every unsplit tile in it; re-orders if costs have been measured."""
        _check(load_library().rt_debug_set_cheap_claims(self._h, float(cheap_below)))

    def cheap_tiles(self) -> np.ndarray:
        """Per XCD group, the tiles at the end of its list that the AO pass claims whole, one per wave
        (include/rt_hip_debug.h, rt_debug_cheap_tiles)."""
        out = np.zeros(8, np.uint32)
        _check(load_library().rt_debug_cheap_tiles(self._h, out.ctypes.data))
        return out

    def prune_facts(self) -> dict:
        """What the closest-hit walk's pruning rests on in the uploaded scene (include/rt_hip_debug.h, rt_debug_prune_facts):
        `prune_margin` is finite on a host that prunes (a stream host) and +inf on one that does not (a one-shot host)."""
        margin, unpruned, primary = C.c_float(), C.c_uint32(), C.c_uint32()
        _check(load_library().rt_debug_prune_facts(self._h, C.byref(margin), C.byref(unpruned), C.byref(primary)))
        return {"prune_margin": float(margin.value), "unpruned_bytes": unpruned.value, "primary_bytes": primary.value}

    def walk_entries(self) -> dict:
        """The intervals of the node array the tiles' any-hit packets walk (include/rt_hip_debug.h, rt_walk_entries)."""
        hit, narrowed, share, packet_share = C.c_uint32(), C.c_uint32(), C.c_double(), C.c_double()
        _check(load_library().rt_walk_entries(self._h, C.byref(hit), C.byref(narrowed), C.byref(share), C.byref(packet_share)))
        return {"tiles_hit": hit.value, "tiles_narrowed": narrowed.value, "mean_share": share.value,
                "mean_packet_share": packet_share.value}

    def walk_interval_ends(self) -> dict:
        """Where the intervals the any-hit packets use end, by kind (include/rt_hip_debug.h, rt_debug_walk_interval_ends)."""
        out = np.zeros(6, np.uint32)
        _check(load_library().rt_debug_walk_interval_ends(self._h, out.ctypes.data))
        keys = ("intervals", "whole_array", "after_leaf", "after_inner", "last_is_leaf", "last_is_inner")
        return {k: int(v) for k, v in zip(keys, out)}

    def stats(self) -> dict:
        s = _Stats()
        _check(load_library().rt_get_stats(self._h, C.byref(s)))
        return {k: int(getattr(s, k)) for k, _ in _Stats._fields_}

    @property
    def last_kernel_ms(self) -> float:
        return float(load_library().rt_last_kernel_ms(self._h))

    @property
    def total_kernel_ms(self) -> float:
        return float(load_library().rt_total_kernel_ms(self._h))

    @property
    def last_ao_ms(self) -> float:
        return float(load_library().rt_last_ao_ms(self._h))

    @property
    def total_ao_ms(self) -> float:
        return float(load_library().rt_total_ao_ms(self._h))

    @property
    def kernel_launches(self) -> int:
        return int(load_library().rt_kernel_launches(self._h))

    def reset_timers(self) -> None:
        load_library().rt_reset_timers(self._h)

    # ---- ray queries (include/rt_hip_query.h) ----
    def trace_closest(self, origins, directions, max_distance: float = 100000.0, outputs=QUERY_OUTPUTS, sort: bool = True) -> dict:
        """Closest hit of every ray: {output name: array}.  numpy (N, 3) / (N, 4) float32 in, numpy out (blocking); torch
        tensors on the host's GPU in, torch tensors out, enqueued on torch.cuda.current_stream() without waiting."""
        return Host._trace(self, "rt_trace", QUERY_OUTPUTS, _HitArrays, True, origins, directions, max_distance, outputs, sort)

    def trace_occluded(self, origins, directions, max_distance: float = 100000.0, sort: bool = True):
        """Occlusion of every ray (the `hit` of trace_closest for the same rays and max_distance): uint8 (N,)."""
        return Host._trace(self, "rt_trace", QUERY_OUTPUTS, _HitArrays, False, origins, directions, max_distance, ("hit",), sort)["hit"]

    def _trace(self, family: str, legal: tuple, wrap, closest: bool, origins, directions, max_distance: float, outputs, sort: bool) -> dict:
        """The ray queries, plain and instanced: <family>_closest with wrap(the pointers of `legal`), or <family>_occluded.
        (The public methods reach these shared bodies through the class: nothing is looked up on `self` before the inputs
        have been checked.)"""
        outputs = _known(outputs, legal)
        io = _QueryArrays(origins, directions, ("origins", "directions"), "rays")
        out = io.outputs(outputs)
        args = (io.n, float(max_distance), 0 if sort else RT_QUERY_NO_SORT)
        if closest:
            io.call(self._h, family + "_closest", *args, C.byref(wrap(*io.pointers(out, legal))))
        else:
            io.call(self._h, family + "_occluded", *args, *io.pointers(out, ("hit",)))
        return out

    # ---- instanced ray queries (include/rt_hip_instances.h) ----
    def set_instances(self, transforms) -> None:
        """Poses n copies of the host's scene: float32 (n, 3, 4), the rows of world_from_object = [A | t]; n = 0 clears the
        set.  The set outlives update_vertices, build_scene and uploads.  RtError -1 for a transform with an entry that is not
        finite, a zero determinant or an inverse that is not finite: the host's set stays what it was."""
        w = _transforms12(transforms)
        _check(load_library().rt_set_instances(self._h, w.ctypes.data if len(w) else None, len(w)))
        self._instance_transforms = w.copy()  # (what instances() hands back: the library keeps its own copy)
        self._instances_built = False

    def build_instances(self, transforms) -> None:
        """set_instances with the set made ON the device (rt_build_instances, include/rt_hip_instance_build.h): inverses,
        bounds and the top-level tree -- a radix tree over Morton keys, instance_plan_lbvh restates it -- come from kernels;
        every instanced query runs on the set as on set_instances's.  `transforms`: a float32 numpy array (n, 3, 4) (one
        upload), or a contiguous float32 torch tensor (n, 3, 4) on the host's GPU, whose pointer is handed over with no host
        copy, enqueued on torch.cuda.current_stream(); the tensor may be reused on return.  The call waits once, for 36
        bytes.  n = 0 clears the set; the set replaces set_instances's and is replaced by it.  RtError -1 for a refused
        transform, found on the device: the host's set stays what it was."""
        lib = load_library()
        if _is_torch(transforms):
            import torch

            t = transforms
            if t.dtype != torch.float32 or t.dim() != 3 or tuple(t.shape[1:]) != (3, 4):
                raise ValueError("transforms: expected a float32 tensor of shape (n, 3, 4), the rows of [A | t]")
            if t.device.type != "cuda" or (t.device.index is not None and t.device.index != self._device):
                raise ValueError("transforms: the tensor must be on the host's GPU")
            if not t.is_contiguous():
                raise ValueError("transforms: the tensor must be contiguous")
            n = int(t.shape[0])
            if n and t.data_ptr() % 16:
                raise ValueError("transforms: the tensor's memory must be 16-byte aligned")
            _check(lib.rt_build_instances_device(self._h, t.data_ptr() if n else None, n, torch.cuda.current_stream(t.device).cuda_stream))
        else:
            if not isinstance(transforms, np.ndarray):
                raise ValueError("transforms: expected a float32 numpy array or torch tensor of shape (n, 3, 4)")
            w = _transforms12(transforms)
            _check(lib.rt_build_instances(self._h, w.ctypes.data if len(w) else None, len(w)))
        self._instance_transforms = np.zeros((0, 3, 4), np.float32)
        self._instances_built = True

    def instance_bounds(self) -> np.ndarray:
        """float32 (n, 4): what the instanced closest-point walk holds a copy's boxes against (rt_instance_bounds), for a
        set of either kind, as it is on the device (made again first if the scene changed)."""
        lib = load_library()
        out = np.zeros((int(lib.rt_instance_count(self._h)), 4), np.float32)
        _check(lib.rt_instance_bounds(self._h, out.ctypes.data))
        return out

    def last_instance_build_ms(self) -> float:
        """HIP-event time of the planning launches of the last device-side plan of the set, a build or a refresh (0: none)."""
        return float(load_library().rt_last_instance_build_ms(self._h))

    def instances(self) -> dict:
        """{"world_from_object": float32 (n, 3, 4) as given, "object_from_world": float32 (n, 3, 4) as the kernel uses it,
        "nodes": INSTANCE_NODE (2n - 1,), the top-level tree as it is on the device (made again first if the scene changed)}.
        A set made by build_instances has all three read from the device."""
        lib = load_library()
        n = int(lib.rt_instance_count(self._h))
        world, inverse = getattr(self, "_instance_transforms", np.zeros((0, 3, 4), np.float32)).copy(), np.zeros((n, 3, 4), np.float32)
        if getattr(self, "_instances_built", False):
            world = np.zeros((n, 3, 4), np.float32)
            _check(lib.rt_instances_world_from_object(self._h, world.ctypes.data))
        nodes = np.zeros(int(lib.rt_instance_node_count(self._h)), INSTANCE_NODE)
        _check(lib.rt_instances_object_from_world(self._h, inverse.ctypes.data))
        _check(lib.rt_instance_nodes(self._h, nodes.ctypes.data))
        return {"world_from_object": world, "object_from_world": inverse, "nodes": nodes}

    def trace_instances_closest(self, origins, directions, max_distance: float = 100000.0, outputs=INSTANCE_OUTPUTS,
                                sort: bool = True) -> dict:
        """Closest hit of every WORLD-space ray among the posed copies of the scene: the record of trace_closest -- position,
        distance and normal in world space, leaf and barycentrics of the copy's triangle -- and "instance", the copy
        (0xFFFFFFFF without a hit).  Inputs and forms as for trace_closest."""
        return Host._trace(self, "rt_trace_instances", INSTANCE_OUTPUTS, _instance_hits, True, origins, directions, max_distance, outputs, sort)

    def trace_instances_occluded(self, origins, directions, max_distance: float = 100000.0, sort: bool = True):
        """Occlusion of every world-space ray by any copy (the `hit` of trace_instances_closest): uint8 (N,)."""
        return Host._trace(self, "rt_trace_instances", INSTANCE_OUTPUTS, _instance_hits, False, origins, directions, max_distance, ("hit",),
                           sort)["hit"]

    # ---- instanced ambient occlusion (include/rt_hip_instance_views.h) ----
    def instances_ambient_occlusion(self, points, normals, seeds=None, outputs=AO_OUTPUTS, sort: bool = True) -> dict:
        """ambient_occlusion at WORLD-space points against the posed copies of the scene (set_instances): the rays
        ambient_occlusion makes for a point -- ao_rays writes them out --, each cast as trace_instances_occluded casts it with
        max_distance = ao_max_distance: {"ao": float32 (N,), "occluded": uint32 (N,)} (those named in `outputs`).  Inputs,
        seeds, sorting and the numpy / torch forms are ambient_occlusion's."""
        return Host._ao(self, "rt_trace_instances_ao", points, normals, seeds, outputs, sort)

    # ---- instanced multi-hit queries (include/rt_hip_instance_multihit.h) ----
    def trace_instances_multihit(self, origins, directions, max_distance: float = 100000.0, k: int = 4,
                                 outputs=INSTANCE_MULTIHIT_OUTPUTS, sort: bool = True) -> dict:
        """Everything a WORLD-space ray crosses among the posed copies of the scene (set_instances): trace_multihit's
        outputs -- "count": uint32 (N,), every (copy, triangle) pair the walks accept, whatever k; the first k of them by
        (distance, instance, leaf index), records as trace_instances_closest makes them -- and "instance": uint32 (N, k),
        the copy of every slot (0xFFFFFFFF in unused slots) (those named in `outputs`).  k, inputs and the numpy / torch
        forms are trace_multihit's."""
        return Host._multihit(self, "rt_trace_instances_multihit", INSTANCE_MULTIHIT_OUTPUTS, _instance_multihits, origins, directions,
                              max_distance, k, outputs, sort)

    def count_instances_hits(self, origins, directions, max_distance: float = 100000.0, sort: bool = True):
        """The number of (copy, triangle) pairs the walks accept for every world-space ray (trace_instances_multihit's
        "count", the k = 0 form that keeps no list): uint32 (N,)."""
        return self.trace_instances_multihit(origins, directions, max_distance, k=0, outputs=("count",), sort=sort)["count"]

    # ---- instanced directional occlusion (include/rt_hip_instance_directional.h) ----
    def instances_directional_occlusion(self, points, normals, seeds=None, outputs=DIRECTIONAL_OUTPUTS, sort: bool = True) -> dict:
        """directional_occlusion at WORLD-space points against the posed copies of the scene (set_instances): the rays of a
        point are ao_rays's, each cast as trace_instances_occluded casts it with max_distance = ao_max_distance; "mask",
        "occluded", "ao" and "bent" are made of those flags as directional_occlusion makes them ("occluded" and "ao" are
        instances_ambient_occlusion's).  Inputs, seeds, sorting and the numpy / torch forms are ambient_occlusion's."""
        return Host._directional(self, "rt_trace_instances_ao_directional", points, normals, seeds, outputs, sort)

    # ---- segment queries (include/rt_hip_segment.h) ----
    def segments_occluded(self, a, b, interval=SEGMENT_INTERVAL, sort: bool = True):
        """Line of sight: uint8 (N,), 1 iff something blocks the segment from a[i] to b[i] at a fraction r of it with
        interval[0] < r < interval[1].  a, b: (N, 3) / (N, 4) float32.  numpy in, numpy out (blocking); torch tensors on the
        host's GPU in, a torch tensor out, enqueued on torch.cuda.current_stream() without waiting (as for trace_occluded)."""
        return self._segments(False, a, b, interval, ("hit",), sort)["hit"]

    def segments_closest(self, a, b, interval=SEGMENT_INTERVAL, outputs=SEGMENT_OUTPUTS, sort: bool = True) -> dict:
        """The first blocker of every segment, the record of trace_closest: {"hit": uint8 (N,), "distance": float32 (N,) --
        a length from a[i], not a fraction --, "leaf", "barycentric", "position", "normal"} (those named in `outputs`);
        without a blocker: +inf, 0xFFFFFFFF, zeros.  Inputs and forms as for segments_occluded."""
        return self._segments(True, a, b, interval, tuple(outputs), sort)

    def _segments(self, closest: bool, a, b, interval, outputs, sort: bool, instanced: bool = False) -> dict:
        family, legal, wrap = (("rt_instances_segments", INSTANCE_OUTPUTS, _instance_hits) if instanced
                               else ("rt_segments", SEGMENT_OUTPUTS, _HitArrays))
        outputs = _known(outputs, legal)
        t_lo, t_hi = interval
        io = _QueryArrays(a, b, ("a", "b"), "points")
        out = io.outputs(outputs)
        args = (io.n, float(t_lo), float(t_hi), 0 if sort else RT_QUERY_NO_SORT)
        if closest:
            io.call(self._h, family + "_closest", *args, C.byref(wrap(*io.pointers(out, legal))))
        else:
            io.call(self._h, family + "_occluded", *args, *io.pointers(out, ("hit",)))
        return out

    def visibility(self, points, targets, interval=SEGMENT_INTERVAL, outputs=VISIBILITY_OUTPUTS, sort: bool = True) -> dict:
        """Every point against every target: {"mask": uint32 (P, W), W = ceil(T / 32) -- bit j & 31 of word j >> 5 of row i
        is 1 iff the segment from points[i] to targets[j] is occluded, padding bits 0 (unpack_visibility_mask makes booleans
        of it) --, "count": uint32 (P,), the row's popcount: the targets point i does NOT see} (those named in `outputs`).
        points: (P, 3) / (P, 4), targets: (T, 3) / (T, 4) float32, P T <= 2^27; the P x T rays are never written out.
        numpy / torch forms as for segments_occluded."""
        return self._visibility("rt_visibility_masks", points, targets, interval, outputs, sort)

    def _visibility(self, function: str, points, targets, interval, outputs, sort: bool) -> dict:
        outputs = _known(outputs, VISIBILITY_OUTPUTS)
        t_lo, t_hi = interval
        both = _is_torch(points), _is_torch(targets)
        if both[0] != both[1]:
            raise ValueError("points and targets must both be torch tensors or both numpy arrays")
        io = _QueryArrays(points, None, ("points",), "points")
        pad = _rays4_torch if io.torch else _rays4_numpy
        targets4 = pad(targets, "targets")
        if io.torch and targets4.device != io.a.device:
            raise ValueError("points and targets must be on the same device")
        nt = int(targets4.shape[0])
        words = (nt + 31) // 32
        out = io.outputs(outputs, shapes={"mask": (np.uint32, (words,))})
        pointers = [io.ptr(out[name]) if name in out and io.n and nt else None for name in VISIBILITY_OUTPUTS]
        if io.n and nt == 0:  # (nothing is launched: the rows have no words, every count is 0)
            for name in out:
                out[name][...] = 0
        io.call(self._h, function, io.n, io.ptr(targets4) if nt else None, nt, float(t_lo), float(t_hi),
                0 if sort else RT_QUERY_NO_SORT, C.byref(_VisibilityArrays(*pointers)))
        if io.torch and targets4 is not targets:  # (the padded copy must live until the kernels have read it)
            targets4.record_stream(io.current)
        return out

    # ---- instanced segment queries (include/rt_hip_instance_segments.h) ----
    def instances_segments_occluded(self, a, b, interval=SEGMENT_INTERVAL, sort: bool = True):
        """segments_occluded with every posed copy of the scene (set_instances) in the way: uint8 (N,), 1 iff some copy
        blocks the WORLD-space segment from a[i] to b[i] at a fraction r of it with interval[0] < r < interval[1].  Inputs
        and the numpy / torch forms as for segments_occluded."""
        return self._segments(False, a, b, interval, ("hit",), sort, instanced=True)["hit"]

    def instances_segments_closest(self, a, b, interval=SEGMENT_INTERVAL, outputs=INSTANCE_OUTPUTS, sort: bool = True) -> dict:
        """The first blocker of every world-space segment among the posed copies, the record of trace_instances_closest:
        position, distance (a length from a[i]) and normal in world space, leaf and barycentrics of the copy's triangle,
        and "instance", the copy (those named in `outputs`); without a blocker: +inf, 0xFFFFFFFF, zeros."""
        return self._segments(True, a, b, interval, tuple(outputs), sort, instanced=True)

    def instances_visibility(self, points, targets, interval=SEGMENT_INTERVAL, outputs=VISIBILITY_OUTPUTS, sort: bool = True) -> dict:
        """visibility with every posed copy of the scene in the way: the mask rows and counts of world-space points against
        world-space targets, laid out as visibility lays them out; the P x T rays are never written out."""
        return self._visibility("rt_instances_visibility_masks", points, targets, interval, outputs, sort)

    # ---- closest-point queries (include/rt_hip_nearest.h) ----
    def closest_points(self, points, max_distance: float = float("inf"), outputs=NEAREST_OUTPUTS, sort: bool = True) -> dict:
        """The nearest point of the surface for every point: {"hit": uint8 (N,), 1 iff the surface lies within max_distance;
        "distance": float32 (N,); "leaf": uint32 (N,); "barycentric", "position", "normal": float32 (N, 3)} (those named in
        `outputs`); without one: +inf, 0xFFFFFFFF, zeros.  points: (N, 3) / (N, 4) float32.  numpy in, numpy out (blocking);
        a torch tensor on the host's GPU in, torch tensors out, enqueued on torch.cuda.current_stream() without waiting (as
        for trace_closest)."""
        return Host._points(self, "rt_closest_points", NEAREST_OUTPUTS, _HitArrays, points, max_distance, outputs, sort)

    def _points(self, function: str, legal: tuple, wrap, points, max_distance: float, outputs, sort: bool) -> dict:
        """The closest-point queries, plain, signed and instanced: `function` with wrap(the pointers of `legal`)."""
        outputs = _known(outputs, legal)
        io = _QueryArrays(points, None, ("points",), "points")
        out = io.outputs(outputs)
        io.call(self._h, function, io.n, float(max_distance), 0 if sort else RT_QUERY_NO_SORT, C.byref(wrap(*io.pointers(out, legal))))
        return out

    # ---- signed distance queries (include/rt_hip_signed.h) ----
    def signed_distance(self, points, max_distance: float = float("inf"), outputs=SIGNED_OUTPUTS, sort: bool = True) -> dict:
        """closest_points with a sign: the same record, "distance" negative where the point lies inside a closed, outward
        oriented mesh -- by the angle-weighted pseudonormal of the vertex, edge or face the nearest point lies on --, and
        "feature": uint8 (N,), an index into FEATURES (0xFF: nothing within max_distance); "pseudonormal": float32 (N, 4), that
        feature's pseudonormal and its dot product with point - position.  Inputs and the numpy / torch forms as for
        closest_points.  The first call after an upload or a build makes the sign table (prepare_signed_distance)."""
        return Host._points(self, "rt_signed_distance", SIGNED_OUTPUTS, lambda *at: _SignedArrays(_HitArrays(*at[:6]), at[6], at[7]), points,
                            max_distance, outputs, sort)

    def signed_distance_grid(self, origin, spacing, shape, max_distance: float = float("inf"), as_torch: bool = False, leaf: bool = False):
        """The signed distance field of the scene on a regular grid: float32 (nz, ny, nx) for shape = (nx, ny, nz), voxel
        [k, j, i] at origin + (i, j, k) * spacing (float32, each coordinate origin + float32(i) * spacing), +inf where
        nothing lies within max_distance; every voxel is, bit for bit, signed_distance's answer for that point.  leaf=True:
        (distances, uint32 leaves of the same shape).  A numpy array (blocking), or with as_torch=True a torch tensor on the
        host's GPU, enqueued on torch.cuda.current_stream() without waiting."""
        o = np.ascontiguousarray(origin, np.float32).reshape(3)
        sp = np.ascontiguousarray(np.broadcast_to(np.asarray(spacing, np.float32), (3,)))
        dims = np.ascontiguousarray([int(x) for x in shape], np.int64).reshape(3)
        if (dims < 0).any() or (dims >= 1 << 32).any():
            raise ValueError("shape: expected three counts (nx, ny, nz)")
        if int(dims[0]) * int(dims[1]) * int(dims[2]) > 1 << 31:  # (before anything of that size is allocated)
            raise RtError(RT_E_INVALID, "signed_distance_grid: more than 2^31 voxels in one grid")
        dims = dims.astype(np.uint32)
        lib, nzyx = load_library(), (int(dims[2]), int(dims[1]), int(dims[0]))
        if as_torch:
            import torch

            device = torch.device("cuda", self._device)
            d = torch.empty(nzyx, dtype=torch.float32, device=device)
            l = torch.empty(nzyx, dtype=torch.uint32, device=device) if leaf else None
            _check(lib.rt_signed_distance_grid_device(self._h, o.ctypes.data, sp.ctypes.data, dims.ctypes.data, float(max_distance),
                                                      d.data_ptr() or 4, None if l is None else l.data_ptr() or 4,
                                                      torch.cuda.current_stream(device).cuda_stream))
        else:
            d = np.empty(nzyx, np.float32)
            l = np.empty(nzyx, np.uint32) if leaf else None
            _check(lib.rt_signed_distance_grid(self._h, o.ctypes.data, sp.ctypes.data, dims.ctypes.data, float(max_distance),
                                               d.ctypes.data, None if l is None else l.ctypes.data))
        return (d, l) if leaf else d

    def prepare_signed_distance(self) -> None:
        """Makes the signed queries' sign table now (rt_prepare_signed_distance), so that the first query does not."""
        _check(load_library().rt_prepare_signed_distance(self._h))

    def last_sign_build_ms(self) -> float:
        """HIP-event time of the last build or refresh of the sign table, ms (0.0 before the first)."""
        return float(load_library().rt_last_sign_build_ms(self._h))

    def sign_table(self) -> np.ndarray:
        """(rt_debug_sign_table, for tests) The sign table as the device holds it: SIGN_RECORD (leaves,) -- per leaf the
        pseudonormals of the edges AB, AC, BC (.w: the face's unit normal) and of the vertices A, B, C (.w: the corner angles)."""
        lib, leaves = load_library(), C.c_uint32()
        _check(lib.rt_debug_record_counts(self._h, None, C.byref(leaves)))
        out = np.zeros(leaves.value, SIGN_RECORD)
        _check(lib.rt_debug_sign_table(self._h, out.ctypes.data or 4))
        return out

    # ---- instanced closest-point queries (include/rt_hip_instance_nearest.h) ----
    def instances_closest_points(self, points, max_distance: float = float("inf"), outputs=INSTANCE_OUTPUTS, sort: bool = True) -> dict:
        """The nearest point of the surface among the posed copies of the scene (set_instances) for every WORLD-space point:
        the record of closest_points in world space -- distance, position, normal; leaf and barycentrics of the copy's
        triangle -- and "instance", the copy (those named in `outputs`); without one: +inf, 0xFFFFFFFF, zeros.  Inputs and
        the numpy / torch forms as for closest_points."""
        return Host._points(self, "rt_instances_closest_points", INSTANCE_OUTPUTS, _instance_hits, points, max_distance, outputs, sort)

    def set_nearest_walk(self, no_start: bool = False, no_prune: bool = False, count: bool = False) -> None:
        """(rt_debug_set_nearest_walk) How later closest_points and instances_closest_points calls walk; anything but the
        default needs the A/B build."""
        _check(load_library().rt_debug_set_nearest_walk(self._h, (1 if no_start else 0) | (2 if no_prune else 0) | (4 if count else 0)))

    def last_nearest_counts(self) -> tuple:
        """(rt_debug_last_nearest_counts) (box tests, triangle tests) of the last counted closest_points call, over its points."""
        nodes, tris = C.c_uint64(), C.c_uint64()
        _check(load_library().rt_debug_last_nearest_counts(self._h, C.byref(nodes), C.byref(tris)))
        return int(nodes.value), int(tris.value)

    # ---- multi-hit queries (include/rt_hip_multihit.h) ----
    def trace_multihit(self, origins, directions, max_distance: float = 100000.0, k: int = 4, outputs=MULTIHIT_OUTPUTS,
                       sort: bool = True) -> dict:
        """Everything a ray crosses: {"count": uint32 (N,), the number of triangles the reference's walk accepts for the ray
        (all of them, whatever k); "distance" / "leaf": (N, k), "barycentric" / "position" / "normal": (N, k, 3), the first
        k of them by (distance, leaf index), unused slots filled with +inf / 0xFFFFFFFF / 0} (those named in `outputs`).
        0 <= k <= RT_MULTIHIT_MAX_K; with k = 0 only "count" can be asked for.  numpy (N, 3) / (N, 4) float32 in, numpy
        out (blocking); torch tensors on the host's GPU in, torch tensors out, enqueued on torch.cuda.current_stream()
        without waiting (as for trace_closest)."""
        return Host._multihit(self, "rt_trace_multihit", MULTIHIT_OUTPUTS, _MultiHitArrays, origins, directions, max_distance, k, outputs, sort)

    def _multihit(self, function: str, legal: tuple, wrap, origins, directions, max_distance: float, k: int, outputs, sort: bool) -> dict:
        """The multi-hit queries, plain and instanced: `function` with wrap(the pointers of `legal`)."""
        outputs = _known(outputs, legal)
        k = int(k)
        if k < 0:
            raise ValueError("k must not be negative")
        io = _QueryArrays(origins, directions, ("origins", "directions"), "rays")
        out = io.outputs(outputs, k, shapes={"instance": (np.uint32, (k,))})
        arrays = wrap(*io.pointers(out, legal, name_empty=True))
        io.call(self._h, function, io.n, float(max_distance), k, 0 if sort else RT_QUERY_NO_SORT, C.byref(arrays))
        return out

    def count_hits(self, origins, directions, max_distance: float = 100000.0, sort: bool = True):
        """The number of triangles the reference's walk accepts for every ray (trace_multihit's "count", the k = 0 form
        that keeps no list): uint32 (N,)."""
        return self.trace_multihit(origins, directions, max_distance, k=0, outputs=("count",), sort=sort)["count"]

    @property
    def last_query_ms(self) -> float:
        """HIP-event time of the last query's kernels (sort + walk), ms: a ray query, a multi-hit query or an ambient-occlusion
        query."""
        return float(load_library().rt_last_query_ms(self._h))

    # ---- ambient-occlusion queries (include/rt_hip_ao.h) ----
    @property
    def ao_rays_per_point(self) -> tuple:
        """(rays the reference casts per point with this host's options, the n of `1 - hits / n`)."""
        rays, divisor = C.c_uint32(), C.c_uint32()
        _check(load_library().rt_ao_rays_per_point(self._h, C.byref(rays), C.byref(divisor)))
        return int(rays.value), int(divisor.value)

    def ambient_occlusion(self, points, normals, seeds=None, outputs=AO_OUTPUTS, sort: bool = True) -> dict:
        """The reference's ambient_occlusion() at every point with this host's AO options: {"ao": float32 (N,), "occluded":
        uint32 (N,)} (those named in `outputs`).  points / normals: (N, 3) / (N, 4) float32, the normals used as given;
        seeds: uint32 (N,) -- the reference's `index` of a point, used by the RANDOM method only -- or None: 0 .. N-1.
        numpy in, numpy out (blocking); torch tensors on the host's GPU in, torch tensors out, enqueued on
        torch.cuda.current_stream() without waiting (as for the ray queries, the default stream's handle is NULL, which
        the library reads as the host's own stream: work under a stream of your own, or synchronise around the call)."""
        return Host._ao(self, "rt_trace_ao", points, normals, seeds, outputs, sort)

    def _ao(self, function: str, points, normals, seeds, outputs, sort: bool) -> dict:
        """The ambient-occlusion queries, plain and instanced."""
        outputs = _known(outputs, AO_OUTPUTS)
        io = _QueryArrays(points, normals, ("points", "normals", "seeds"), "points", also=seeds)
        if seeds is not None:
            seeds = io.seeds(seeds)
        out = io.outputs(outputs)
        io.call(self._h, function, io.ptr(seeds) if seeds is not None and io.n else None, io.n, 0 if sort else RT_QUERY_NO_SORT,
                *io.pointers(out, AO_OUTPUTS))
        return out

    # ---- directional occlusion queries (include/rt_hip_directional.h) ----
    @property
    def ao_mask_words(self) -> int:
        """W: the uint32 words of a point's mask row, ceil(rays per point / 32)."""
        words = C.c_uint32()
        _check(load_library().rt_ao_mask_words(self._h, C.byref(words)))
        return int(words.value)

    def directional_occlusion(self, points, normals, seeds=None, outputs=DIRECTIONAL_OUTPUTS, sort: bool = True) -> dict:
        """Which of every point's ambient-occlusion rays were blocked, and what follows from that: {"mask": uint32 (N, W) --
        bit k & 31 of word k >> 5 is 1 iff ray k of the point was blocked (unpack_ao_mask makes booleans of it) --,
        "occluded": uint32 (N,), the row's popcount, "ao": float32 (N,) -- both as ambient_occlusion returns them --,
        "bent": float32 (N, 3), the sum of the directions of the point's open rays, added in ray order and not normalised}
        (those named in `outputs`).  Ray k is the k-th ray the reference's ambient_occlusion() casts; ao_rays returns
        the rays themselves.  Inputs, seeds, sorting and the numpy / torch forms are ambient_occlusion's."""
        return Host._directional(self, "rt_trace_ao_directional", points, normals, seeds, outputs, sort)

    def _directional(self, function: str, points, normals, seeds, outputs, sort: bool) -> dict:
        """The directional occlusion queries, plain and instanced."""
        outputs = _known(outputs, DIRECTIONAL_OUTPUTS)
        io = _QueryArrays(points, normals, ("points", "normals", "seeds"), "points", also=seeds)
        if seeds is not None:
            seeds = io.seeds(seeds)
        out = io.outputs(outputs, shapes={"mask": (np.uint32, (self.ao_mask_words,))} if "mask" in outputs else None)
        arrays = _DirectionalArrays(*io.pointers(out, DIRECTIONAL_OUTPUTS))
        io.call(self._h, function, io.ptr(seeds) if seeds is not None and io.n else None, io.n, 0 if sort else RT_QUERY_NO_SORT,
                C.byref(arrays))
        return out

    def ao_rays(self, points, normals, seeds=None) -> dict:
        """The rays ambient_occlusion and directional_occlusion cast: {"origins": float32 (N, 4), "directions": float32
        (N, R, 4)}, direction k of point i at [i, k], the fourth component 0; R = ao_rays_per_point[0].  The directions are
        as cast: not normalised where the reference does not normalise them.  No ray is walked.  Inputs, seeds and the
        numpy / torch forms are ambient_occlusion's."""
        io = _QueryArrays(points, normals, ("points", "normals", "seeds"), "points", also=seeds)
        if seeds is not None:
            seeds = io.seeds(seeds)
        rays = self.ao_rays_per_point[0]
        out = io.outputs(("origins", "directions"), shapes={"origins": (np.float32, (4,)), "directions": (np.float32, (rays, 4))})
        io.call(self._h, "rt_ao_rays", io.ptr(seeds) if seeds is not None and io.n else None, io.n,
                *io.pointers(out, ("origins", "directions")))
        return out

    def vertex_bent_normals(self, scene: "Scene") -> np.ndarray:
        """Per-vertex bent-normal baking: directional_occlusion(scene.vertices, scene.vnormals)["bent"], the raw sum of the
        open rays' directions per vertex of the file, in its order (as vertex_ao is for "ao"); normalise, or divide by the
        number of open rays, as the use demands.  A vertex with a zero normal gets what the arithmetic gives: not a number."""
        return self.directional_occlusion(scene.vertices, scene.vnormals, outputs=("bent",))["bent"]

    # ---- frame layers (include/rt_hip_layers.h) ----
    def render_layers(self, outputs=LAYER_OUTPUTS, as_torch: bool = False) -> dict:
        """The layers behind the frame's grey image, per sub-pixel, for the rays the frame itself casts: {output name:
        (H, W) or (H, W, 3) array} with H x W = total_height x total_width (those named in `outputs`; a host whose options
        have ambient occlusion off has no "ao": leave it out).  "value" holds the bits download() returns after render().
        numpy out (blocking), or with as_torch=True torch tensors on the host's GPU, enqueued on
        torch.cuda.current_stream() without waiting (as for the ray queries, the default stream's handle is NULL, which the
        library reads as the host's own stream: work under a stream of your own, or synchronise around the call)."""
        outputs = _known(outputs, LAYER_OUTPUTS)
        h, w = self.options.total_height, self.options.total_width
        shapes = {name: (h, w) + ((_OUTPUT_LAYOUT[name][1],) if _OUTPUT_LAYOUT[name][1] > 1 else ()) for name in outputs}
        lib = load_library()
        if as_torch:
            import torch

            # (the host's GPU: the index it was created on; -1 stands for OCRT_DEVICE or 0, as in the library)
            index = getattr(self, "_device", -1)
            device = torch.device("cuda", index if index >= 0 else int(os.environ.get("OCRT_DEVICE", "0")))
            out = {name: torch.empty(shape, dtype=getattr(torch, np.dtype(_OUTPUT_LAYOUT[name][0]).name), device=device)
                   for name, shape in shapes.items()}
            arrays = _LayerArrays(*[out[name].data_ptr() if name in out else None for name in LAYER_OUTPUTS])
            _check(lib.rt_render_layers_device(self._h, C.byref(arrays), torch.cuda.current_stream(device).cuda_stream))
            return out
        out = {name: np.empty(shape, dtype=_OUTPUT_LAYOUT[name][0]) for name, shape in shapes.items()}
        arrays = _LayerArrays(*[out[name].ctypes.data if name in out else None for name in LAYER_OUTPUTS])
        _check(lib.rt_render_layers(self._h, C.byref(arrays)))
        return out

    # ---- multi-view rendering (include/rt_hip_views.h) ----
    def render_views(self, cameras, outputs=("value",), as_torch: bool = False) -> dict:
        """The frame layers and the finished 8-bit image of V poses against the uploaded scene, in one call and without a
        new upload: {output name: (V, H, W) or (V, H, W, 3) array} with H x W = total_height x total_width, and "image":
        (V, height, width) uint8 (those named in `outputs`, from VIEW_OUTPUTS).  View v's block of a layer is what
        render_layers returns on a host that was given cameras[v] with set_camera before its upload; "image" is what its
        download_u8() returns after render().  `cameras`: a sequence of Camera, or a (V, 4, 3) float32 array (eye, right,
        up, forward per view, used as given).  The host's own pose plays no part.  numpy out (blocking), or with
        as_torch=True torch tensors on the host's GPU, enqueued on torch.cuda.current_stream() (the rules are
        render_layers')."""
        return self._render_views(cameras, tuple(outputs), as_torch, VIEW_OUTPUTS)

    # ---- instanced views (include/rt_hip_instance_views.h) ----
    def render_instance_views(self, cameras, outputs=("value",), as_torch: bool = False) -> dict:
        """render_views of the posed copies of the scene (set_instances): every layer, the finished 8-bit image, and
        "instance": uint32 (V, H, W), the copy a sub-pixel's record lies in (0xFFFFFFFF without a hit) (those named in
        `outputs`, from INSTANCE_VIEW_OUTPUTS).  The record layers are trace_instances_closest's for the view's own rays, in
        world space; "ao" is instances_ambient_occlusion at the record's position and normal; "value" and "image" are made
        of them as render_views makes them.  Cameras and the numpy / torch forms are render_views'."""
        return self._render_views(cameras, tuple(outputs), as_torch, INSTANCE_VIEW_OUTPUTS)

    def _render_views(self, cameras, outputs: tuple, as_torch: bool, legal: tuple) -> dict:
        outputs = _known(outputs, legal)
        instanced = legal is INSTANCE_VIEW_OUTPUTS
        if isinstance(cameras, np.ndarray):
            if cameras.dtype != np.float32 or cameras.ndim != 3 or cameras.shape[1:] != (4, 3):
                raise ValueError("cameras: expected a float32 array of shape (V, 4, 3), or a sequence of Camera")
            poses = np.ascontiguousarray(cameras)
        else:
            cameras = list(cameras)
            if not all(isinstance(c, Camera) for c in cameras):
                raise ValueError("cameras: expected a sequence of Camera, or a float32 array of shape (V, 4, 3)")
            poses = np.array([c.as_array() for c in cameras], dtype=np.float32).reshape(-1, 4, 3)
        views = int(poses.shape[0])
        h, w = self.options.total_height, self.options.total_width
        shapes = {name: (views, self.options.height, self.options.width) if name == "image" else
                  (views, h, w) + ((_OUTPUT_LAYOUT[name][1],) if _OUTPUT_LAYOUT[name][1] > 1 else ()) for name in outputs}
        dtypes = {name: np.uint8 if name == "image" else _OUTPUT_LAYOUT[name][0] for name in outputs}
        lib = load_library()
        if as_torch:
            import torch

            index = getattr(self, "_device", -1)
            device = torch.device("cuda", index if index >= 0 else int(os.environ.get("OCRT_DEVICE", "0")))
            out = {name: torch.empty(shape, dtype=getattr(torch, np.dtype(dtypes[name]).name), device=device)
                   for name, shape in shapes.items()}
            address = lambda t: t.data_ptr()
        else:
            out = {name: np.empty(shape, dtype=dtypes[name]) for name, shape in shapes.items()}
            address = lambda a: a.ctypes.data
        # (an array that holds nothing is not named: V = 0 asks for nothing)
        pointers = [address(out[name]) if name in out and views else None for name in INSTANCE_VIEW_OUTPUTS]
        arrays = _ViewArrays(_LayerArrays(*pointers[:-2]), pointers[-2])
        function = "rt_render_views"
        if instanced:
            arrays, function = _InstanceViewArrays(arrays, pointers[-1]), "rt_render_instance_views"
        if as_torch:
            _check(getattr(lib, function + "_device")(self._h, poses.ctypes.data, views, C.byref(arrays),
                                                      torch.cuda.current_stream(device).cuda_stream))
        else:
            _check(getattr(lib, function)(self._h, poses.ctypes.data, views, C.byref(arrays)))
        return out

    def set_views_chunk(self, max_views: int) -> None:
        """Test aid (include/rt_hip_debug.h, rt_debug_set_views_chunk): at most `max_views` views per chunk of a
        render_views call; 0: as many as fit.  Same results."""
        _check(load_library().rt_debug_set_views_chunk(self._h, int(max_views)))

    def last_views(self) -> dict:
        """What the last render_views call did (include/rt_hip_debug.h, rt_debug_last_views): {"views", "chunks",
        "ao_points": the sub-pixels its ambient-occlusion step ran over -- the hit ones}."""
        views, chunks, points = C.c_uint32(), C.c_uint32(), C.c_uint64()
        _check(load_library().rt_debug_last_views(self._h, C.byref(views), C.byref(chunks), C.byref(points)))
        return {"views": views.value, "chunks": chunks.value, "ao_points": points.value}

    # ---- vertex updates (include/rt_hip_update.h) ----
    def update_vertices(self, vertices, vnormals=None) -> None:
        """Refits the uploaded scene on the device to new vertex positions, without a new upload (rt_update_vertices):
        `vertices` (V, 3) or (V, 4) float32 replaces every position -- V must be the upload's --, `vnormals` the shading
        normals (None: they stay as uploaded; Scene.refit recomputes them on the CPU).  numpy arrays (blocking; refuses
        coordinates that are not finite or exceed 1e37), or torch tensors on the host's GPU, enqueued on
        torch.cuda.current_stream() without waiting (the rules are the queries').  Every query, render_layers and
        render_views see the update; render() raises RtError -4 until the next upload."""
        given = [vertices] + ([] if vnormals is None else [vnormals])
        on_device = any(_is_torch(x) for x in given)
        if on_device and not all(_is_torch(x) for x in given):
            raise ValueError("vertices and vnormals must both be torch tensors or both numpy arrays")
        pad = _rays4_torch if on_device else _rays4_numpy
        v = pad(vertices, "vertices")
        n = None if vnormals is None else pad(vnormals, "vnormals")
        if n is not None and (n.shape[0] != v.shape[0] or (on_device and n.device != v.device)):
            raise ValueError("vertices and vnormals must hold the same number of vertices" + (" on the same device" if on_device else ""))
        lib = load_library()
        if on_device:
            import torch

            current = torch.cuda.current_stream(v.device)
            _check(lib.rt_update_vertices_device(self._h, v.data_ptr(), None if n is None else n.data_ptr(), int(v.shape[0]),
                                                 current.cuda_stream))
            for t, was in ((v, vertices), (n, vnormals)):  # (the padded copies must live until the kernels have read them)
                if t is not None and t is not was:
                    t.record_stream(current)
        else:
            _check(lib.rt_update_vertices(self._h, v.ctypes.data, None if n is None else n.ctypes.data, int(v.shape[0])))

    @property
    def last_update_ms(self) -> float:
        """HIP-event time of the last update_vertices' kernels, ms (0.0 before the first)."""
        return float(load_library().rt_last_update_ms(self._h))

    # ---- device-side builds (include/rt_hip_build.h) ----
    def build_scene(self, vertices, faces, vnormals=None) -> None:
        """Builds the scene ON the device from triangles (rt_build_scene): `vertices` (V, 3) or (V, 4) float32, `faces`
        (F, 3) vertex ids, `vnormals` like vertices.  The new scene replaces the host's (or comes first); every query,
        render_layers, render_views and update_vertices work on it, render() raises RtError -4 until the next upload;
        `leaf` indices count in the build's order: face_of_leaf.  numpy arrays (blocking; vnormals None: computed on the CPU
        as Scene.from_arrays does; refuses a face index >= V and coordinates that are not finite or exceed 1e37), or torch
        tensors on the host's GPU (faces int32 or int64; vnormals required), enqueued on torch.cuda.current_stream() -- the
        call waits for it once; a face index out of range is found on the device: RtError -1, the previous scene stays."""
        given = [vertices, faces] + ([] if vnormals is None else [vnormals])
        on_device = any(_is_torch(x) for x in given)
        if on_device and not all(_is_torch(x) for x in given):
            raise ValueError("vertices, faces and vnormals must all be torch tensors or all numpy arrays")
        pad = _rays4_torch if on_device else _rays4_numpy
        v = pad(vertices, "vertices")
        n = None if vnormals is None else pad(vnormals, "vnormals")
        if n is not None and (n.shape[0] != v.shape[0] or (on_device and n.device != v.device)):
            raise ValueError("vertices and vnormals must hold the same number of vertices" + (" on the same device" if on_device else ""))
        lib = load_library()
        if on_device:
            import torch

            if n is None:
                raise RtError(RT_E_INVALID, "build_scene: the device form needs vnormals (the device does not compute vertex normals)")
            if faces.dtype not in (torch.int32, torch.int64) or faces.device != v.device:
                raise ValueError("faces: expected an int32 or int64 tensor on the vertices' device")
            f = faces.reshape(-1).to(torch.int32).contiguous()  # (the bits of a uint32 id below 2^31)
            if f.numel() % 3:
                raise ValueError("faces must hold 3 vertex ids per triangle")
            current = torch.cuda.current_stream(v.device)
            _check(lib.rt_build_scene_device(self._h, v.data_ptr(), n.data_ptr(), int(v.shape[0]), f.data_ptr(), f.numel() // 3,
                                             current.cuda_stream))
        else:
            f = np.ascontiguousarray(faces, dtype=np.uint32).reshape(-1)
            if f.size % 3:
                raise ValueError("faces must hold 3 vertex ids per triangle")
            _check(lib.rt_build_scene(self._h, v.ctypes.data, None if n is None else n.ctypes.data, int(v.shape[0]), f.ctypes.data,
                                      f.size // 3))

    def face_of_leaf(self, leaf=None) -> np.ndarray:
        """Scene.face_of_leaf for the scene this host built (rt_built_faces): the file-order face a query's `leaf` index
        stands for; without an argument the whole map.  Leaves of 0xFFFFFFFF (no hit) map to 0xFFFFFFFF.  RtError -4 where
        the host's scene was uploaded, not built."""
        lib, leaves = load_library(), C.c_uint32()
        _check(lib.rt_debug_record_counts(self._h, None, C.byref(leaves)))
        faces = np.zeros(leaves.value, np.uint32)
        _check(lib.rt_built_faces(self._h, faces.ctypes.data))
        if leaf is None:
            return faces
        leaf = np.asarray(leaf, dtype=np.uint32)
        miss = leaf == 0xFFFFFFFF
        return np.where(miss, np.uint32(0xFFFFFFFF), faces[np.where(miss, 0, leaf)]).astype(np.uint32)

    @property
    def last_build_ms(self) -> float:
        """HIP-event time of the last build_scene's kernels, ms (0.0 before the first)."""
        return float(load_library().rt_last_build_ms(self._h))

    def last_build_times(self) -> dict:
        """Where the last build's time went (include/rt_hip_debug.h, rt_debug_last_build_times), ms: the topology's kernels,
        the records' kernels, the host's schedule step between them."""
        ms = (C.c_float * 3)()
        _check(load_library().rt_debug_last_build_times(self._h, ms))
        return {"topology_ms": float(ms[0]), "records_ms": float(ms[1]), "schedule_host_ms": float(ms[2])}

    def set_refit_group(self, nodes: int) -> None:
        """Test aid (include/rt_hip_debug.h, rt_debug_set_refit_group): at most `nodes` inner nodes per group of an update's
        schedule; 0: the default.  Same results."""
        _check(load_library().rt_debug_set_refit_group(self._h, int(nodes)))

    def records(self) -> dict:
        """The scene on the device as every query walks it (include/rt_hip_debug.h, rt_debug_download_records): {"nodes":
        NODE_RECORD (N,), "tris": TRI_RECORD (T,), "shade": SHADE_RECORD (T,)} structured arrays, taken once everything
        enqueued has finished."""
        lib, nodes, leaves = load_library(), C.c_uint32(), C.c_uint32()
        _check(lib.rt_debug_record_counts(self._h, C.byref(nodes), C.byref(leaves)))
        out = {"nodes": np.zeros(nodes.value, NODE_RECORD), "tris": np.zeros(leaves.value, TRI_RECORD),
               "shade": np.zeros(leaves.value, SHADE_RECORD)}
        _check(lib.rt_debug_download_records(self._h, out["nodes"].ctypes.data, out["tris"].ctypes.data, out["shade"].ctypes.data))
        return out

    def vertex_ao(self, scene: "Scene") -> np.ndarray:
        """Per-vertex AO baking: ambient_occlusion(scene.vertices, scene.vnormals)["ao"], one value per vertex of the file, in
        its order.  A vertex with a zero normal (one no face uses) gets the reference's answer for a zero normal: its
        tangent frame is not a number, none of its rays hits anything, the value is 1.0."""
        return self.ambient_occlusion(scene.vertices, scene.vnormals, outputs=("ao",))["ao"]


class FrameRing:
    """rt_ring: several render hosts of one scene on one GPU that take frames in turn (include/rt_hip_ring.h, "frame
    ring").  The library owns the hosts, their streams and captured graphs, the frame bookkeeping and -- with a
    communicator attached -- the band gather; this class only forwards.  `submit()` enqueues a frame and returns at
    once, `collect()` waits for the oldest one, `run(k)` is k steps of a steady stream in ONE call into the library."""

    def __init__(self, options: Options, scene: Optional["Scene"] = None, device: int = 0, rank: int = 0, nranks: int = 1,
                 hosts: int = 3, camera: Optional[Camera] = None):
        self.options = options
        self._r = load_library().rt_ring_create(C.byref(options), device, rank, nranks, hosts)
        if not self._r:
            _raise_last()
        if camera is not None:  # (before the upload: the pose is fixed per upload)
            self.set_camera(camera)
        if scene is not None:
            self.upload_scene(scene)

    def set_camera(self, camera: Camera) -> None:
        """The pose of all the ring's hosts (include/rt_hip_camera.h, rt_ring_set_camera): before the upload only."""
        _check(load_library().rt_ring_set_camera(self._r, C.byref(camera)))

    def close(self) -> None:
        if getattr(self, "_r", None):
            # the hosts handed out by host() point into the ring: they die with it
            for ref in getattr(self, "_lent", []):
                h = ref()
                if h is not None:
                    h._h = None
                    h._owner = None
            self._lent = []
            load_library().rt_ring_destroy(self._r)
            self._r = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload_scene(self, scene: "Scene") -> None:
        _check(load_library().rt_ring_upload_scene(self._r, scene._h))

    def set_gather_timeout(self, seconds: float) -> None:
        """The exchange step waits at most this long (default 30 s) for a frame's gather, then fails with RtError."""
        _check(load_library().rt_ring_set_gather_timeout(self._r, float(seconds)))

    def rccl_info(self):
        """(ranks of the attached communicator by ncclCommCount, RCCL version code by ncclGetVersion); -1 = unknown."""
        a, b = C.c_int(), C.c_int()
        _check(load_library().rt_ring_rccl_info(self._r, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def set_calibration(self, on: bool) -> None:
        """Before an upload: whether the upload measures which form of the AO pass suits the scene (default: yes)."""
        _check(load_library().rt_ring_set_calibration(self._r, int(on)))

    def calibration(self):
        """(ms per ao_kernel without the look-ahead loads, with them -- 0.0: not measured --, whether they are in use)."""
        a, b, c = C.c_float(), C.c_float(), C.c_int()
        _check(load_library().rt_ring_calibration(self._r, C.byref(a), C.byref(b), C.byref(c)))
        return float(a.value), float(b.value), bool(c.value)

    def device_bytes(self):
        """(bytes of the scene's arrays on the device, copies of them among the hosts -- one --, bytes of everything requested)."""
        a, c, t = C.c_uint64(), C.c_uint32(), C.c_uint64()
        _check(load_library().rt_ring_device_bytes(self._r, C.byref(a), C.byref(c), C.byref(t)))
        return int(a.value), int(c.value), int(t.value)

    @property
    def size(self) -> int:
        return load_library().rt_ring_size(self._r)

    @property
    def slots(self) -> int:
        """Band buffers (2 x size): frame f is rendered into buffer f % slots."""
        return load_library().rt_ring_slots(self._r)

    @property
    def local_rows(self) -> int:
        return load_library().rt_ring_local_rows(self._r)

    @property
    def in_flight(self) -> int:
        return load_library().rt_ring_in_flight(self._r)

    def host(self, slot: int) -> "Host":
        """Host `slot` as a borrowed Host (statistics, timers, downloads of its last frame)."""
        h = load_library().rt_ring_host(self._r, slot)
        if not h:
            raise IndexError(slot)
        host = Host._borrowed(self.options, h, owner=self)  # (the view keeps the ring alive)
        if not hasattr(self, "_lent"):
            self._lent = []
        self._lent = [r for r in self._lent if r() is not None]
        self._lent.append(weakref.ref(host))
        return host

    @property
    def hosts(self):
        return [self.host(k) for k in range(self.size)]

    def set_graph_mode(self, on: bool) -> None:
        _check(load_library().rt_ring_set_graph_mode(self._r, int(on)))

    def set_pacing(self, beta: float) -> None:
        """0: submit as soon as a host is free; default 0.5 (include/rt_hip_ring.h, rt_ring_set_pacing)."""
        _check(load_library().rt_ring_set_pacing(self._r, float(beta)))

    def bind_output(self, slot: int, device_ptr: int) -> None:
        _check(load_library().rt_ring_bind_output(self._r, slot, device_ptr))

    def submit(self) -> int:
        f = C.c_uint64()
        _check(load_library().rt_ring_submit(self._r, C.byref(f)))
        return int(f.value)

    def collect_info(self):
        """Waits for the oldest frame; returns (frame number, slot, device address of its bands)."""
        f, s, p = C.c_uint64(), C.c_uint32(), C.c_void_p()
        _check(load_library().rt_ring_collect(self._r, C.byref(f), C.byref(s), C.byref(p)))
        return int(f.value), int(s.value), int(p.value or 0)

    def collect(self) -> np.ndarray:
        """Waits for the oldest frame and returns its 8-bit image (an unpartitioned ring, or rank 0 of a gathering one)."""
        self.collect_info()
        return self.download_last()

    def step(self) -> None:
        _check(load_library().rt_ring_step(self._r))

    def run(self, frames: int) -> None:
        _check(load_library().rt_ring_run(self._r, int(frames)))

    def drain(self) -> None:
        _check(load_library().rt_ring_drain(self._r))

    def last_image_device(self) -> int:
        p = C.c_void_p()
        _check(load_library().rt_ring_last_image_device(self._r, C.byref(p)))
        return int(p.value or 0)

    def download_last(self) -> np.ndarray:
        img = np.empty((self.options.height, self.options.width), dtype=np.uint8)
        _check(load_library().rt_ring_download_last(self._r, img.ctypes.data))
        return img

    def reset_clock(self) -> None:
        _check(load_library().rt_ring_reset_clock(self._r))

    def keep_frame_times(self, on: bool = True) -> None:
        _check(load_library().rt_ring_keep_frame_times(self._r, int(on)))

    def frame_times(self, frame: int):
        """(begin, ao begin, ao end, end) of a collected frame in ms since reset_clock()."""
        t = (C.c_float * 4)()
        _check(load_library().rt_ring_frame_times(self._r, frame, t))
        return tuple(float(x) for x in t)

    def timers(self) -> dict:
        k, a, nk, na = C.c_double(), C.c_double(), C.c_uint64(), C.c_uint64()
        _check(load_library().rt_ring_timers(self._r, C.byref(k), C.byref(nk), C.byref(a), C.byref(na)))
        return {"kernel_ms": k.value, "frames": int(nk.value), "ao_ms": a.value, "ao_frames": int(na.value)}

    def reset_timers(self) -> None:
        load_library().rt_ring_reset_timers(self._r)

    def cpu_times(self) -> dict:
        a, b, c, n = C.c_double(), C.c_double(), C.c_double(), C.c_uint64()
        _check(load_library().rt_ring_cpu_times(self._r, C.byref(a), C.byref(b), C.byref(c), C.byref(n)))
        return {"submit_s": a.value, "wait_s": b.value, "collect_s": c.value, "frames": int(n.value)}

    def attach_rccl(self, unique_id: bytes) -> None:
        """Collective over the job (ncclCommInitRank): every rank passes the 128 bytes rank 0 got from rccl_unique_id()."""
        if len(unique_id) != 128:
            raise ValueError("an RCCL unique id is 128 bytes")
        buf = C.create_string_buffer(bytes(unique_id), 128)
        _check(load_library().rt_ring_attach_rccl(self._r, buf))

    def rccl_self_test(self) -> None:
        _check(load_library().rt_ring_rccl_self_test(self._r))


def rccl_available() -> bool:
    return bool(load_library().rt_rccl_available())


def rccl_unique_id() -> bytes:
    buf = C.create_string_buffer(128)
    _check(load_library().rt_rccl_unique_id(buf))
    return buf.raw


def resize_cpu(options: Options, tmp: np.ndarray) -> np.ndarray:
    """RayTracer::resize on the host (reference src/ray_tracer.cc:3-16)."""
    t = np.ascontiguousarray(tmp, dtype=np.float32)
    if t.size != options.total_width * options.total_height:
        raise RtError(RT_E_INVALID, "tmp must hold total_width*total_height floats")
    out = np.empty((options.height, options.width), dtype=np.uint8)
    _check(load_library().rt_resize_cpu(C.byref(options), t.ctypes.data, out.ctypes.data))
    return out


def partition_rows(options: Options, rank: int, nranks: int) -> np.ndarray:
    """Global output row of every local row of `rank` (rows >= height are padding)."""
    lib = load_library()
    count = lib.rt_partition_local_rows(C.byref(options), rank, nranks)
    return np.array([lib.rt_partition_global_row(C.byref(options), rank, nranks, j) for j in range(count)],
                    dtype=np.int64)


def pgm_bytes(image_u8: np.ndarray) -> bytes:
    """The file `render` writes: 'P5 W H 255\\n' + raw bytes (reference src/render.cc:135-136)."""
    h, w = image_u8.shape
    return f"P5 {w} {h} 255\n".encode() + np.ascontiguousarray(image_u8, dtype=np.uint8).tobytes()
