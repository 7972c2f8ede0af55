"""The exported query entry points are forwarders to one body per family (csrc/c_api.cc, <family>_call): every variant of a
family -- host or device memory, closest or occluded, plain or instanced -- must refuse a null host with the same code and
the same text, before it looks at anything else.  Needs no device: nothing gets as far as one."""
import ctypes as C

import pytest

import opencl_raytracer_amd as rt

# family -> the entry points folded onto its body
FAMILIES = {
    "rays": ("rt_trace_closest", "rt_trace_occluded", "rt_trace_closest_device", "rt_trace_occluded_device", "rt_trace_instances_closest",
             "rt_trace_instances_occluded", "rt_trace_instances_closest_device", "rt_trace_instances_occluded_device"),
    "segments": ("rt_segments_closest", "rt_segments_occluded", "rt_segments_closest_device", "rt_segments_occluded_device",
                 "rt_instances_segments_closest", "rt_instances_segments_occluded", "rt_instances_segments_closest_device",
                 "rt_instances_segments_occluded_device"),
    "visibility": ("rt_visibility_masks", "rt_visibility_masks_device", "rt_instances_visibility_masks",
                   "rt_instances_visibility_masks_device"),
    "points": ("rt_closest_points", "rt_closest_points_device", "rt_instances_closest_points", "rt_instances_closest_points_device"),
    "signed": ("rt_signed_distance", "rt_signed_distance_device"),
    "multihit": ("rt_trace_multihit", "rt_trace_multihit_device", "rt_trace_instances_multihit", "rt_trace_instances_multihit_device"),
    "ao": ("rt_trace_ao", "rt_trace_ao_device", "rt_trace_instances_ao", "rt_trace_instances_ao_device"),
    "directional": ("rt_trace_ao_directional", "rt_trace_ao_directional_device", "rt_trace_instances_ao_directional",
                    "rt_trace_instances_ao_directional_device"),
    "ao_rays": ("rt_ao_rays", "rt_ao_rays_device"),
    "layers": ("rt_render_layers", "rt_render_layers_device"),
}
# What the library answered before the entry points were folded: (return code, rt_last_error_code(), rt_last_error()).
NULL_HOST = (-1, -1, b"null host")  # (the host is checked before a family's name is put into any message)
RECORDED = {"rays": NULL_HOST, "segments": NULL_HOST, "visibility": NULL_HOST, "points": NULL_HOST, "signed": NULL_HOST,
            "multihit": NULL_HOST, "ao": NULL_HOST, "directional": NULL_HOST, "ao_rays": NULL_HOST, "layers": NULL_HOST}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_every_variant_refuses_a_null_host_alike(family):
    lib = rt.load_library()
    for name in FAMILIES[family]:
        _, argtypes = rt.api._SIGNATURES[name]
        assert all(a in (C.c_void_p, C.c_uint32, C.c_float) for a in argtypes), name
        rc = getattr(lib, name)(*[None if a is C.c_void_p else 0 for a in argtypes])
        assert (rc, lib.rt_last_error_code(), lib.rt_last_error()) == RECORDED[family], name


def test_the_table_names_every_folded_entry_point():
    """Every *_device query entry point of the binding has its blocking twin in the same family, and the other way round."""
    for family, names in FAMILIES.items():
        plain = {n for n in names if not n.endswith("_device")}
        assert {n + "_device" for n in plain} == set(names) - plain, family
        assert all(n in rt.api._SIGNATURES for n in names), family
