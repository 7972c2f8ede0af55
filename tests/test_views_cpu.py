"""CPU: multi-view rendering (include/rt_hip_views.h) without a GPU -- the header, the exports and the binding, and what
Host.render_views refuses before any library call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return text, sorted(set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", text)))


def test_header_exports_and_binding(rt):
    text, names = declared("rt_hip_views.h")
    assert names == ["rt_render_views", "rt_render_views_device"]
    _, debug = declared("rt_hip_debug.h")
    assert {"rt_debug_set_views_chunk", "rt_debug_last_views"} <= set(debug)
    lib = C.CDLL(rt.lib_path())
    from opencl_raytracer_amd import api

    for name in names + ["rt_debug_set_views_chunk", "rt_debug_last_views"]:
        assert hasattr(lib, name), name
        assert name in api._SIGNATURES, name
    fields = re.search(r"typedef struct rt_view_arrays \{(.*?)\} rt_view_arrays;", text, flags=re.S).group(1)
    assert re.findall(r"(\w+);", fields) == ["layers", "image"]
    assert api.VIEW_OUTPUTS == rt.VIEW_OUTPUTS == api.LAYER_OUTPUTS + ("image",)
    assert [f for f, _ in api._ViewArrays._fields_] == ["layers", "image"]
    assert C.sizeof(api._ViewArrays) == 11 * C.sizeof(C.c_void_p)
    assert api._ViewArrays.image.offset == C.sizeof(api._LayerArrays)
    assert C.sizeof(api.Camera) == 48  # rt_camera: the poses lie back to back
    # null arguments are refused before any device is touched
    L = rt.load_library()
    assert L.rt_render_views(None, None, 0, None) == -1 and L.rt_render_views_device(None, None, 0, None, None) == -1
    assert L.rt_debug_set_views_chunk(None, 2) == -1 and L.rt_debug_last_views(None, None, None, None) == -1
    # the seam itself did not grow
    seam, _ = declared("rt_hip.h")
    assert "views" not in seam


def test_render_views_refuses_before_any_library_call(rt):
    """Unknown outputs and wrongly shaped cameras raise ValueError on an object that has no handle and no options: nothing
    of the library can have been called."""
    bare = object.__new__(rt.Host)
    cam = rt.Camera.from_vectors((0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, -1))
    with pytest.raises(ValueError, match="unknown outputs"):
        rt.Host.render_views(bare, [cam], outputs=("depth",))
    with pytest.raises(ValueError, match="unknown outputs"):
        rt.Host.render_views(bare, [cam], outputs=("value", "images"))
    for bad in (np.zeros((2, 3, 4), np.float32), np.zeros((4, 3), np.float32), np.zeros((2, 4, 3), np.float64),
                np.zeros((2, 12), np.float32), [cam, "camera"], [np.zeros((4, 3), np.float32)]):
        with pytest.raises(ValueError, match="cameras"):
            rt.Host.render_views(bare, bad)
    # (well-formed arguments get past the checks, to the options this object does not have)
    with pytest.raises(AttributeError):
        rt.Host.render_views(bare, np.zeros((2, 4, 3), np.float32))
    with pytest.raises(AttributeError):
        rt.Host.render_views(bare, [cam, cam], outputs=rt.VIEW_OUTPUTS)
