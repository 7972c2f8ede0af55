"""CPU: instanced ambient occlusion and instanced views (include/rt_hip_instance_views.h) without a GPU -- the header, the
exports and the binding; the composition helpers of tests/instance_views_oracle.py against the BVH-free float64 reference
(tests/instance_reference.py); the restated head-light term against the layers oracle's; the identity relation on the
oracles with the two caps of its -0 filter for the pose the GPU test uses; and what the Python methods refuse before any
library call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import instance_cases as cases
import instance_oracle as io
import instance_reference as ir
import instance_views_oracle as ivo
import layers_oracle as lo
import orc
from conftest import ROOT

ENTRY_POINTS = ["rt_render_instance_views", "rt_render_instance_views_device", "rt_trace_instances_ao", "rt_trace_instances_ao_device"]


def declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return text, sorted(set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", text)))


def test_header_exports_and_binding(rt):
    text, names = declared("rt_hip_instance_views.h")
    assert names == ENTRY_POINTS
    lib = C.CDLL(rt.lib_path())
    from opencl_raytracer_amd import api

    for name in names:
        assert hasattr(lib, name), name
        assert name in api._SIGNATURES, name
    fields = re.search(r"typedef struct rt_instance_view_arrays \{(.*?)\} rt_instance_view_arrays;", text, flags=re.S).group(1)
    assert re.findall(r"(\w+);", fields) == ["views", "instance"]
    assert [f for f, _ in api._InstanceViewArrays._fields_] == ["views", "instance"]
    assert api._InstanceViewArrays.instance.offset == C.sizeof(api._ViewArrays) and C.sizeof(api._InstanceViewArrays) == 12 * C.sizeof(C.c_void_p)
    assert rt.INSTANCE_VIEW_OUTPUTS == rt.VIEW_OUTPUTS + ("instance",)
    for method in ("instances_ambient_occlusion", "render_instance_views"):
        assert hasattr(rt.Host, method), method
    # null arguments are refused before any device is touched
    L = rt.load_library()
    assert L.rt_render_instance_views(None, None, 0, None) == -1 and L.rt_render_instance_views_device(None, None, 0, None, None) == -1
    assert L.rt_trace_instances_ao(None, None, None, None, 0, 0, None, None) == -1
    assert L.rt_trace_instances_ao_device(None, None, None, None, 0, 0, None, None, None) == -1
    # the sentence of rt_hip_instances.h that lists what ignores the set names the instanced forms now
    parent = open(os.path.join(ROOT, "include", "rt_hip_instances.h")).read()
    assert "rt_hip_instance_views.h" in parent
    # the kernels are part of the one translation unit
    unit = open(os.path.join(ROOT, "opencl_raytracer_amd", "csrc", "kernels.hip")).read()
    assert '#include "kernels/instance_views.hip.h"' in unit


def test_python_methods_refuse_before_any_library_call(rt):
    bare = object.__new__(rt.Host)
    cam = rt.Camera.from_vectors((0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, -1))
    p = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError, match="unknown outputs"):
        rt.Host.render_instance_views(bare, [cam], outputs=("instance", "depth"))
    with pytest.raises(ValueError, match="unknown outputs"):
        rt.Host.render_views(bare, [cam], outputs=("instance",))  # (the plain form has no such layer)
    for bad in (np.zeros((2, 3, 4), np.float32), np.zeros((2, 4, 3), np.float64), [cam, "camera"]):
        with pytest.raises(ValueError, match="cameras"):
            rt.Host.render_instance_views(bare, bad, outputs=("instance",))
    with pytest.raises(AttributeError):  # (well-formed arguments get past the checks, to the options this object does not have)
        rt.Host.render_instance_views(bare, [cam], outputs=rt.INSTANCE_VIEW_OUTPUTS)
    ao = rt.Host.instances_ambient_occlusion
    with pytest.raises(ValueError, match="unknown outputs"):
        ao(bare, p, p, outputs=("ao", "mask"))
    with pytest.raises(ValueError):
        ao(bare, p.astype(np.float64), p)
    with pytest.raises(ValueError):
        ao(bare, p, p[:3])
    with pytest.raises(ValueError):
        ao(bare, p, p, seeds=np.zeros(4, np.int64))
    with pytest.raises(ValueError):
        ao(bare, p, p, seeds=np.zeros(3, np.uint32))
    with pytest.raises(ValueError):
        ao(bare, np.zeros((4, 2), np.float32), p)


@pytest.mark.parametrize("shading", [1, 0])
def test_restated_shade_is_the_layers_oracles(rt, scene_for, shading):
    """On a plain scene the head-light term restated in numpy == the layers oracle's `shade`, word for word; and one identity
    instance gives the composition that very layer where the relation holds."""
    _, arrays = scene_for("blob", "sah")
    opt = rt.Options.defaults(width=24, height=20, n_super_samples=2, ao_num_samples=2, enable_shading=shading)
    params = orc.params_from_options(opt)
    pose = ivo.oblique_pose(rt, arrays)
    plain = lo.render(params, arrays, pose)
    assert plain["hit"].any() and not plain["hit"].all()
    mine = ivo.shade(plain["normal"], plain["direction"], plain["hit"], bool(shading))
    assert ivo.same_words(mine, plain["shade"]).all()
    if shading:
        lit = plain["shade"][plain["hit"].astype(bool)]
        assert (lit > 0).any() and (lit < 1).any()
    else:
        assert (plain["shade"][plain["hit"].astype(bool)] == 1).all()
    # NaN loses: fmaxf(NaN, 0) = 0
    assert ivo.shade(np.full((1, 3), np.nan, np.float32), np.ones((1, 3), np.float32), [1], True)[0] == 0.0


@pytest.mark.parametrize("mesh", ["blob", "bunny"])
def test_identity_relation_and_its_caps_on_the_oracles(rt, scene_for, mesh):
    params, arrays, plan, pose, plain = ivo.identity_case(rt, scene_for, mesh)
    record, ao, hit = ivo.identity_masks(params, arrays, pose, plain)
    left_out, ao_left_out = 1.0 - record.mean(), 1.0 - ao[hit].mean()
    print(f"IDENTITY {mesh}: {hit.sum()} of {len(hit)} sub-pixels hit; the -0 filter leaves out {left_out:.4f} of the sub-pixels, "
          f"{ao_left_out:.4f} of the hit ones for ao")
    assert hit.sum() > 100 and not hit.all()
    assert left_out <= ivo.RECORD_CAP and ao_left_out <= ivo.AO_CAP
    got = ivo.view(params, arrays, plan, pose)
    at = record & (plain["distance"].reshape(-1) < np.inf)
    for f in lo.RECORD + ("direction", "shade"):
        a, b = got[f].reshape(len(hit), -1)[at], plain[f].reshape(len(hit), -1)[at]
        assert ivo.same_words(a, b).all(), (mesh, f)
    assert (got["instance"].reshape(-1)[at & hit] == 0).all() and (got["instance"].reshape(-1)[~hit] == 0xFFFFFFFF).all()
    with_ao = ao & (plain["distance"].reshape(-1) < np.inf)
    for f in ("ao", "value"):
        assert ivo.same_words(got[f].reshape(-1)[with_ao], plain[f].reshape(-1)[with_ao]).all(), (mesh, f)
    assert (got["ao"].reshape(-1)[with_ao] < 1).any()


@pytest.mark.parametrize("family", ["rotations", "shear", "mirror"])
def test_composition_against_the_float64_reference(rt, scene_for, family):
    """One view's rays and the ambient-occlusion rays of its hit sub-pixels: the composition's records and flags against the
    reference that knows no tree, with that module's own tolerances."""
    scene, arrays = scene_for("blob", "longest")
    opt = rt.Options.defaults(width=48, height=40, n_super_samples=1, ao_num_samples=2, ao_max_distance=0.5)
    params = orc.params_from_options(opt)
    W = cases.family(family, arrays)
    plan = rt.instance_plan(*cases.root_box(arrays), W)
    pose = ivo.cameras(rt, plan)[0]
    o, d = ivo.camera_rays(params, arrays, pose)
    got = ivo.view(params, arrays, plan, pose)
    flat = {f: got[f].reshape((len(o),) + got[f].shape[2:]) for f in ivo.RECORD}
    hit = flat["hit"].astype(bool)
    assert hit.sum() > 20 and not hit.all() and (family == "mirror" or len(np.unique(flat["instance"][hit])) > 1)
    ref = ir.instanced(scene, W, o, d, 1e5)
    rep = ir.compare_closest(scene, ref, flat)
    print(f"INSTANCE VIEWS {family}: {rep}")
    assert not rep.failures(tol=ir.TOL, max_unjudged=0.01), rep.failures(tol=ir.TOL, max_unjudged=0.01)
    seeds = np.flatnonzero(hit).astype(np.uint32)
    ao_o, ao_d = ivo.ao_rays(params, arrays, flat["position"][hit], flat["normal"][hit], seeds)
    per = ao_d.shape[1]
    ro, rd = np.repeat(ao_o, per, axis=0), ao_d.reshape(-1, 3)
    flags = io.occluded(arrays, plan, ro, rd, params.ao_max_distance)
    rep = ir.compare_occluded(ir.instanced(scene, W, ro, rd, params.ao_max_distance), flags)
    print(f"INSTANCE AO {family}: {rep}")
    # (these rays start 1e-5 off a surface, inside the band in which the reference judges nothing: most go unjudged; no
    # judged one may differ)
    assert rep["judged_share"] > 0 and not rep.failures(tol=ir.TOL, max_unjudged=1.0), rep.failures(tol=ir.TOL, max_unjudged=1.0)
    want = ivo.ao(params, arrays, plan, flat["position"][hit], flat["normal"][hit], seeds)
    assert np.array_equal(want["occluded"], flags.reshape(-1, per).sum(axis=1)) and want["occluded"].any()
    assert ivo.same_words(got["ao"].reshape(-1)[hit], want["ao"]).all() and (got["ao"].reshape(-1)[~hit] == 1).all()
    with np.errstate(all="ignore"):
        assert ivo.same_words(got["value"], (got["shade"] * got["ao"]).astype(np.float32)).all()
