"""CPU: the instanced directional occlusion queries (include/rt_hip_instance_directional.h) without a GPU -- the header, the
exports and the binding; the composed oracle (tests/instance_directional_oracle.py) against the BVH-free float64 reference
(tests/instance_reference.py on the written-out rays): bits on judged rays, `occluded` and `bent` on points all of whose rays
are judged, `bent` within shading_reference's tolerance (the directions are the plain query's and do not involve the set).
Every case prints its report (pytest -s)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import instance_cases as cases
import instance_directional_oracle as ido
import instance_views_oracle as ivo
import orc
import shading_reference as sr
from conftest import ROOT

ENTRY_POINTS = ["rt_trace_instances_ao_directional", "rt_trace_instances_ao_directional_device"]
N_POINTS = 400
RAYS_OF = {2: 14, 3: 28, 5: 71}  # ao_num_samples -> rays per point (UNIFORM)


def test_header_exports_and_binding(rt):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt_hip_instance_directional.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", text))) == ENTRY_POINTS
    assert '#include "rt_hip_directional.h"' in text and "rt_ao_directional_arrays" in text
    lib = C.CDLL(rt.lib_path())
    from opencl_raytracer_amd import api

    for name, model in zip(ENTRY_POINTS, ("rt_trace_ao_directional", "rt_trace_ao_directional_device")):
        assert hasattr(lib, name), name
        assert api._SIGNATURES[name] == api._SIGNATURES[model], name  # argument order follows rt_hip_directional.h
    assert callable(getattr(rt.Host, "instances_directional_occlusion", None))
    unit = open(os.path.join(ROOT, "opencl_raytracer_amd", "csrc", "kernels.hip")).read()
    assert '#include "kernels/instance_directional.hip.h"' in unit
    # the mask kernels share their ray and their tail
    plain = open(os.path.join(ROOT, "opencl_raytracer_amd", "csrc", "kernels", "directional.hip.h")).read()
    mine = open(os.path.join(ROOT, "opencl_raytracer_amd", "csrc", "kernels", "instance_directional.hip.h")).read()
    for shared in ("ao_mask_ray", "ao_mask_flags"):
        assert shared in plain and shared in mine, shared
    assert "atomicOr" not in mine and plain.count("atomicOr(") == 1
    older = open(os.path.join(ROOT, "include", "rt_hip_instances.h")).read()
    assert "rt_hip_instance_directional.h" in older and "directional" not in re.sub(r"/\*.*?\*/", "", older, flags=re.S)
    L = rt.load_library()
    assert L.rt_trace_instances_ao_directional(None, None, None, None, 0, 0, None) == -1
    assert L.rt_trace_instances_ao_directional_device(None, None, None, None, 0, 0, None, None) == -1


def test_binding_refuses_before_any_library_call(rt):
    bare = object.__new__(rt.Host)
    p = np.zeros((4, 3), np.float32)
    call = rt.Host.instances_directional_occlusion
    with pytest.raises(ValueError, match="unknown outputs"):
        call(bare, p, p, outputs=("mask", "instance"))
    with pytest.raises(ValueError):
        call(bare, p.astype(np.float64), p)
    with pytest.raises(ValueError):
        call(bare, p, p[:3])
    with pytest.raises(ValueError):
        call(bare, p, p, seeds=np.zeros(4, np.int64))
    with pytest.raises(ValueError):
        call(bare, p, p, seeds=np.zeros(3, np.uint32))


@pytest.mark.parametrize("samples", sorted(RAYS_OF))
@pytest.mark.parametrize("family", ["rotations", "overlap_pair", "tie_pair"])
def test_composition_against_the_float64_reference(rt, scene_for, family, samples):
    scene, arrays = scene_for("blob", "longest")
    opt = rt.Options.defaults(width=16, height=16, n_super_samples=1, ao_num_samples=samples, ao_max_distance=0.5)
    params = orc.params_from_options(opt)
    W = cases.family(family, arrays)
    plan = rt.instance_plan(*cases.root_box(arrays), W)
    points, normals = ido.lifted_points(arrays, plan, cases.rays(plan["nodes"], 3000, 7), N_POINTS)
    assert len(points) == N_POINTS
    origins, directions = ivo.ao_rays(params, arrays, points, normals)
    R = directions.shape[1]
    assert R == RAYS_OF[samples]
    got = ido.directional(params, arrays, plan, points, normals)
    ref = ido.reference(scene, W, origins, directions, params.ao_max_distance)
    rep = sr.compare_directional(ref, {f: got[f] for f in ido.OUTPUTS})
    blocked = float((got["occluded"] > 0).mean())
    unjudged_rays, unjudged_points = 1.0 - rep["judged_rays_share"], 1.0 - rep["judged_share"]
    print(f"INSTANCE DIRECTIONAL {family} R = {R}: {rep}; unjudged {unjudged_rays:.4%} of the rays, {unjudged_points:.2%} of the "
          f"points; {blocked:.1%} of the points have a blocked ray")
    assert not any(rep["mismatches"].values()), rep["mismatches"]
    assert rep["worst"]["bent"] <= sr.TOL["bent"], rep["worst"]
    assert unjudged_rays <= 0.001 and unjudged_points <= 0.02
    assert blocked >= 0.05
    # the composition's own consistency: padding bits 0, the popcount, the ordered sum on the flags
    assert np.array_equal(sr.unpack(got["mask"], 32 * got["mask"].shape[1])[:, :R], got["flags"])
    assert not sr.unpack(got["mask"], 32 * got["mask"].shape[1])[:, R:].any()
    assert np.array_equal(sr.popcount(got["mask"]), got["occluded"])
    # `occluded` and `ao` are the instanced ambient-occlusion composition's, word for word
    want = ivo.ao(params, arrays, plan, points, normals)
    assert np.array_equal(got["occluded"], want["occluded"]) and ivo.same_words(got["ao"], want["ao"]).all()


def test_comparator_reports_a_doctored_mask(rt, scene_for):
    scene, arrays = scene_for("blob", "longest")
    opt = rt.Options.defaults(width=16, height=16, n_super_samples=1, ao_num_samples=2, ao_max_distance=0.5)
    params = orc.params_from_options(opt)
    W = cases.family("overlap_pair", arrays)
    plan = rt.instance_plan(*cases.root_box(arrays), W)
    points, normals = ido.lifted_points(arrays, plan, cases.rays(plan["nodes"], 3000, 7), 100)
    origins, directions = ivo.ao_rays(params, arrays, points, normals)
    got = ido.directional(params, arrays, plan, points, normals)
    ref = ido.reference(scene, W, origins, directions, params.ao_max_distance)
    i, k = (int(x[0]) for x in np.nonzero(ref["judged"] & ref["point_judged"][:, None]))
    bad = {f: got[f].copy() for f in ido.OUTPUTS}
    bad["mask"][i, k >> 5] ^= np.uint32(1 << (k & 31))
    rep = sr.compare_directional(ref, bad)
    assert rep["mismatches"]["mask"] == 1 and rep["mismatches"]["occluded"] >= 1
