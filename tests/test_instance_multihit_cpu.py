"""CPU: the instanced multi-hit queries' contract (include/rt_hip_instance_multihit.h) -- the header, the exports and the
binding; the C oracle (tests/instance_multihit_oracle.c) against the BVH-free float64 reference
(tests/instance_multihit_reference.py) with 16 slots; the layered stack under two copies, whose lists overflow; the
comparator against doctored answers; and the header's relations, oracle against oracle.  No GPU.

What is asserted: on judged rays the counts, faces and instances are equal, the slots in the contract's order and the float
fields within instance_reference.TOL; at most 1 % of a case's rays go unjudged.  Every case prints its report (pytest -s)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import instance_cases as cases
import instance_multihit_oracle as imo
import instance_multihit_reference as imr
import instance_oracle as io
import multihit_oracle as mo
from conftest import ROOT

ENTRY_POINTS = ["rt_trace_instances_multihit", "rt_trace_instances_multihit_device"]
MESHES = ("blob", "ties")
BVHS = ("longest", "sah")
N_RAYS = 3000
K = imo.MAX_K
NONE = imo.NONE
_REF = {}


def plan_for(rt, arrays, transforms) -> dict:
    plan = rt.instance_plan(*cases.root_box(arrays), transforms)
    plan["world_from_object"] = transforms
    return plan


def max_distance_of(mesh, family) -> float:
    """tests/test_instances_cpu.py's rotation: one of {1e5, 5, 0.3} per case, every value taken by some family of every mesh."""
    return cases.MAX_DISTANCES[(cases.FAMILIES.index(family) + MESHES.index(mesh)) % 3]


def reference(key, scene, W, o, d, max_distance):
    """(the reference knows no tree: one answer for both builders)"""
    if key not in _REF:
        _REF[key] = imr.instanced(scene, W, o, d, max_distance)
        for v in _REF[key].values():
            v.setflags(write=False)
    return _REF[key]


def test_headers_exports_and_binding(rt):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt_hip_instance_multihit.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", text))) == ENTRY_POINTS
    fields = re.search(r"typedef struct rt_instance_multihit_arrays \{(.*?)\} rt_instance_multihit_arrays;", text, flags=re.S).group(1)
    assert re.findall(r"(\w+);", fields) == ["slots", "instance"]
    lib = C.CDLL(rt.lib_path())
    from opencl_raytracer_amd import api

    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in api._SIGNATURES, name
    for suffix in ("", "_device"):  # argument order follows rt_hip_multihit.h
        assert api._SIGNATURES["rt_trace_instances_multihit" + suffix] == api._SIGNATURES["rt_trace_multihit" + suffix]
    assert [f for f, _ in api._InstanceMultiHitArrays._fields_] == ["slots", "instance"]
    assert api._InstanceMultiHitArrays.instance.offset == C.sizeof(api._MultiHitArrays)
    assert api.INSTANCE_MULTIHIT_OUTPUTS == api.MULTIHIT_OUTPUTS + ("instance",) == rt.INSTANCE_MULTIHIT_OUTPUTS
    for method in ("trace_instances_multihit", "count_instances_hits"):
        assert callable(getattr(rt.Host, method, None)), method
    assert '#include "../oracle/rt_oracle.c"' in open(os.path.join(ROOT, "tests", "instance_multihit_oracle.c")).read()
    unit = open(os.path.join(ROOT, "opencl_raytracer_amd", "csrc", "kernels.hip")).read()
    assert '#include "kernels/instance_multihit.hip.h"' in unit
    # the sentence of rt_hip_instances.h that said this family has no instanced form names it now, and declares nothing new
    older = open(os.path.join(ROOT, "include", "rt_hip_instances.h")).read()
    assert "rt_hip_instance_multihit.h" in older and "have none" not in older
    assert "multihit" not in re.sub(r"/\*.*?\*/", "", older, flags=re.S)
    # null arguments are refused before any device is touched
    L = rt.load_library()
    assert L.rt_trace_instances_multihit(None, None, None, 0, 1e5, 4, 0, None) == -1
    assert L.rt_trace_instances_multihit_device(None, None, None, 0, 1e5, 4, 0, None, None) == -1


def test_binding_refuses_before_any_library_call(rt):
    bare = object.__new__(rt.Host)
    p = np.zeros((4, 3), np.float32)
    multi, count = rt.Host.trace_instances_multihit, rt.Host.count_instances_hits
    with pytest.raises(ValueError, match="unknown outputs"):
        multi(bare, p, p, outputs=("count", "hit"))
    with pytest.raises(ValueError, match="unknown outputs"):
        rt.Host.trace_multihit(bare, p, p, outputs=("instance",))  # (the plain form has no such array)
    with pytest.raises(ValueError, match="negative"):
        multi(bare, p, p, k=-1)
    for call in (multi, count):
        with pytest.raises(ValueError):
            call(bare, p.astype(np.float64), p)
        with pytest.raises(ValueError):
            call(bare, p, p[:3])
        with pytest.raises(ValueError):
            call(bare, np.zeros((4, 2), np.float32), p)
    with pytest.raises(AttributeError):  # (well-formed arguments get past the checks, to the handle this object does not have)
        multi(bare, p, p)


@pytest.mark.parametrize("family", cases.FAMILIES)
@pytest.mark.parametrize("bvh", BVHS)
@pytest.mark.parametrize("mesh", MESHES)
def test_oracle_against_the_reference(rt, scene_for, mesh, bvh, family):
    scene, arrays = scene_for(mesh, bvh)
    W = cases.family(family, arrays)
    plan = plan_for(rt, arrays, W)
    o, d = cases.rays(plan["nodes"], N_RAYS, seed=700 + cases.FAMILIES.index(family))
    max_distance = max_distance_of(mesh, family)
    ref = reference((mesh, family), scene, W, o, d, max_distance)
    got = imo.multihit(arrays, plan, o, d, max_distance, K)
    what = f"{mesh}/{bvh} {family} ({len(W)} instances) max_distance {max_distance}"
    rep = imr.compare_multihit(scene, ref, got, K)
    print(f"INSTANCE MULTIHIT {what}: {rep}; most members on a ray {int(got['count'].max())}")
    bad = rep.failures(tol=imr.TOL, max_unjudged=0.01)
    assert not bad, (what, bad)
    assert imo.in_contract_order(got).all() and imo.fill_values_hold(got).all(), what
    assert (ref["count"] > 0).mean() > 0.005, what  # (no case passes on misses alone; a max_distance of 0.3 leaves few)
    if mesh == "blob" and len(W) > 1:  # some ray whose slots hold two different instances
        two = (got["count"] >= 2) & (got["instance"][:, 0] != got["instance"][:, 1])
        assert two.any(), what
    if family == "tie_pair":  # every pair of equal distances lists instance 0 before 1
        used = got["leaf"] != NONE
        tie = used[:, :-1] & used[:, 1:] & (got["distance"][:, :-1] == got["distance"][:, 1:]) & (got["leaf"][:, :-1] == got["leaf"][:, 1:])
        assert tie.sum() > 100, what
        assert (got["instance"][:, :-1][tie] == 0).all() and (got["instance"][:, 1:][tie] == 1).all(), what
        assert (got["count"] % 2 == 0).all(), what


@pytest.mark.parametrize("family", ["tie_pair", "overlap_pair"])
@pytest.mark.parametrize("bvh", BVHS)
def test_layered_stack_overflows_the_lists(rt, bvh, family):
    """The families above reach at most a dozen members per ray: the layered stack of the plain multi-hit tests under two
    copies has rays with far more than RT_MULTIHIT_MAX_K, and ties of every kind."""
    scene, arrays = mo.layered_scene(rt, bvh)
    W = cases.family(family, arrays)
    plan = plan_for(rt, arrays, W)
    # (multihit_oracle.layered_rays' axis rays run along the world's z: through a rotated copy they cross a few layers at most
    # -- none of them more than 16 members under tie_pair -- so they are carried along by the first copy's transform)
    o, d, n_axis = imo.layered_rays(plan, arrays, W, n_axis=3000, n_oblique=1500)
    ref = reference(("layered", family), scene, W, o, d, 1e5)
    got = imo.multihit(arrays, plan, o, d, 1e5, K)
    over = float((got["count"][:n_axis] > K).mean())
    what = f"layered/{bvh} {family}"
    rep = imr.compare_multihit(scene, ref, got, K)
    print(f"INSTANCE MULTIHIT {what}: {rep}; {over:.2%} of the axis rays cross more than {K} members, most {int(got['count'].max())}")
    assert over >= 0.05, what
    bad = rep.failures(tol=imr.TOL, max_unjudged=0.01)
    assert not bad, (what, bad)
    assert imo.in_contract_order(got).all() and imo.fill_values_hold(got).all(), what
    two = (got["count"] >= 2) & (got["instance"][:, 0] != got["instance"][:, 1])
    assert two.any(), what
    # equal distances that only the instance, and only the leaf, order
    used = got["leaf"] != NONE
    same_d = used[:, :-1] & used[:, 1:] & (got["distance"][:, :-1] == got["distance"][:, 1:])
    assert (same_d & (got["instance"][:, :-1] != got["instance"][:, 1:])).any() or family == "overlap_pair", what
    assert (same_d & (got["instance"][:, :-1] == got["instance"][:, 1:])).any(), what


def test_comparator_reports_doctored_answers(rt, scene_for):
    scene, arrays = scene_for("blob", "longest")
    W = cases.family("overlap_pair", arrays)
    plan = plan_for(rt, arrays, W)
    o, d = cases.rays(plan["nodes"], N_RAYS, seed=700 + cases.FAMILIES.index("overlap_pair"))
    max_distance = max_distance_of("blob", "overlap_pair")
    ref = reference(("blob", "overlap_pair"), scene, W, o, d, max_distance)
    good = imo.multihit(arrays, plan, o, d, max_distance, K)
    assert not imr.compare_multihit(scene, ref, good, K).failures(tol=imr.TOL, max_unjudged=0.01)
    # a judged ray with two members at clearly different distances
    pick = np.flatnonzero(ref["judged"] & (good["count"] >= 2) & (good["distance"][:, 1] > 1.01 * good["distance"][:, 0] + 1e-3))
    assert len(pick) > 10
    i = int(pick[0])

    def doctored(change):
        bad = {f: v.copy() for f, v in good.items()}
        change(bad)
        return imr.compare_multihit(scene, ref, bad, K)

    def swap(a):
        for f in imo.SLOT_FIELDS:
            a[f][i, [0, 1]] = a[f][i, [1, 0]]

    rep = doctored(swap)
    assert rep["mismatches"]["order"] >= 1 and rep["mismatches"]["leaf"] + rep["mismatches"]["instance"] >= 1, rep

    def other_instance(a):
        a["instance"][i, 0] = 1 - a["instance"][i, 0]

    rep = doctored(other_instance)
    assert rep["mismatches"]["instance"] == 1 and rep.failures(tol=imr.TOL), rep

    def fewer(a):
        a["count"][i] -= 1

    rep = doctored(fewer)
    assert rep["mismatches"]["count"] == 1 and rep.failures(tol=imr.TOL), rep

    def filled(a):  # an unused slot that names an instance
        j = int(np.flatnonzero(ref["judged"] & (good["count"] < K))[0])
        a["instance"][j, K - 1] = 0

    assert doctored(filled)["mismatches"]["fill"] == 1


@pytest.mark.parametrize("family", ["rotations", "tie_pair", "overlap_pair", "grid"])
@pytest.mark.parametrize("bvh", BVHS)
def test_relations_to_the_closest_and_occluded_oracles(rt, scene_for, bvh, family):
    _, arrays = scene_for("blob", bvh)
    plan = plan_for(rt, arrays, cases.family(family, arrays))
    o, d = cases.rays(plan["nodes"], 1500, seed=31)
    oo, od = cases.odd_rays(plan["nodes"])
    o, d = np.concatenate([o, oo]), np.concatenate([d, od])
    for max_distance in cases.MAX_DISTANCES:
        full = imo.multihit(arrays, plan, o, d, max_distance, K)
        what = (bvh, family, max_distance)
        assert np.array_equal(full["count"] > 0, io.occluded(arrays, plan, o, d, max_distance).astype(bool)), what
        near = io.closest(arrays, plan, o, d, max_distance)
        at = near["distance"] < np.inf
        assert at.any() or max_distance < 1.0, what
        for f in imo.SLOT_FIELDS:
            assert imo.same_words(full[f][:, 0][at], near[f][at]).all(), (what, f)
        assert imo.in_contract_order(full).all() and imo.fill_values_hold(full).all(), what
        for k in (0, 1, 2, 3, 5, 8, 15):  # a call with k returns the first k slots of the call with 16
            imo.assert_same(imo.multihit(arrays, plan, o, d, max_distance, k), imo.first_slots(full, k), (what, k))


def test_identity_relation_on_the_oracles(rt, scene_for):
    """One identity instance, rays without -0: count and every slot are the plain multi-hit oracle's, word for word, with
    instance 0 in the used slots."""
    cases_run = [(mesh, bvh, scene_for(mesh, bvh)[1]) for mesh in MESHES for bvh in BVHS]
    cases_run += [("layered", bvh, mo.layered_scene(rt, bvh)[1]) for bvh in BVHS]
    for mesh, bvh, arrays in cases_run:
        W = cases.family("identity", arrays)
        assert np.array_equal(W[0], np.eye(3, 4, dtype=np.float32))
        plan = plan_for(rt, arrays, W)
        o, d = cases.rays(plan["nodes"], N_RAYS, seed=811)
        oo, od = cases.odd_rays(plan["nodes"])
        parts_o, parts_d = [o, oo], [d, od]
        if mesh == "layered":
            ao, ad = mo.axis_rays(1000, 3)
            parts_o.append(ao)
            parts_d.append(ad)
        o, d = cases.without_negative_zero(np.concatenate(parts_o), np.concatenate(parts_d))
        for max_distance in cases.MAX_DISTANCES:
            got = imo.multihit(arrays, plan, o, d, max_distance, K)
            want = mo.multihit(arrays, o, d, max_distance, K)
            assert want["count"].any() and (mesh != "layered" or max_distance < 1e5 or (want["count"] > K).any())
            for f in mo.FIELDS:
                assert imo.same_words(got[f], want[f]).all(), (mesh, bvh, max_distance, f)
            used = want["leaf"] != NONE
            assert (got["instance"][used] == 0).all() and (got["instance"][~used] == NONE).all()
