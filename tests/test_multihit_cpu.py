"""CPU: the multi-hit queries' oracle (tests/multihit_oracle.c) checked against the closest-hit oracle and its own contract,
the inputs of the GPU tests checked for what they must provoke, and the library's exported entry points."""
import os
import subprocess

import numpy as np
import pytest

import multihit_oracle as mo
import orc
import query_oracle as qo

MULTIHIT_SYMBOLS = ("rt_trace_multihit", "rt_trace_multihit_device")
CLOSEST_FIELDS = ("distance", "leaf", "barycentric", "position", "normal")


def test_multihit_header_declares_the_entry_points():
    path = os.path.join(os.path.dirname(__file__), "..", "include", "rt_hip_multihit.h")
    assert os.path.exists(path)
    header = open(path).read()
    for s in MULTIHIT_SYMBOLS:
        assert s + "(" in header, s
    assert "RT_MULTIHIT_MAX_K 16u" in header


def test_library_exports_the_multihit_entry_points(rt):
    out = subprocess.run(["nm", "-D", "--defined-only", rt.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    missing = [s for s in MULTIHIT_SYMBOLS if s not in exported]
    assert not missing, missing


def test_binding_knows_the_multihit_entry_points(rt):
    for s in MULTIHIT_SYMBOLS:
        assert s in rt.api._SIGNATURES, s
    assert callable(getattr(rt.Host, "trace_multihit", None))
    assert callable(getattr(rt.Host, "count_hits", None))


@pytest.mark.parametrize("bvh", ["longest", "sah"])
@pytest.mark.parametrize("mesh", ["blob", "ties"])
def test_oracle_agrees_with_the_closest_hit_oracle(rt, scene_for, mesh, bvh):
    _, arrays = scene_for(mesh, bvh)
    opt = rt.Options.defaults(width=64, height=48, n_super_samples=1, enable_ao=0)
    o4, d4 = qo.camera_rays(orc.params_from_options(opt))
    for md in (100000.0, 2.5):  # (2.5 from the camera at z = 2: the limit culls some of the boxes)
        multi = mo.multihit(arrays, o4, d4, md, 5)
        near = qo.closest(arrays, o4, d4, md)
        assert md < 100.0 or (multi["count"] > 1).any()
        # slot 0 is the closest hit, word for word, wherever that hit has a distance below +inf
        kept = near["hit"].astype(bool) & (near["distance"] < np.inf)
        for f in CLOSEST_FIELDS:
            same = mo.same_words(multi[f][:, 0], near[f])
            assert same[kept].all(), (f, int((~same[kept]).sum()))
        # count > 0 is the occlusion answer
        assert np.array_equal(multi["count"] > 0, qo.occluded(arrays, o4, d4, md).astype(bool))
        assert mo.in_contract_order(multi).all()
        assert mo.fill_values_hold(multi).all()
        # fewer slots: the same count, the first slots of the longer answer
        short = mo.multihit(arrays, o4, d4, md, 2)
        for f in mo.FIELDS:
            assert mo.same_words(short[f], mo.first_slots(multi, 2)[f]).all(), f


@pytest.mark.parametrize("bvh", ["longest", "sah"])
def test_layered_scene_overflows_lists_and_ties_distances(rt, bvh):
    """Non-vacuity of the GPU test's inputs: lists longer than RT_MULTIHIT_MAX_K, and equal distances that only the leaf
    index orders."""
    _, arrays = mo.layered_scene(rt, bvh)
    o, d, n_axis = mo.layered_rays(arrays)
    assert len(o) == 20000
    res = mo.multihit(arrays, o, d, 100000.0, mo.MAX_K)
    assert (res["count"][:n_axis] > mo.MAX_K).sum() >= n_axis // 4
    used = res["leaf"] != mo.NONE
    tie = used[:, :-1] & used[:, 1:] & (res["distance"][:, :-1] == res["distance"][:, 1:]) & \
        (res["leaf"][:, :-1] != res["leaf"][:, 1:])
    assert tie.any(axis=1).sum() >= 100
    assert mo.in_contract_order(res).all()
    assert mo.fill_values_hold(res).all()
    assert (res["count"][n_axis:] > 0).any()  # the oblique rays meet the stack too
