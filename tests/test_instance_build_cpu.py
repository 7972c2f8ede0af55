"""CPU: device-side instance sets (include/rt_hip_instance_build.h) as the host restates them -- rt_instance_plan_lbvh
against an independent top-down numpy restatement of the tree (tests/instance_build_cases.py), against the host planner's
numbers (rt_instance_plan: the same inverses, the same six floats per leaf box), the tree's shape, ties, a root box that is
not finite, the refusals, the C oracle on both trees with the float64 judge over it, and the restatement under the address
and undefined-behaviour sanitizers in a stand-alone program (which also holds the bounds against ocrt::instance_bounds).
No GPU."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import instance_build_cases as bc
import instance_cases as cases
import instance_oracle as io
import instance_reference as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("rt_build_instances_device", "rt_build_instances", "rt_instances_world_from_object", "rt_instance_bounds",
                "rt_last_instance_build_ms", "rt_instance_plan_lbvh")
NONE = 0xFFFFFFFF
MESHES = ("single", "ties", "blob")
MAX_UNJUDGED = 0.0007  # (at most 0.07 % of a case's rays)
# The rays of a case: the 3000 of tests/test_instances_cpu.py (the same generator and seeds), and MORE_RAYS further ones.
# The bound above is a RATE.  At 3000 rays one ray is 0.033 % and the bound is 2.1 rays: a case whose rate lies well below
# the bound shows three unjudged rays by chance every few cases.  The sample has to resolve the bound: one ray a tenth of it
# or less, n >= 10 / 0.0007 = 14 286 -- hence 15 000 rays a case.
N_RAYS, MORE_RAYS = 3000, 12000


def check_tree(nodes, n):
    """A full binary tree in pre-order with tiling skips, every instance exactly once, inner boxes the children's min / max."""
    assert len(nodes) == 2 * n - 1
    skip, leaf = nodes["skip"].astype(np.int64), nodes["leaf"]
    seen = []
    stack = [(0, len(nodes))]
    while stack:
        at, size = stack.pop()
        assert skip[at] == size, (at, skip[at], size)
        if size == 1:
            assert leaf[at] != NONE
            seen.append(int(leaf[at]))
            continue
        assert leaf[at] == NONE and size % 2 == 1
        first = at + 1
        second = first + skip[first]
        assert second < at + size and skip[first] + skip[second] + 1 == size
        lo, hi = np.minimum(nodes["lo"][first], nodes["lo"][second]), np.maximum(nodes["hi"][first], nodes["hi"][second])
        assert np.array_equal(nodes["lo"][at], lo) and np.array_equal(nodes["hi"][at], hi)
        stack += [(first, int(skip[first])), (second, int(skip[second]))]
    assert sorted(seen) == list(range(n))


def test_header_library_and_binding(rt):
    header = os.path.join(ROOT, "include", "rt_hip_instance_build.h")
    assert os.path.exists(header), "include/rt_hip_instance_build.h is missing"
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(ENTRY_POINTS)
    lib = C.CDLL(rt.lib_path())
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in rt.api._SIGNATURES, name
    for method in ("build_instances", "instances", "instance_bounds", "last_instance_build_ms"):
        assert hasattr(rt.Host, method), method
    assert callable(rt.instance_plan_lbvh)
    assert "rt_hip_instance_build.h" in open(os.path.join(ROOT, "include", "rt_hip_instances.h")).read()
    assert "rt_hip_instance_build.h" in open(os.path.join(ROOT, "README.md")).read()
    csrc = os.path.join(ROOT, "opencl_raytracer_amd", "csrc")
    # one text for the arithmetic, free of the device runtime, taken by the planner, the restatement and the kernels
    shared = open(os.path.join(csrc, "instance_plan.h")).read()
    assert "hip_runtime" not in shared and "hip/" not in shared
    for name in ("instance_inverse", "instance_reach", "instance_margin", "instance_box", "eigen_bounds", "instance_bound", "outward_down",
                 "outward_up", "rounded_down"):
        assert re.search(r"\b" + name + r"\(", shared), name
        assert not re.search(r"^(?:static |inline )?(?:bool|double|float|void) " + name + r"\(", open(os.path.join(csrc, "instances.cc")).read(), re.M), name
    assert '#include "instance_plan.h"' in open(os.path.join(csrc, "kernels.hip")).read()
    restatement = open(os.path.join(csrc, "instance_build.cc")).read()
    assert "hip_runtime" not in restatement and "rt_instance_plan_lbvh" in restatement


@pytest.fixture(scope="module")
def plans(rt, scene_for):
    """(mesh, set name) -> (W, the library's restatement, the host planner's plan): made once, read-only."""
    made = {}
    for mesh in MESHES:
        _, arrays = scene_for(mesh, "longest")
        lo, hi = cases.root_box(arrays)
        for name, W in bc.sets(arrays).items():
            made[(mesh, name)] = (W, rt.instance_plan_lbvh(lo, hi, W), rt.instance_plan(lo, hi, W))
    return made


@pytest.mark.parametrize("mesh", MESHES)
def test_plan_equals_the_numpy_restatement(rt, scene_for, plans, mesh):
    _, arrays = scene_for(mesh, "longest")
    lo, hi = cases.root_box(arrays)
    names = [name for m, name in plans if m == mesh]
    assert {f"many{n}" for n in bc.COUNTS} <= set(names) and set(cases.FAMILIES + cases.HARD_FAMILIES) <= set(names)
    for name in names:
        W, got, _ = plans[(mesh, name)]
        want = bc.restated_plan(rt, lo, hi, W)
        assert got["nodes"].tobytes() == want["nodes"].tobytes(), (mesh, name)
        assert got["object_from_world"].tobytes() == want["object_from_world"].tobytes(), (mesh, name)


@pytest.mark.parametrize("mesh", MESHES)
def test_same_numbers_as_the_host_planner_and_a_tree(plans, mesh):
    for (m, name), (W, got, host) in plans.items():
        if m != mesh:
            continue
        n = len(W)
        assert got["object_from_world"].tobytes() == host["object_from_world"].tobytes(), name
        mine, theirs = bc.leaf_boxes_of(got["nodes"], n), bc.leaf_boxes_of(host["nodes"], n)
        assert mine[0].tobytes() == theirs[0].tobytes() and mine[1].tobytes() == theirs[1].tobytes(), name
        check_tree(got["nodes"], n)
        assert got["nodes"]["lo"][0].tobytes() == host["nodes"]["lo"][0].tobytes(), name  # (the root: the same union)
        assert got["nodes"]["hi"][0].tobytes() == host["nodes"]["hi"][0].tobytes(), name
        assert got["bounds"].shape == (n, 4) and np.isfinite(got["bounds"]).all() and (got["bounds"] >= 0).all(), name


def test_equal_keys_come_out_in_rising_index(rt, scene_for):
    _, arrays = scene_for("blob", "longest")
    lo, hi = cases.root_box(arrays)
    for n in (2, 70, 257):
        nodes = rt.instance_plan_lbvh(lo, hi, bc.identical(arrays, n))["nodes"]
        check_tree(nodes, n)
        assert np.array_equal(nodes["leaf"][nodes["leaf"] != NONE], np.arange(n))
        assert len(np.unique(bc.keys_of(*bc.leaf_boxes_of(nodes, n)))) == 1


def test_a_root_box_that_is_not_finite(rt, scene_for):
    _, arrays = scene_for("blob", "longest")
    lo, hi = cases.root_box(arrays)
    W = cases.many(arrays, 65)
    for bad in (np.nan, np.inf, -np.inf):
        broken = hi.copy()
        broken[1] = bad
        plan = rt.instance_plan_lbvh(lo, broken, W)
        nodes = plan["nodes"]
        check_tree(nodes, 65)
        assert np.isneginf(nodes["lo"]).all() and np.isposinf(nodes["hi"]).all()
        assert np.array_equal(nodes["leaf"][nodes["leaf"] != NONE], np.arange(65))  # (all keys 0: the order is by index)
        assert (plan["bounds"][:, 0] == 0).all()  # (nothing is passed by)
        assert plan["object_from_world"].tobytes() == rt.instance_plan(lo, hi, W)["object_from_world"].tobytes()
        assert nodes.tobytes() == bc.restated_plan(rt, lo, broken, W)["nodes"].tobytes()


def test_refusals_write_nothing(rt, scene_for):
    _, arrays = scene_for("blob", "longest")
    lo, hi = cases.root_box(arrays)
    lib = rt.load_library()
    INVALID = rt.api.RT_E_INVALID
    for n in (1, 3, 257):
        good = cases.many(arrays, n)
        plan = rt.instance_plan_lbvh(lo, hi, good)
        for name, bad in bc.bad_transforms(arrays).items():
            for at in sorted({0, n // 2, n - 1}):
                W = good.copy()
                W[at] = bad
                O, nodes, bounds = plan["object_from_world"].copy(), plan["nodes"].copy(), plan["bounds"].copy()
                rc = lib.rt_instance_plan_lbvh(lo.ctypes.data, hi.ctypes.data, W.ctypes.data, n, O.ctypes.data, nodes.ctypes.data, bounds.ctypes.data)
                assert rc == INVALID, (name, n, at)
                assert O.tobytes() == plan["object_from_world"].tobytes() and nodes.tobytes() == plan["nodes"].tobytes(), (name, n, at)
                assert bounds.tobytes() == plan["bounds"].tobytes(), (name, n, at)
                with pytest.raises(rt.RtError) as e:
                    rt.instance_plan_lbvh(lo, hi, W)
                assert e.value.code == INVALID
    good = cases.many(arrays, 3)
    assert lib.rt_instance_plan_lbvh(lo.ctypes.data, hi.ctypes.data, good.ctypes.data, 0, None, None, None) == INVALID
    assert lib.rt_instance_plan_lbvh(lo.ctypes.data, hi.ctypes.data, good.ctypes.data, (1 << 20) + 1, None, None, None) == INVALID
    assert lib.rt_instance_plan_lbvh(None, hi.ctypes.data, good.ctypes.data, 3, None, None, None) == INVALID
    assert lib.rt_instance_plan_lbvh(lo.ctypes.data, hi.ctypes.data, good.ctypes.data, 3, None, None, None) == 0
    with pytest.raises(ValueError):
        rt.instance_plan_lbvh(lo, hi, good.astype(np.float64))


@pytest.mark.parametrize("family", cases.FAMILIES)
@pytest.mark.parametrize("mesh", ("blob", "ties"))
def test_oracle_on_both_plans(rt, scene_for, mesh, family):
    """The C oracle walks both trees over the same leaf boxes: boxes along a path are unions and the slab test is monotone in
    its bounds, so a ray with finite components enters the same copies in either tree and the records are equal word for
    word; the float64 judge, which knows no tree, then passes the LBVH plan's answer.

    Measured: no mismatch among judged rays in any of the 18 cases, and every record equal word for word between the two
    plans.  Unjudged rays of 15 000: none in four cases, at most 8 (0.053 %) in thirteen, 10 (0.067 %) in `ties mirror`; `blob
    identity` 6 (0.040 %).  Which rays go unjudged is the judge's own borderline rule and involves no tree.  On the first 3000
    rays alone the counts are 0 in nine cases, 1 in seven, 2 in `ties mirror` and 3 (0.10 %) in `blob identity` -- the same
    three rays go unjudged on the median-split plan in tests/test_instances_cpu.py --: a sample that cannot resolve the
    bound (N_RAYS above says why the case has more rays)."""
    scene, arrays = scene_for(mesh, "longest")
    lo, hi = cases.root_box(arrays)
    W = cases.family(family, arrays)
    median, lbvh = rt.instance_plan(lo, hi, W), rt.instance_plan_lbvh(lo, hi, W)
    for plan in (median, lbvh):
        plan["world_from_object"] = W
    o, d = cases.rays(median["nodes"], N_RAYS, seed=700 + cases.FAMILIES.index(family))
    more_o, more_d = cases.rays(median["nodes"], MORE_RAYS, seed=1700 + cases.FAMILIES.index(family))
    o, d = np.concatenate([o, more_o]), np.concatenate([d, more_d])
    assert np.isfinite(o).all() and np.isfinite(d).all()
    max_distance = cases.MAX_DISTANCES[(cases.FAMILIES.index(family) + ("blob", "ties").index(mesh)) % 3]
    what = f"{mesh} {family} ({len(W)} instances) max_distance {max_distance}"
    got, other = io.closest(arrays, lbvh, o, d, max_distance), io.closest(arrays, median, o, d, max_distance)
    for f in ("hit", "distance", "leaf", "instance", "barycentric", "position", "normal"):
        assert io.same_words(got[f], other[f]).all(), (what, f)
    occ = io.occluded(arrays, lbvh, o, d, max_distance)
    assert np.array_equal(occ, io.occluded(arrays, median, o, d, max_distance)) and np.array_equal(occ, got["hit"]), what
    ref = ir.instanced(scene, W, o, d, max_distance)
    for rep in (ir.compare_occluded(ref, occ), ir.compare_closest(scene, ref, got)):
        print(f"INSTANCE BUILD {what}: {rep}")
        bad = rep.failures(tol=ir.TOL, max_unjudged=MAX_UNJUDGED)
        assert not bad, (what, bad)


def test_restatement_under_the_sanitizers():
    """tests/instance_build_sanitize.cc with csrc/instance_build.cc and csrc/instances.cc, -fsanitize=address,undefined, as a
    child process: nothing is loaded into this interpreter."""
    out = os.path.join(tempfile.mkdtemp(prefix="ocrt_instance_build_sanitize_"), "instance_build_sanitize")
    csrc = os.path.join(ROOT, "opencl_raytracer_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", out, os.path.join(ROOT, "tests", "instance_build_sanitize.cc"),
                    os.path.join(csrc, "instance_build.cc"), os.path.join(csrc, "instances.cc")], check=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "INSTANCE_BUILD_SANITIZE_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
