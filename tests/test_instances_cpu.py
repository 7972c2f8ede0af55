"""CPU: the instanced ray queries' contract (include/rt_hip_instances.h) -- the host-only planner (rt_instance_plan: the
inverses by the header's formula, the top-level tree, its boxes), the C oracle (tests/instance_oracle.c) against the BVH-free
float64 reference (tests/instance_reference.py), the identity relation to the ray queries' oracle, and the planner under
the address and undefined-behaviour sanitizers in a stand-alone program.  No GPU.

What is asserted: on judged rays the flags, faces and instances are equal and the float fields lie within
instance_reference.TOL; at most 1 % of a case's rays go unjudged.  Every case prints its report (pytest -s)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import instance_cases as cases
import instance_oracle as io
import instance_reference as ir
import query_oracle as qo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("rt_set_instances", "rt_instance_count", "rt_instances_object_from_world",
                "rt_instance_node_count", "rt_instance_nodes", "rt_trace_instances_closest", "rt_trace_instances_occluded",
                "rt_trace_instances_closest_device", "rt_trace_instances_occluded_device", "rt_instance_plan")
MESHES = ("blob", "ties")
BVHS = ("longest", "sah")
N_RAYS = 3000
NONE = 0xFFFFFFFF
_REF = {}


def plan_for(rt, arrays, transforms) -> dict:
    lo, hi = cases.root_box(arrays)
    plan = rt.instance_plan(lo, hi, transforms)
    plan["world_from_object"] = transforms
    return plan


def max_distance_of(mesh, family) -> float:
    """One of {1e5, 5, 0.3} per case, every value taken by some family of every mesh."""
    return cases.MAX_DISTANCES[(cases.FAMILIES.index(family) + MESHES.index(mesh)) % 3]


def restated_inverse(W32) -> np.ndarray:
    """The header's formula in numpy float64, operation by operation, rounded once to float32."""
    W = W32.astype(np.float64)
    a, b, c, x = W[:, 0, 0], W[:, 0, 1], W[:, 0, 2], W[:, 0, 3]
    d, e, f, y = W[:, 1, 0], W[:, 1, 1], W[:, 1, 2], W[:, 1, 3]
    g, h, i, z = W[:, 2, 0], W[:, 2, 1], W[:, 2, 2], W[:, 2, 3]
    adj = [[e * i - f * h, c * h - b * i, b * f - c * e], [f * g - d * i, a * i - c * g, c * d - a * f],
           [d * h - e * g, b * g - a * h, a * e - b * d]]
    det = (a * adj[0][0] + b * adj[1][0]) + c * adj[2][0]
    out = np.zeros(W.shape, np.float32)
    for r in range(3):
        q = [adj[r][k] / det for k in range(3)]
        out[:, r, 0], out[:, r, 1], out[:, r, 2] = q[0], q[1], q[2]
        out[:, r, 3] = -((q[0] * x + q[1] * y) + q[2] * z)
    return out


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
        assert np.array_equal(nodes["lo"][at].view(np.uint32), lo.view(np.uint32)) and np.array_equal(nodes["hi"][at].view(np.uint32), hi.view(np.uint32))
        stack += [(first, int(skip[first])), (second, int(skip[second]))]
    assert sorted(seen) == list(range(n))


def test_header_library_and_binding(rt):
    header = os.path.join(ROOT, "include", "rt_hip_instances.h")
    assert os.path.exists(header), "include/rt_hip_instances.h is missing"
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(ENTRY_POINTS)
    lib = C.CDLL(rt.lib_path())
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in rt.api._SIGNATURES, name
    for method in ("set_instances", "instances", "trace_instances_closest", "trace_instances_occluded"):
        assert hasattr(rt.Host, method), method
    assert rt.INSTANCE_OUTPUTS == rt.api.QUERY_OUTPUTS + ("instance",) and rt.INSTANCE_NODE.itemsize == 32
    assert '#include "../oracle/rt_oracle.c"' in open(os.path.join(ROOT, "tests", "instance_oracle.c")).read()
    # the planner is free of the device runtime: its file names no HIP header
    planner = open(os.path.join(ROOT, "opencl_raytracer_amd", "csrc", "instances.cc")).read()
    assert "hip_runtime" not in planner and "rt_instance_plan" in planner


@pytest.mark.parametrize("n", cases.COUNTS)
def test_planner(rt, scene_for, n):
    _, arrays = scene_for("blob", "longest")
    lo, hi = cases.root_box(arrays)
    W = cases.many(arrays, n, seed=n)
    if n >= 3:
        W[1] = cases.family("mirror", arrays)[0]
        W[2] = cases.family("shear", arrays)[0]
    plan = rt.instance_plan(lo, hi, W)
    O, nodes = plan["object_from_world"], plan["nodes"]
    assert np.array_equal(O.view(np.uint32), restated_inverse(W).view(np.uint32))
    # ... which IS an inverse
    A, Q = W[:, :, :3].astype(np.float64), O[:, :, :3].astype(np.float64)
    assert np.abs(np.einsum("nij,njk->nik", A, Q) - np.eye(3)).max() < 1e-5
    check_tree(nodes, n)
    # each leaf box holds the float64 image of the root box's eight corners
    corners = np.array([[(hi if k >> a & 1 else lo)[a] for a in range(3)] for k in range(8)], np.float64)
    leaves = nodes[nodes["leaf"] != NONE]
    W64 = W.astype(np.float64)[leaves["leaf"]]
    image = np.einsum("nij,kj->nki", W64[:, :, :3], corners) + W64[:, None, :, 3]
    assert (image >= leaves["lo"][:, None, :].astype(np.float64)).all() and (image <= leaves["hi"][:, None, :].astype(np.float64)).all()
    # ... and no farther beyond it than the margin derived in csrc/instances.cc, restated: m_k = 2^-20 (G + sum_j |A_kj| q_j),
    # G = 4 x the set's reach, q_j = (|O_j0| + |O_j1| + |O_j2|) G + |O_j3|; plus the two outward steps in float32
    absW, absO = np.abs(W.astype(np.float64)), np.abs(O.astype(np.float64))
    reach = (absW[:, :, :3] @ np.maximum(np.abs(lo), np.abs(hi)).astype(np.float64) + absW[:, :, 3]).max()
    G = 4.0 * reach
    q = absO[:, :, :3].sum(axis=2) * G + absO[:, :, 3]
    margin = (2.0 ** -20 * (G + np.einsum("nkj,nj->nk", absW[:, :, :3], q)))[leaves["leaf"]]
    slack = margin + 2.0 ** -22 * (np.abs(image).max(axis=1) + margin)  # (two ulps of the float32 bound)
    assert ((image.min(axis=1) - leaves["lo"]) <= slack).all() and ((leaves["hi"] - image.max(axis=1)) <= slack).all()
    assert ((image.min(axis=1) - leaves["lo"]) >= margin * 0.999).all() and ((leaves["hi"] - image.max(axis=1)) >= margin * 0.999).all()
    # the same call twice: the same plan (nothing depends on the time of day)
    again = rt.instance_plan(lo, hi, W)
    assert np.array_equal(again["nodes"].tobytes(), nodes.tobytes())


def test_planner_with_a_root_box_that_is_not_finite(rt, scene_for):
    _, arrays = scene_for("blob", "longest")
    lo, hi = cases.root_box(arrays)
    W = cases.many(arrays, 5)
    for bad in (np.nan, np.inf):
        broken = hi.copy()
        broken[1] = bad
        nodes = rt.instance_plan(lo, broken, W)["nodes"]
        check_tree(nodes, 5)
        assert np.isneginf(nodes["lo"]).all() and np.isposinf(nodes["hi"]).all()


def test_odd_transforms_are_refused_and_leave_the_plan_in_place(rt, scene_for):
    _, arrays = scene_for("blob", "longest")
    lo, hi = cases.root_box(arrays)
    lib = rt.load_library()
    good = cases.many(arrays, 3)
    plan = rt.instance_plan(lo, hi, good)
    INVALID = rt.api.RT_E_INVALID
    for name, odd in cases.odd_transforms(arrays).items():
        for at in range(3):
            W = good.copy()
            W[at] = odd[0]
            O, nodes = plan["object_from_world"].copy(), plan["nodes"].copy()
            assert lib.rt_instance_plan(lo.ctypes.data, hi.ctypes.data, W.ctypes.data, 3, O.ctypes.data, nodes.ctypes.data) == INVALID, name
            assert O.tobytes() == plan["object_from_world"].tobytes() and nodes.tobytes() == plan["nodes"].tobytes(), name
        with pytest.raises(rt.RtError) as e:
            rt.instance_plan(lo, hi, odd)
        assert e.value.code == INVALID
    assert lib.rt_instance_plan(lo.ctypes.data, hi.ctypes.data, good.ctypes.data, 0, None, None) == INVALID
    assert lib.rt_instance_plan(lo.ctypes.data, hi.ctypes.data, good.ctypes.data, (1 << 20) + 1, None, None) == INVALID
    assert lib.rt_instance_plan(None, hi.ctypes.data, good.ctypes.data, 3, None, None) == INVALID
    assert lib.rt_instance_plan(lo.ctypes.data, hi.ctypes.data, good.ctypes.data, 3, None, None) == 0
    with pytest.raises(ValueError):
        rt.instance_plan(lo, hi, good.astype(np.float64))
    with pytest.raises(ValueError):
        rt.instance_plan(lo, hi, good[:, :, :3])


@pytest.mark.parametrize("family", cases.FAMILIES)
@pytest.mark.parametrize("bvh", BVHS)
@pytest.mark.parametrize("mesh", MESHES)
def test_oracle_against_the_reference(rt, scene_for, mesh, bvh, family):
    scene, arrays = scene_for(mesh, bvh)
    W = cases.family(family, arrays)
    plan = plan_for(rt, arrays, W)
    o, d = cases.rays(plan["nodes"], N_RAYS, seed=700 + cases.FAMILIES.index(family))
    max_distance = max_distance_of(mesh, family)
    key = (mesh, family)
    if key not in _REF:  # (the reference knows no tree: one answer for both builders)
        _REF[key] = ir.instanced(scene, W, o, d, max_distance)
        for v in _REF[key].values():
            v.setflags(write=False)
    ref = _REF[key]
    got = io.closest(arrays, plan, o, d, max_distance)
    occ = io.occluded(arrays, plan, o, d, max_distance)
    what = f"{mesh}/{bvh} {family} ({len(W)} instances) max_distance {max_distance}"
    assert np.array_equal(occ, got["hit"]), what
    for rep in (ir.compare_occluded(ref, occ), ir.compare_closest(scene, ref, got)):
        print(f"INSTANCES {what}: {rep}")
        bad = rep.failures(tol=ir.TOL, max_unjudged=0.01)
        assert not bad, (what, bad)
    assert (ref["count"] > 0).mean() > 0.005, what  # (no case passes on misses alone; a max_distance of 0.3 leaves few)
    if family == "tie_pair":
        assert (got["instance"][got["hit"].astype(bool)] == 0).all()
    # without a hit: the fill values, word for word
    free = ~got["hit"].astype(bool)
    assert np.isposinf(got["distance"][free]).all() and (got["leaf"][free] == NONE).all() and (got["instance"][free] == NONE).all()
    for f in ("barycentric", "position", "normal"):
        assert (got[f][free].view(np.uint32) == 0).all(), (what, f)


def test_identity_relation_on_the_oracles(rt, scene_for):
    """One identity instance, rays without -0: instance_oracle == query_oracle, word for word where the distance is finite."""
    for mesh in MESHES:
        for bvh in BVHS:
            _, arrays = scene_for(mesh, bvh)
            W = cases.family("identity", arrays)
            assert np.array_equal(W[0], np.eye(3, 4, dtype=np.float32))
            plan = plan_for(rt, arrays, W)
            assert np.array_equal(plan["object_from_world"][0], np.eye(3, 4, dtype=np.float32))
            o, d = cases.rays(plan["nodes"], N_RAYS, seed=811)
            oo, od = cases.odd_rays(plan["nodes"])
            o, d = cases.without_negative_zero(np.concatenate([o, oo]), np.concatenate([d, od]))
            for max_distance in cases.MAX_DISTANCES:
                got = io.closest(arrays, plan, o, d, max_distance)
                want = qo.closest(arrays, o, d, max_distance)
                assert np.array_equal(io.occluded(arrays, plan, o, d, max_distance), qo.occluded(arrays, o, d, max_distance)), (mesh, bvh)
                assert np.array_equal(got["hit"], want["hit"]) and want["hit"].any()
                at = want["distance"] < np.inf
                for f in ("hit", "distance", "leaf", "barycentric", "position", "normal"):
                    assert io.same_words(got[f][at], want[f][at]).all(), (mesh, bvh, f)
                assert (got["instance"][at] == 0).all()


def test_odd_rays_on_the_oracle(rt, scene_for):
    """Every float is legal: the oracle answers odd rays, and a ray without a direction or with a NaN hits nothing."""
    _, arrays = scene_for("blob", "longest")
    plan = plan_for(rt, arrays, cases.family("rotations", arrays))
    o, d = cases.odd_rays(plan["nodes"])
    got = io.closest(arrays, plan, o, d, 1e5)
    assert np.array_equal(io.occluded(arrays, plan, o, d, 1e5), got["hit"]) and got["hit"].any()
    quiet = (d == 0).all(axis=1) | np.isnan(o).any(axis=1) | np.isnan(d).any(axis=1)
    assert quiet.sum() > 100 and not got["hit"][quiet].any()


def test_planner_under_the_sanitizers():
    """tests/instances_sanitize.cc with csrc/instances.cc, -fsanitize=address,undefined, as a child process."""
    out = os.path.join(tempfile.mkdtemp(prefix="ocrt_instances_sanitize_"), "instances_sanitize")
    csrc = os.path.join(ROOT, "opencl_raytracer_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", out, os.path.join(ROOT, "tests", "instances_sanitize.cc"),
                    os.path.join(csrc, "instances.cc")], check=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "INSTANCES_SANITIZE_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
