"""CPU: the instanced closest-point queries' contract (include/rt_hip_instance_nearest.h) -- the brute-force C oracle
(tests/instance_nearest_oracle.c: csrc/instance_nearest.h, csrc/nearest_point.h) against the float64 reference
(tests/instance_nearest_reference.py), the header and the binding, the identity relation and the tie rule at oracle level,
the bounds' sweep and the host-side nested walk (tests/instance_nearest_margin_check.cc).  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import instance_cases as ic
import instance_nearest_cases as inc
import instance_nearest_oracle as ino
import instance_nearest_reference as inref
import nearest_cases as cases
import nearest_oracle as orc_n

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("rt_instances_closest_points", "rt_instances_closest_points_device")
MESHES = ("blob", "single", "ties", "handcrafted")


def test_header_library_and_binding(rt):
    header = os.path.join(ROOT, "include", "rt_hip_instance_nearest.h")
    assert os.path.exists(header), "include/rt_hip_instance_nearest.h is missing"
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(ENTRY_POINTS)
    import ctypes as C

    lib = C.CDLL(rt.lib_path())
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in rt.api._SIGNATURES, name
    assert hasattr(rt.Host, "instances_closest_points")
    # the shared arithmetic is ONE file: the kernel's translation unit, the oracle and the margin program all name it
    csrc = os.path.join(ROOT, "opencl_raytracer_amd", "csrc")
    assert '"instance_nearest.h"' in open(os.path.join(csrc, "kernels.hip")).read()
    assert "csrc/instance_nearest.h" in open(os.path.join(ROOT, "tests", "instance_nearest_oracle.c")).read()
    assert "csrc/instance_nearest.h" in open(os.path.join(ROOT, "tests", "instance_nearest_margin_check.cc")).read()
    shared = open(os.path.join(csrc, "instance_nearest.h")).read()
    assert "hip_runtime" not in shared and "#include <hip" not in shared
    # the sentence the issue quotes is corrected, and the older headers declare nothing new
    older = open(os.path.join(ROOT, "include", "rt_hip_instances.h")).read()
    assert "rt_hip_instance_nearest.h" in older and "closest_points" not in re.sub(r"/\*.*?\*/", "", older, flags=re.S)


@pytest.fixture(scope="module")
def meshes(rt, scene_for):
    out = {name: inc.Mesh(scene_for(name, "longest")[0]) for name in ("blob", "single", "ties")}
    out["handcrafted"] = inc.handcrafted_mesh(rt)
    return out


def point_sets(rt, meshes):
    """(case name, mesh, plan, points, radii): every family on every mesh; the large set on blob gets fewer points."""
    for m, name in enumerate(MESHES):
        mesh = meshes[name]
        for f, family in enumerate(ic.FAMILIES):
            plan = mesh.plan(rt, mesh.family(family))
            big = family == "grid" and name == "blob"
            n_box, n_surface = (120, 45) if big else (260, 90)
            pts = np.concatenate([inc.in_top_box(plan, n_box, 100 * m + f), inc.on_world_surface(mesh, plan, n_surface, 100 * m + f + 50),
                                  inc.far_from_set(plan, 10, 100 * m + f + 70)])
            yield f"{name} {family}", mesh, plan, pts, ((np.inf, 0.3) if big else cases.RADII)


@pytest.fixture(scope="module")
def measured(rt, meshes):
    """Every case through the oracle and the comparator, once."""
    worst, violations, answers = {k: 0.0 for k in inref.MEASURED}, [], {}
    for name, mesh, plan, points, radii in point_sets(rt, meshes):
        pairs = mesh.pairs(plan, points)
        for radius in radii:
            answer = mesh.oracle(plan, points, radius)
            answers[(name, radius)] = (plan, points, answer)
            got = mesh.compare(plan, points, radius, answer, pairs=pairs)
            violations += [f"{name}, radius {radius}: {v}" for v in got["violations"]]
            for k, x in got["measured"].items():
                worst[k] = max(worst[k], x)
    return worst, violations, answers


def test_oracle_against_the_reference(measured):
    """The two agree on every family and mesh within TOL = 8 x MEASURED, and MEASURED is what this run measures: not above
    the record, and the record not stale by 4 x."""
    worst, violations, _ = measured
    print("measured:", {k: float(f"{v:.3g}") for k, v in worst.items()})
    assert not violations, violations[:10]
    for check, value in worst.items():
        assert value <= inref.MEASURED[check] * 1.0000001, (check, value, inref.MEASURED[check])
        assert value >= inref.MEASURED[check] / 4.0, ("the record is stale: far above what is measured", check, value)


def test_radii_and_empty_records(measured):
    """`found` is distance <= max_distance in binary32 against the unbounded answer; a found record is the unbounded one."""
    _, _, answers = measured
    for mesh in MESHES:
        for family in ("rotations", "shear", "mirror"):
            _, _, free = answers[(f"{mesh} {family}", np.inf)]
            assert free["hit"].all()
            for radius in cases.RADII[1:]:
                _, _, got = answers[(f"{mesh} {family}", radius)]
                want = free["distance"] <= np.float32(radius)
                assert np.array_equal(got["hit"].astype(bool), want), (mesh, family, radius)
                for k in got:
                    assert ino.same_words(got[k][want], free[k][want]).all(), (mesh, family, radius, k)
                assert np.isposinf(got["distance"][~want]).all()
                assert (got["leaf"][~want] == ino.NONE).all() and (got["instance"][~want] == ino.NONE).all()
                for k in ("barycentric", "position", "normal"):
                    assert (got[k][~want] == 0).all()


def test_regions_are_all_exercised(rt, meshes):
    """blob under `rotations`, 500 points in each copy's own box x 1.5 (in the top-level box most points lie far from every
    copy, and a far point's nearest is a vertex): at least 10 % each nearest to a vertex, an edge's interior, a face's
    interior, and every copy answers for some."""
    blob = meshes["blob"]
    plan = blob.plan(rt, blob.family("rotations"))
    W = plan["world_from_object"].astype(np.float64)
    near = [cases.in_box(blob.vertices, 500, 7 + k).astype(np.float64) @ w[:, :3].T + w[:, 3] for k, w in enumerate(W)]
    answer = blob.oracle(plan, np.concatenate(near).astype(np.float32))
    assert answer["hit"].all()
    vertex, edge, face = cases.region_shares(answer["barycentric"])
    print(f"vertex {vertex:.3f}, edge {edge:.3f}, face {face:.3f}; instances {np.bincount(answer['instance'])}")
    assert min(vertex, edge, face) >= 0.10, (vertex, edge, face)
    assert len(np.unique(answer["instance"])) == len(plan["world_from_object"])


def test_identity_relation_on_the_oracles(rt, meshes):
    """One identity instance: every word is the plain oracle's, instance 0 where found.  (The header promises it for scenes
    without a -0; it holds on these four, blob's -0 coordinates included: none of them reaches an output word.)"""
    eye = np.zeros((1, 3, 4), np.float32)
    eye[0, :, :3] = np.eye(3)
    for name in MESHES:
        mesh = meshes[name]
        plan = mesh.plan(rt, eye)
        pts = np.concatenate([inc.mixed_points(mesh, plan, 400, 150, 20, 11), inc.odd_points(plan)])
        for radius in cases.RADII + cases.ODD_RADII:
            got = mesh.oracle(plan, pts, radius)
            want = orc_n.closest_points(mesh.leaf_faces, mesh.vertices, mesh.vnormals, pts, radius)
            for k in want:
                assert ino.same_words(got[k], want[k]).all(), (name, radius, k)
            assert np.array_equal(got["instance"], np.where(want["hit"] != 0, 0, ino.NONE))


def test_tie_pair_instance_zero_wins(rt, meshes):
    """The same transform twice: every pair ties, and the lower instance wins everywhere; its record is the single copy's."""
    for name in MESHES:
        mesh = meshes[name]
        W = mesh.family("tie_pair")
        plan, one = mesh.plan(rt, W), mesh.plan(rt, W[:1])
        pts = inc.mixed_points(mesh, plan, 400, 150, 20, 13)
        got, single = mesh.oracle(plan, pts), mesh.oracle(one, pts)
        assert got["hit"].all() and (got["instance"] == 0).all(), name
        for k in got:
            assert ino.same_words(got[k], single[k]).all(), (name, k)


def test_odd_inputs(rt, meshes):
    blob = meshes["blob"]
    plan = blob.plan(rt, blob.family("shear"))
    points = inc.in_top_box(plan, 40, 5)
    for radius in cases.ODD_RADII:
        got = blob.oracle(plan, points, radius)
        if radius == 0.0:  # (-0.0)
            assert np.array_equal(got["hit"], blob.oracle(plan, points, 0.0)["hit"])
            continue
        assert not got["hit"].any() and np.isposinf(got["distance"]).all() and (got["instance"] == ino.NONE).all(), radius
        assert not blob.compare(plan, points, radius, got)["violations"]
    odd = inc.odd_points(plan)
    got = blob.oracle(plan, odd)
    bad = ~np.isfinite(odd).all(axis=1)
    assert np.array_equal(got["hit"].astype(bool), ~bad)
    assert np.isposinf(got["distance"][bad]).all() and (got["position"][bad] == 0).all() and (got["instance"][bad] == ino.NONE).all()
    assert not blob.compare(plan, odd, np.inf, got)["violations"]


@pytest.fixture(scope="module")
def margin_program(tmp_path_factory):
    """tests/instance_nearest_margin_check.cc with the planner, built with the sanitizers as the stand-alone program it is."""
    exe = str(tmp_path_factory.mktemp("instance_nearest_margin") / "instance_nearest_margin_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "instance_nearest_margin_check.cc"),
                    os.path.join(ROOT, "opencl_raytracer_amd", "csrc", "instances.cc")], check=True)
    return exe


def test_margin_check_program(tmp_path, meshes, margin_program):
    """The sweep of both predicates, and the host-side nested walk of real trees and sets against brute force, bit for bit."""
    files = []
    for name, families in (("blob", ("rotations", "shear", "scales")), ("ties", ("mirror", "grid", "tie_pair")),
                           ("handcrafted", ("shear", "overlap_pair", "translations")), ("single", ("scales", "grid"))):
        for family in families:
            path = str(tmp_path / f"{name}_{family}.scene")
            inc.write_scene_file(path, meshes[name], meshes[name].family(family))
            files.append(path)
    path = str(tmp_path / "ties_many.scene")
    inc.write_scene_file(path, meshes["ties"], ic.many(meshes["ties"].scene, 300))
    done = subprocess.run([margin_program] + files + [path], capture_output=True, text=True)
    print(done.stdout[-2000:])
    assert done.returncode == 0, done.stdout[-3000:] + done.stderr[-3000:]
    assert "violations 0" in done.stdout and "walk mismatches 0" in done.stdout


def test_margin_check_program_has_teeth(margin_program):
    """With every copy's scale inflated by 2 % the sweep must find violations: the bound is not slack by that much."""
    done = subprocess.run([margin_program, "--inflate-scale", "1.02"], capture_output=True, text=True)
    print(done.stdout[-1500:])
    assert done.returncode == 1 and "violations 0" not in done.stdout, done.stdout[-3000:] + done.stderr[-3000:]


def test_host_walk_prunes_the_grid(tmp_path, meshes, margin_program):
    """`grid` (125 copies of blob), 4096 points in the top-level box: the host-side walk tests under a tenth of all pairs --
    the cap tests/test_instance_nearest_gpu.py holds the kernel's counters to."""
    path = str(tmp_path / "blob_grid.scene")
    inc.write_scene_file(path, meshes["blob"], meshes["blob"].family("grid"))
    done = subprocess.run([margin_program, "--box-points", "4096", path], capture_output=True, text=True)
    print(done.stdout[-1500:])
    assert done.returncode == 0, done.stdout[-3000:] + done.stderr[-3000:]
    share = float(re.search(r"share of all pairs tested ([0-9.eE+-]+)", done.stdout).group(1))
    assert share < 0.1, share
