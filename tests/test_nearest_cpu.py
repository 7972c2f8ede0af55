"""CPU: the closest-point queries' contract (include/rt_hip_nearest.h) -- the brute-force C oracle (tests/nearest_oracle.c,
the routine of csrc/nearest_point.h) against the float64 reference (tests/distance_reference.py), the header and the
binding, the pruning margin's sweep and the host-side walk (tests/nearest_margin_check.cc).  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import distance_reference as ref
import nearest_cases as cases
import nearest_oracle as orc_n

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("rt_closest_points", "rt_closest_points_device")


def test_header_library_and_binding(rt):
    header = os.path.join(ROOT, "include", "rt_hip_nearest.h")
    assert os.path.exists(header), "include/rt_hip_nearest.h is missing"
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(ENTRY_POINTS)
    import ctypes as C

    lib = C.CDLL(rt.lib_path())
    for name in ENTRY_POINTS + ("rt_debug_set_nearest_walk", "rt_debug_last_nearest_counts"):
        assert hasattr(lib, name), name
        assert name in rt.api._SIGNATURES, name
    assert hasattr(rt.Host, "closest_points")
    assert rt.NEAREST_OUTPUTS == ("hit", "distance", "leaf", "barycentric", "position", "normal")
    # the shared arithmetic is ONE file: the kernel's translation unit and the oracle both name it
    assert "nearest_point.h" in open(os.path.join(ROOT, "opencl_raytracer_amd", "csrc", "kernels.hip")).read()
    assert "csrc/nearest_point.h" in open(os.path.join(ROOT, "tests", "nearest_oracle.c")).read()


class Mesh:
    """A mesh with a tree: what the oracle (leaf order) and the reference (file order) each need of it."""

    def __init__(self, scene):
        self.scene = scene
        self.vertices, self.vnormals = scene.vertices.copy(), scene.vnormals.copy()
        self.faces = scene.faces.reshape(-1, 3).copy()
        self.leaf_faces = scene.sorted_faces.copy()
        self.face_of_leaf = scene.face_of_leaf().copy()

    def oracle(self, points, radius=np.inf):
        return orc_n.closest_points(self.leaf_faces, self.vertices, self.vnormals, points, radius)

    def compare(self, points, radius, answer, pairs=None):
        return ref.compare(points, self.vertices, self.vnormals, self.faces, self.face_of_leaf, radius, answer, pairs=pairs)


@pytest.fixture(scope="module")
def meshes(rt, scene_for):
    out = {name: Mesh(scene_for(name, "longest")[0]) for name in ("blob", "single", "ties", "interior_hard")}
    v, f = cases.handcrafted()
    out["handcrafted"] = Mesh(rt.Scene.from_arrays(v, f).build_bvh(0))
    return out


def point_sets(meshes):
    """(name, mesh, points, radii)"""
    blob = meshes["blob"]
    yield "blob box", blob, cases.in_box(blob.vertices, 3000, 1), cases.RADII
    yield "blob surface", blob, cases.on_surface(blob.vertices, blob.faces, 1000, 2), cases.RADII
    yield "blob far", blob, cases.far_away(blob.vertices, 1000, 3), (np.inf,)
    for k, name in enumerate(("single", "ties", "handcrafted")):
        m = meshes[name]
        pts = np.concatenate([cases.in_box(m.vertices, 300, 10 + k), cases.on_surface(m.vertices, m.faces, 90, 20 + k)])
        yield name, m, pts, cases.RADII
    hard = meshes["interior_hard"]
    yield "interior_hard", hard, cases.in_box(hard.vertices, 150, 4, factor=1.1), (np.inf, 0.3)


@pytest.fixture(scope="module")
def measured(meshes):
    """Every case through the oracle and the comparator, once: ({check: worst}, [violation ...], {case: oracle answer})."""
    worst, violations, answers = {k: 0.0 for k in ref.MEASURED}, [], {}
    for name, mesh, points, radii in point_sets(meshes):
        pairs = ref.pair_distances(points, mesh.vertices, mesh.faces)
        for radius in radii:
            answer = mesh.oracle(points, radius)
            answers[(name, radius)] = (points, answer)
            got = mesh.compare(points, radius, answer, pairs=pairs)
            violations += [f"{name}, radius {radius}: {v}" for v in got["violations"]]
            for k, x in got["measured"].items():
                worst[k] = max(worst[k], x)
    return worst, violations, answers


def test_oracle_against_the_reference(measured):
    """The two oracles agree on every case within TOL = 8 x MEASURED, and MEASURED is what this run measures (the constants
    of tests/distance_reference.py are a record of it, not a wish: a figure above the record fails here)."""
    worst, violations, _ = measured
    print("measured:", {k: float(f"{v:.3g}") for k, v in worst.items()})
    assert not violations, violations[:10]
    for check, value in worst.items():
        assert value <= ref.MEASURED[check] * 1.0000001, (check, value, ref.MEASURED[check])
        assert value >= ref.MEASURED[check] / 4.0, ("the record is stale: far above what is measured", check, value)


def test_regions_are_all_exercised(measured):
    """blob, 3000 points in its box x 1.5: at least 10 % each nearest to a vertex, an edge's interior, a face's interior."""
    _, _, answers = measured
    _, answer = answers[("blob box", np.inf)]
    assert answer["hit"].all()
    vertex, edge, face = cases.region_shares(answer["barycentric"])
    print(f"vertex {vertex:.3f}, edge {edge:.3f}, face {face:.3f}; distances {answer['distance'].min():.3g} .. {answer['distance'].max():.3g}")
    assert min(vertex, edge, face) >= 0.10, (vertex, edge, face)


def test_radii(measured):
    """`found` is distance <= max_distance in binary32 against the unbounded answer, and a found record is the unbounded one."""
    _, _, answers = measured
    for name in ("blob box", "blob surface", "single", "ties", "handcrafted"):
        points, free = answers[(name, np.inf)]
        assert free["hit"].all(), name
        for radius in cases.RADII[1:]:
            _, got = answers[(name, radius)]
            want = free["distance"] <= np.float32(radius)
            assert np.array_equal(got["hit"].astype(bool), want), (name, radius)
            for k in got:
                assert orc_n.same_words(got[k][want], free[k][want]).all(), (name, radius, k)
            assert np.isposinf(got["distance"][~want]).all() and (got["leaf"][~want] == orc_n.NONE).all()
            for k in ("barycentric", "position", "normal"):
                assert (got[k][~want] == 0).all(), (name, radius, k)
    # a radius of 0 finds the points that ARE vertices
    points, got = answers[("blob surface", 0.0)]
    assert got["hit"][:300].all()


def test_odd_inputs(meshes):
    blob = meshes["blob"]
    points = cases.in_box(blob.vertices, 40, 5)
    for radius in cases.ODD_RADII:
        got = blob.oracle(points, radius)
        if radius == 0.0:  # (-0.0)
            assert np.array_equal(got["hit"], blob.oracle(points, 0.0)["hit"])
            continue
        assert not got["hit"].any() and np.isposinf(got["distance"]).all() and (got["leaf"] == orc_n.NONE).all(), radius
        assert not blob.compare(points, radius, got)["violations"]
    odd = cases.odd_points(blob.vertices)
    got = blob.oracle(odd)
    bad = ~np.isfinite(odd).all(axis=1)
    assert np.array_equal(got["hit"].astype(bool), ~bad)
    assert np.isposinf(got["distance"][bad]).all() and (got["position"][bad] == 0).all()
    assert not blob.compare(odd, np.inf, got)["violations"]


def test_degenerate_faces_and_ties(meshes):
    """No NaN for finite input on the meshes with faces that are segments or points; of coincident leaves the lowest wins."""
    for name in ("ties", "handcrafted"):
        m = meshes[name]
        pts = np.concatenate([cases.in_box(m.vertices, 500, 30), cases.on_surface(m.vertices, m.faces, 99, 31)])
        got = m.oracle(pts)
        assert got["hit"].all() and np.isfinite(got["distance"]).all() and np.isfinite(got["position"]).all(), name
        for leaf in range(len(m.face_of_leaf)):
            for q in pts[:50]:
                one = orc_n.pair(m.leaf_faces, m.vertices, leaf, q)
                assert np.isfinite(one["d2"]) and 0.0 <= one["s"] <= 1.0 and 0.0 <= one["t"] <= 1.0, (name, leaf, q, one)
    m = meshes["handcrafted"]
    coincident = sorted(leaf for leaf, face in enumerate(m.face_of_leaf) if face in (0, 1, 2))  # (cases.handcrafted)
    assert len(coincident) == 3
    above = np.array([[0.25, 0.25, 0.3], [0.1, 0.2, -0.2], [0.3, 0.3, 0.0]], dtype=np.float32)
    got = m.oracle(above)
    assert (got["leaf"] == coincident[0]).all(), (got["leaf"], coincident)
    # the point triangle answers with its point
    got = m.oracle(np.array([[2.5, 2.5, 2.5]], dtype=np.float32))
    assert np.array_equal(got["position"][0], np.float32([2, 2, 2])) and m.face_of_leaf[got["leaf"][0]] == 3


def test_doctored_answers_are_reported(meshes):
    """Each of three wrong answers the comparator must name: the leaf swapped for a farther neighbour, the position pushed
    off the face, the distance of the second-nearest face."""
    blob = meshes["blob"]
    points = cases.in_box(blob.vertices, 200, 6)
    good = blob.oracle(points)
    pairs = ref.pair_distances(points, blob.vertices, blob.faces)
    assert not blob.compare(points, np.inf, good, pairs=pairs)["violations"]
    order = np.argsort(pairs, axis=1)
    leaf_of_face = np.empty(len(blob.face_of_leaf), np.int64)
    leaf_of_face[blob.face_of_leaf] = np.arange(len(blob.face_of_leaf))
    # a farther neighbour: the first face in distance order that lies clearly farther
    rows = np.arange(len(points))
    farther = np.array([next(f for f in order[i] if pairs[i, f] > pairs[i, order[i, 0]] + 1e-3) for i in rows])

    def doctored(**changes):
        bad = {k: v.copy() for k, v in good.items()}
        for k, v in changes.items():
            bad[k][:20] = v[:20]
        return [x for x in blob.compare(points, np.inf, bad, pairs=pairs)["violations"]]

    swapped = doctored(leaf=leaf_of_face[farther].astype(np.uint32))
    assert any(x.startswith("(c)") for x in swapped), swapped
    pushed = doctored(position=good["position"] + np.float32(1e-3) * good["normal"])
    assert any(x.startswith("(d)") for x in pushed), pushed
    second = doctored(distance=pairs[rows, farther].astype(np.float32))
    assert any(x.startswith("(b)") for x in second) and any(x.startswith("(f)") for x in second), second


def test_margin_check_program(tmp_path, meshes):
    """tests/nearest_margin_check.cc, built with the sanitizers as the stand-alone program it is: the predicate's sweep, and
    the host-side walk of real trees against brute force, bit for bit."""
    exe = str(tmp_path / "nearest_margin_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "nearest_margin_check.cc")], check=True)
    files = []
    for name in ("blob", "ties", "handcrafted", "single"):
        m = meshes[name]
        path = str(tmp_path / (name + ".scene"))
        nodes, aabbs = m.scene.nodes, m.scene.aabbs
        with open(path, "wb") as out:
            np.array([len(nodes), len(m.leaf_faces) // 3, len(m.vertices)], np.uint32).tofile(out)
            np.ascontiguousarray(nodes, np.uint32).tofile(out)
            np.ascontiguousarray(aabbs, np.float32).tofile(out)
            np.ascontiguousarray(m.leaf_faces, np.uint32).tofile(out)
            np.ascontiguousarray(m.vertices, np.float32).tofile(out)
        files.append(path)
    done = subprocess.run([exe] + files, capture_output=True, text=True)
    print(done.stdout[-2000:])
    assert done.returncode == 0, done.stdout[-3000:] + done.stderr[-3000:]
    assert "violations 0" in done.stdout and "walk mismatches 0" in done.stdout
