"""CPU: the signed distance queries' contract (include/rt_hip_signed.h) -- the brute-force C oracle (tests/signed_oracle.c, the
arithmetic of csrc/signed_point.h) against the two float64 truths of tests/signed_reference.py, sp_angle against float64,
the sign table's shared edges, the feature codes, the header and the binding, and the sanitized stand-alone program
(tests/signed_check.cc).  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import distance_reference as ref
import nearest_cases as ncases
import nearest_oracle as orc_n
import signed_cases as cases
import signed_oracle as orc_s
import signed_reference as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("rt_signed_distance", "rt_signed_distance_device", "rt_signed_distance_grid", "rt_signed_distance_grid_device",
                "rt_prepare_signed_distance", "rt_last_sign_build_ms", "rt_debug_sign_table")


class Mesh:
    def __init__(self, rt, vertices, faces, closed, reversed_=False):
        self.scene = rt.Scene.from_arrays(np.asarray(vertices, np.float32), np.asarray(faces, np.uint32)).build_bvh(0)
        self.vertices, self.vnormals = self.scene.vertices.copy(), self.scene.vnormals.copy()
        self.faces = self.scene.faces.reshape(-1, 3).copy()
        self.leaf_faces = self.scene.sorted_faces.copy()
        self.closed, self.reversed = closed, reversed_
        self.normals = sref.Pseudonormals(self.vertices, self.faces)
        self.table = orc_s.table(self.leaf_faces, self.vertices)

    def oracle(self, points, radius=np.inf):
        return orc_s.signed_distance(self.leaf_faces, self.vertices, self.vnormals, points, radius, sign_table=self.table)

    def compare(self, points, inside, pairs=None):
        return sref.compare(points, self.vertices, self.faces, inside, self.closed, self.reversed, pairs=pairs, normals=self.normals)


@pytest.fixture(scope="module")
def meshes(rt, scene_for):
    out = {}
    for name, (v, f) in (("torus", cases.torus()), ("star", cases.star())):
        out[name] = Mesh(rt, v, f, True)
        out[name + " reversed"] = Mesh(rt, v, cases.reversed_faces(f), True, True)
    for name in ("blob", "ties", "single"):
        scene = scene_for(name, "longest")[0]
        out[name] = Mesh(rt, scene.vertices[:, :3], scene.faces.reshape(-1, 3), False)
    return out


def test_the_closed_meshes_are_closed(meshes):
    for name, faces, volume in (("torus", 576, 2.98), ("star", 28, 0.43)):
        m = meshes[name]
        assert len(m.faces) == faces and set(cases.edge_uses(m.faces).values()) == {2}
        assert abs(cases.signed_volume(m.vertices, m.faces) - volume) < 0.01, cases.signed_volume(m.vertices, m.faces)
        assert cases.signed_volume(m.vertices, meshes[name + " reversed"].faces) < 0.0
    assert len(meshes["star"].vertices) == 16
    centre = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.1], [0.0, 0.0, 0.0], [3.0, 0.0, 0.0]])
    assert np.abs(sref.winding_number(centre, meshes["torus"].vertices, meshes["torus"].faces) - [1, 0, 0, 0]).max() < 2e-15 * 8
    centre[0] = [0.7, 0.7, 0.2]  # (between two of the star's points)
    assert np.abs(sref.winding_number(centre, meshes["star"].vertices, meshes["star"].faces) - [0, 1, 1, 0]).max() < 2e-15 * 8


def point_sets(meshes):
    for name, m in meshes.items():
        yield name + " box", m, ncases.in_box(m.vertices, 3000, 1)
        yield name + " far", m, ncases.far_away(m.vertices, 200, 3)
        if m.closed:
            yield name + " features", m, cases.per_feature(m.vertices, m.faces)[0]


@pytest.fixture(scope="module")
def answers(meshes):
    out = {}
    for name, m, points in point_sets(meshes):
        pairs = ref.pair_distances(points, m.vertices, m.faces)
        out[name] = (m, points, pairs, m.oracle(points))
    return out


def test_oracle_against_both_truths(answers):
    """On every judged point the oracle's sign is the float64 pseudonormal's and, on the closed meshes, the winding number's;
    a reversed mesh negates it.  The record beside the sign is the closest-point oracle's, word for word."""
    for name, (m, points, pairs, got) in answers.items():
        held = m.compare(points, got["distance"] < 0, pairs=pairs)
        print(f"{name}: judged {held['judged']}, split {held['split']}, excluded {held['excluded']:.4%}, inside {float((got['distance'] < 0).mean()):.3f}")
        assert not held["violations"], (name, held["violations"])
        plain = orc_n.closest_points(m.leaf_faces, m.vertices, m.vnormals, points)
        for k in plain:
            mine = np.abs(got[k]) if k == "distance" else got[k]
            assert orc_n.same_words(mine, plain[k]).all(), (name, k)
    for name in ("torus", "star"):  # the same points, the faces reversed: every judged sign flips
        m, points, pairs, got = answers[name + " box"]
        _, _, _, back = answers[name + " reversed box"]
        judged = np.abs(got["distance"]) >= ref.TOL["distance"] * ref.scale_of(points, np.abs(got["distance"]))
        assert ((got["distance"] < 0) != (back["distance"] < 0))[judged].all(), name
    for name in ("torus features", "star features"):  # half of the per-feature set lies inside
        m, points, _, got = answers[name]
        half = len(points) // 2
        assert (got["distance"][:half] > 0).all() and (got["distance"][half:] < 0).all(), name


def test_every_feature_class_is_hit_by_name(answers, meshes):
    """The per-feature set: the oracle names the vertex, the edge or the face the point was displaced from."""
    for name in ("torus", "star"):
        m, points, _, got = answers[name + " features"]
        kinds = np.array(cases.per_feature(m.vertices, m.faces)[1])
        feature = got["feature"]
        # (a point displaced from a vertex or an edge is nearest to it only on a side where the surface is convex there: an
        # elliptic vertex of the torus is named from outside, a saddle vertex from neither side, a reflex edge from inside)
        on_vertex = np.isin(feature[kinds == "vertex"], (orc_s.VERTEX_A, orc_s.VERTEX_B, orc_s.VERTEX_C))
        on_edge = np.isin(feature[kinds == "edge"], (orc_s.EDGE_AB, orc_s.EDGE_AC, orc_s.EDGE_BC))
        print(f"{name}: vertices named {on_vertex.mean():.3f}, edges named {on_edge.mean():.3f}")
        assert on_vertex.mean() >= 0.2 and on_edge.mean() >= 0.4, (name, on_vertex.mean(), on_edge.mean())
        assert (feature[kinds == "face"] == orc_s.FACE).all(), name
        if name == "torus":
            assert set(np.unique(feature)) == {0, 1, 2, 3, 4, 5, 6}


def test_region_shares(answers):
    """3000 points in the box x 1.5: at least 10 % each nearest to a vertex, an edge and a face, by np_point.region."""
    for name in ("blob box", "star box"):
        feature = answers[name][3]["feature"]
        vertex, edge, face = (np.isin(feature, (1, 2, 3)).mean(), np.isin(feature, (4, 5, 6)).mean(), (feature == 0).mean())
        print(f"{name}: vertex {vertex:.3f}, edge {edge:.3f}, face {face:.3f}")
        assert min(vertex, edge, face) >= 0.10, (name, vertex, edge, face)
    # ... and the code agrees with the zeros among the barycentrics wherever those are clear-cut
    got = answers["blob box"][3]
    zeros = (np.abs(got["barycentric"]) < 1e-6).sum(axis=1)
    clear = (np.abs(got["barycentric"]) < 1e-6) | (np.abs(got["barycentric"]) > 1e-4)
    kind = np.where(got["feature"] == 0, 0, np.where(got["feature"] <= 3, 2, 1))
    assert (zeros == kind)[clear.all(axis=1)].all()


def test_doctored_answers_are_reported(answers, meshes):
    """Signs flipped on one feature class, and the face's normal where an edge's pseudonormal belongs."""
    for name in ("torus", "star"):
        m, points, pairs, got = answers[name + " box"]
        inside = got["distance"] < 0
        assert not m.compare(points, inside, pairs=pairs)["violations"]
        for codes in ((1, 2, 3), (4, 5, 6), (0,)):
            rows = np.isin(got["feature"], codes)
            assert rows.any()
            bad = m.compare(points, np.where(rows, ~inside, inside), pairs=pairs)["violations"]
            assert any(x.startswith("(i)") for x in bad) and any(x.startswith("(ii)") for x in bad), (name, codes, bad)
    m, points, pairs, got = answers["star box"]
    face_normal = m.table[got["leaf"], :3, 3]
    by_face = ((points.astype(np.float32) - got["position"]) * face_normal).sum(axis=1) < 0
    on_edge = np.isin(got["feature"], (4, 5, 6))
    wrong = np.where(on_edge, by_face, got["distance"] < 0)
    assert (wrong != (got["distance"] < 0)).sum() > 0, "no point of the star's box tells the face normal from the edge's"
    bad = m.compare(points, wrong, pairs=pairs)["violations"]
    assert any("(edge)" in x for x in bad), bad


def test_radii_and_odd_inputs(meshes):
    m = meshes["star"]
    points = np.concatenate([ncases.in_box(m.vertices, 300, 5), ncases.odd_points(m.vertices)])
    free = m.oracle(points)
    for radius in ncases.RADII[1:] + ncases.ODD_RADII:
        got = m.oracle(points, radius)
        want = (np.abs(free["distance"]) <= np.float32(radius)) & free["hit"].astype(bool) & bool(radius >= 0)
        assert np.array_equal(got["hit"].astype(bool), want), radius
        for k in got:
            assert orc_n.same_words(got[k][want], free[k][want]).all(), (radius, k)
        assert np.isposinf(got["distance"][~want]).all() and (got["feature"][~want] == orc_s.NO_FEATURE).all()
        assert (got["pseudonormal"][~want] == 0).all()
    on = m.oracle(m.vertices[:, :3].copy())  # points ON the surface are outside: +0
    assert (on["distance"] == 0).all() and not np.signbit(on["distance"]).any()


def corner_shapes():
    """Pairs of edge vectors from one corner: all angles from slivers of 1e-6 to nearly opposed, lengths from 1e-3 to 1e3."""
    rng = np.random.default_rng(11)
    for angle in np.concatenate([np.geomspace(1e-6, 1.0, 60), np.linspace(1.0, np.pi - 1e-3, 60), np.pi - np.geomspace(1e-6, 1e-3, 20)]):
        for _ in range(6):
            frame = np.linalg.qr(rng.normal(size=(3, 3)))[0]
            la, lb = 10.0 ** rng.uniform(-3, 3, size=2)
            yield (frame[0] * la).astype(np.float32), ((np.cos(angle) * frame[0] + np.sin(angle) * frame[1]) * lb).astype(np.float32)


def test_sp_angle_against_float64():
    worst = 0.0
    for a, b in corner_shapes():
        worst = max(worst, abs(float(orc_s.angle(a, b)) - sref.angle64(a, b)))
    print(f"sp_angle: worst difference {worst:.3g} (record {sref.MEASURED['angle']:.3g})")
    assert worst <= sref.TOL["angle"]
    assert worst <= sref.MEASURED["angle"] * 1.0000001 and worst >= sref.MEASURED["angle"] / 4.0, ("the record is stale", worst)
    zero = np.zeros(3, np.float32)
    x = np.array([1, 0, 0], np.float32)
    assert orc_s.angle(zero, x) == 0 and orc_s.angle(x, zero) == 0 and orc_s.angle(x, x) == 0
    assert orc_s.angle(x, -x) == np.float32(np.pi) and abs(float(orc_s.angle(x, np.array([0, 2, 0], np.float32))) - np.pi / 2) < 1e-6


def test_table_edges_agree_between_the_leaves_that_share_them(meshes):
    """Both leaves of a shared edge hold the same words; a vertex's words are the same in every leaf that names it; the sums
    are the float64 pseudonormals up to rounding."""
    for name in ("torus", "star", "blob", "ties"):
        m = meshes[name]
        lf = m.leaf_faces.reshape(-1, 3)
        edge_words, vertex_words = {}, {}
        for leaf, ids in enumerate(lf):
            for slot, (i, j) in enumerate(((0, 1), (0, 2), (1, 2))):
                key = (min(ids[i], ids[j]), max(ids[i], ids[j]))
                words = m.table[leaf, slot, :3].tobytes()
                assert edge_words.setdefault(key, words) == words, (name, leaf, slot)
            for corner in range(3):
                words = m.table[leaf, 3 + corner, :3].tobytes()
                assert vertex_words.setdefault(int(ids[corner]), words) == words, (name, leaf, corner)
        if m.closed:
            assert all(n == 2 for n in cases.edge_uses(lf).values())
        for key, words in edge_words.items():
            assert np.abs(np.frombuffer(words, np.float32) - m.normals.edge[key]).max() < 1e-5, (name, key)
        for x, words in vertex_words.items():
            assert np.abs(np.frombuffer(words, np.float32) - m.normals.vertex[x]).max() < 5e-5, (name, x)


def test_header_library_and_binding(rt):
    header = os.path.join(ROOT, "include", "rt_hip_signed.h")
    assert os.path.exists(header), "include/rt_hip_signed.h is missing"
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(ENTRY_POINTS)
    import ctypes as C

    lib = C.CDLL(rt.lib_path())
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in rt.api._SIGNATURES, name
    for method in ("signed_distance", "signed_distance_grid", "prepare_signed_distance", "last_sign_build_ms", "sign_table"):
        assert hasattr(rt.Host, method), method
    # the shared arithmetic is ONE file: the kernel's translation unit and the oracle both name it
    assert "signed_point.h" in open(os.path.join(ROOT, "opencl_raytracer_amd", "csrc", "kernels.hip")).read()
    assert "csrc/signed_point.h" in open(os.path.join(ROOT, "tests", "signed_oracle.c")).read()


def test_signed_check_program(tmp_path, meshes, answers):
    """tests/signed_check.cc, built with the sanitizers as the stand-alone program it is: the oracle over the per-feature sets;
    its signs are the ones this process computed."""
    exe = str(tmp_path / "signed_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "signed_check.cc")],
                   check=True)
    for name in ("torus", "star"):
        m, points, _, got = answers[name + " features"]
        path = str(tmp_path / (name + ".mesh"))
        with open(path, "wb") as out:
            np.array([len(m.leaf_faces) // 3, len(m.vertices), len(points)], np.uint32).tofile(out)
            np.ascontiguousarray(m.leaf_faces, np.uint32).tofile(out)
            np.ascontiguousarray(orc_s.as4(m.vertices), np.float32).tofile(out)
            np.ascontiguousarray(orc_s.as4(m.vnormals), np.float32).tofile(out)
            np.ascontiguousarray(orc_s.as4(points), np.float32).tofile(out)
            np.ascontiguousarray(got["distance"], np.float32).tofile(out)
        done = subprocess.run([exe, path], capture_output=True, text=True)
        print(done.stdout[-500:])
        assert done.returncode == 0, done.stdout[-3000:] + done.stderr[-3000:]
        assert "mismatches 0" in done.stdout and f"inside {int((got['distance'] < 0).sum())}" in done.stdout
