"""GPU: instanced closest-point queries (include/rt_hip_instance_nearest.h) against the brute-force CPU oracle of
tests/instance_nearest_oracle.c, every output word for word, and against the float64 comparator of
tests/instance_nearest_reference.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import instance_cases as ic
import instance_nearest_cases as inc
import instance_nearest_oracle as ino
import nearest_cases as cases

pytestmark = pytest.mark.gpu

FIELDS = ino.OUTPUTS
SORT_MIN = 16384  # RT_QUERY_SORT_MIN
MESHES = ("single", "ties", "blob", "handcrafted")


def new_host(rt):
    return rt.Host(rt.Options.defaults(width=64, height=48, n_super_samples=1), 0)


def mesh_for(rt, scene_for, name, bvh="longest"):
    return inc.handcrafted_mesh(rt, 0 if bvh == "longest" else 1) if name == "handcrafted" else inc.Mesh(scene_for(name, bvh)[0])


def posed(rt, mesh, W):
    """A host with the mesh uploaded and the set given; the plan is what the DEVICE holds."""
    host = new_host(rt)
    host.upload_scene(mesh.scene)
    host.set_instances(W)
    return host, host.instances()


def check(host, mesh, plan, points, radius=np.inf, what="", **kw):
    got = host.instances_closest_points(points, radius, **kw)
    ino.assert_same(got, mesh.oracle(plan, points, radius), what)
    return got


@pytest.mark.parametrize("mesh_name", MESHES)
@pytest.mark.parametrize("family", ic.FAMILIES)
def test_families_match_the_oracle(rt, scene_for, mesh_name, family):
    """About 2000 points in the top-level box x 1.25 and the odd points, every radius."""
    mesh = mesh_for(rt, scene_for, mesh_name)
    host, plan = posed(rt, mesh, mesh.family(family))
    points = np.concatenate([inc.in_top_box(plan, 2000, 50), inc.odd_points(plan)])
    for radius in cases.RADII + cases.ODD_RADII:
        check(host, mesh, plan, points, radius, (mesh_name, family, radius))
    host.close()


@pytest.mark.parametrize("family", ["rotations", "shear"])
def test_surface_and_far_points_and_the_float64_comparator(rt, scene_for, family):
    """blob: about 2000 points on the world surface and 1e3 sizes away; the comparator on the GPU's own answers."""
    mesh = mesh_for(rt, scene_for, "blob", "sah")
    host, plan = posed(rt, mesh, mesh.family(family))
    points = np.concatenate([inc.on_world_surface(mesh, plan, 1500, 60), inc.far_from_set(plan, 500, 61)])
    for radius in (np.inf, 0.02, 0.0):
        check(host, mesh, plan, points, radius, (family, radius))
    points = inc.mixed_points(mesh, plan, 600, 200, 20, 62)
    pairs = mesh.pairs(plan, points)
    for radius in (np.inf, 0.3):
        held = mesh.compare(plan, points, radius, host.instances_closest_points(points, radius), pairs=pairs)
        assert not held["violations"], held["violations"][:5]
    host.close()


@pytest.mark.parametrize("count", ic.COUNTS)
def test_instance_counts(rt, scene_for, count):
    mesh = mesh_for(rt, scene_for, "ties")
    host, plan = posed(rt, mesh, ic.many(mesh.scene, count))
    assert len(plan["nodes"]) == 2 * count - 1
    points = inc.mixed_points(mesh, plan, 1500, 400, 50, 70 + count)
    got = check(host, mesh, plan, points, what=("many", count))
    check(host, mesh, plan, points, 0.3, what=("many", count, 0.3))
    assert got["hit"].all() and got["instance"].max() < count
    host.close()


def test_batch_sizes(rt, scene_for):
    mesh = mesh_for(rt, scene_for, "blob")
    host, plan = posed(rt, mesh, mesh.family("rotations"))
    points = inc.in_top_box(plan, 257, 90)
    for n in (0, 1, 63, 64, 65, 257):
        got = check(host, mesh, plan, points[:n], what=("batch", n))
        assert got["hit"].shape == (n,) and got["position"].shape == (n, 3) and got["instance"].shape == (n,)
    host.close()


def test_bunny(rt, scene_for):
    """Three rotated copies, 1000 points."""
    mesh = mesh_for(rt, scene_for, "bunny")
    host, plan = posed(rt, mesh, mesh.family("rotations")[:3])
    points = inc.mixed_points(mesh, plan, 600, 250, 75, 95)
    assert len(points) == 1000
    got = check(host, mesh, plan, points, what="bunny")
    assert len(np.unique(got["instance"])) == 3
    host.close()


def test_sorted_unsorted_and_every_output_subset(rt, scene_for):
    """Unsorted, and sorted with three copies of the points to pass RT_QUERY_SORT_MIN; every output left out in turn, and
    each alone."""
    mesh = mesh_for(rt, scene_for, "blob", "sah")
    host, plan = posed(rt, mesh, mesh.family("shear"))
    one = inc.mixed_points(mesh, plan, 4000, 1200, 150, 80)
    points = np.concatenate([one, one, one])
    assert len(points) >= SORT_MIN
    want = {k: np.concatenate([x, x, x]) for k, x in mesh.oracle(plan, one, 0.3).items()}
    for sort in (True, False):
        ino.assert_same(host.instances_closest_points(points, 0.3, sort=sort), want, ("sort", sort))
        for left_out in FIELDS:
            names = tuple(k for k in FIELDS if k != left_out)
            got = host.instances_closest_points(points, 0.3, outputs=names, sort=sort)
            assert set(got) == set(names)
            ino.assert_same(got, want, ("without", left_out, sort))
        for only in FIELDS:
            ino.assert_same(host.instances_closest_points(points, 0.3, outputs=(only,), sort=sort), want, ("only", only, sort))
    assert host.last_query_ms > 0.0
    host.close()


def test_identity_relation_and_the_plain_query(rt, scene_for):
    """One identity instance: every word is closest_points', instance 0 where found -- and closest_points itself does not
    notice a set, whatever it holds."""
    eye = np.zeros((1, 3, 4), np.float32)
    eye[0, :, :3] = np.eye(3)
    for name in MESHES:
        mesh = mesh_for(rt, scene_for, name)
        host = new_host(rt)
        host.upload_scene(mesh.scene)
        points = np.concatenate([cases.in_box(mesh.vertices, 1500, 40), cases.on_surface(mesh.vertices, mesh.faces, 300, 41),
                                 cases.far_away(mesh.vertices, 50, 42), cases.odd_points(mesh.vertices)])
        before = {radius: host.closest_points(points, radius) for radius in (np.inf, 0.02)}
        host.set_instances(eye)
        for radius, plain in before.items():
            got = host.instances_closest_points(points, radius)
            for k in plain:
                assert ino.same_words(got[k], plain[k]).all(), (name, radius, k)
            assert np.array_equal(got["instance"], np.where(plain["hit"] != 0, 0, ino.NONE))
        host.set_instances(mesh.family("shear"))
        for radius, plain in before.items():
            again = host.closest_points(points, radius)
            for k in plain:
                assert ino.same_words(again[k], plain[k]).all(), ("plain query with a set", name, radius, k)
        host.close()


def displaced(vertices):
    moved = vertices.copy()
    moved[:, :3] += np.float32(0.05) * np.sin(7.0 * vertices[:, [1, 2, 0]]).astype(np.float32)
    return moved


def test_the_set_survives_update_vertices_and_build_scene(rt, scene_for):
    mesh = mesh_for(rt, scene_for, "blob")
    W = mesh.family("rotations")
    host, plan = posed(rt, mesh, W)
    points = inc.mixed_points(mesh, plan, 1500, 400, 50, 100)
    check(host, mesh, plan, points, what="uploaded")
    original = mesh.vertices
    mesh.vertices = displaced(original)
    host.update_vertices(mesh.vertices)  # (the normals stay as uploaded)
    plan = host.instances()
    assert np.array_equal(plan["world_from_object"], W)
    check(host, mesh, plan, points, what="updated")
    check(host, mesh, plan, points, 0.3, what="updated 0.3")
    mesh.vertices = original
    host.build_scene(original, mesh.faces, mesh.vnormals)
    mesh.face_of_leaf = host.face_of_leaf()
    mesh.leaf_faces = mesh.faces[mesh.face_of_leaf].reshape(-1)
    plan = host.instances()
    assert np.array_equal(plan["world_from_object"], W)
    got = check(host, mesh, plan, points, what="built")
    held = mesh.compare(plan, points, np.inf, got)
    assert not held["violations"], held["violations"][:5]
    host.close()


@pytest.mark.parametrize("damage", ["child_outside_parent", "leaf_box_beside_its_triangle", "nan_leaf_box", "inverted_box", "nan_vertex"])
def test_damaged_uploads_equal_brute_force(rt, scene_for, damage):
    """Arrays whose boxes promise nothing: the walk must lean on neither tree."""
    scene, arrays = scene_for("blob", "longest")
    mesh = inc.Mesh(scene)
    nodes, aabbs, verts, faces = arrays.nodes.copy(), arrays.aabbs.copy(), arrays.vertices.copy(), arrays.faces.copy()
    inner = int(np.flatnonzero(nodes > 8)[5])
    leaf = int(np.flatnonzero(nodes == 1)[40])
    if damage == "child_outside_parent":
        aabbs[2 * inner + 1, 0] = aabbs[2 * inner, 0] + 1.0e-3
    elif damage == "leaf_box_beside_its_triangle":
        aabbs[2 * leaf + 1, :3] = aabbs[2 * leaf, :3] + (aabbs[2 * leaf + 1, :3] - aabbs[2 * leaf, :3]) * np.float32(0.25)
    elif damage == "nan_leaf_box":
        aabbs[2 * leaf, 1] = np.nan
    elif damage == "inverted_box":
        aabbs[2 * inner, 0], aabbs[2 * inner + 1, 0] = aabbs[2 * inner + 1, 0], aabbs[2 * inner, 0]
    elif damage == "nan_vertex":
        verts[int(arrays.faces[3 * 17]), 1] = np.nan
    W = mesh.family("shear")
    good = mesh.plan(rt, W)  # (points from the undamaged plan; the oracle needs the transforms and inverses alone)
    host = new_host(rt)
    host.upload(faces, nodes, aabbs, verts, arrays.normals)
    host.set_instances(W)
    mesh.leaf_faces, mesh.vertices, mesh.vnormals = faces, verts, arrays.normals
    points = inc.mixed_points(mesh if damage != "nan_vertex" else inc.Mesh(scene), good, 1200, 300, 50, 110)
    check(host, mesh, good, points, what=damage)
    check(host, mesh, good, points, 0.3, what=damage)
    host.close()


class _DeviceBytes:
    def __init__(self, size):
        self.hip, self.ptr = C.CDLL("libamdhip64.so"), C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.ptr), C.c_size_t(size)) == 0
        assert self.hip.hipMemset(self.ptr, 0, C.c_size_t(size)) == 0

    def free(self):
        self.hip.hipFree(self.ptr)


def test_error_paths(rt, scene_for):
    lib = rt.load_library()
    STATE, INVALID = rt.api.RT_E_STATE, rt.api.RT_E_INVALID
    mesh = mesh_for(rt, scene_for, "blob")
    W = mesh.family("rotations")
    host = new_host(rt)
    p = np.zeros((4, 3), np.float32)
    p4 = np.zeros((4, 4), np.float32)
    inf = float("inf")
    with pytest.raises(rt.RtError) as e:  # before an upload
        host.instances_closest_points(p)
    assert e.value.code == STATE
    host.set_instances(W)  # (a set may be given before an upload; the query still needs one)
    assert lib.rt_instances_closest_points(host._h, p4.ctypes.data, 4, inf, 0, None) == STATE
    host.upload_scene(mesh.scene)
    assert lib.rt_instances_closest_points(host._h, p4.ctypes.data, 4, inf, 0, None) == 0  # (no outputs: nothing is written)
    host.set_instances(np.zeros((0, 3, 4), np.float32))  # without a set
    assert lib.rt_instances_closest_points(host._h, p4.ctypes.data, 4, inf, 0, None) == STATE
    assert lib.rt_instances_closest_points_device(host._h, p4.ctypes.data, 4, inf, 0, None, None) == STATE
    assert lib.rt_instances_closest_points(host._h, None, 0, inf, 0, None) == STATE  # (the set comes before the count)
    host.set_instances(W)
    assert lib.rt_instances_closest_points(host._h, None, 4, inf, 0, None) == INVALID
    assert lib.rt_instances_closest_points_device(host._h, None, 4, inf, 0, None, None) == INVALID
    assert lib.rt_instances_closest_points(host._h, None, 0, inf, 0, None) == 0
    assert lib.rt_instances_closest_points(host._h, p4.ctypes.data, (1 << 27) + 1, inf, 0, None) == INVALID
    assert lib.rt_instances_closest_points(None, p4.ctypes.data, 4, inf, 0, None) == INVALID
    with pytest.raises(ValueError):
        host.instances_closest_points(p.astype(np.float64))
    with pytest.raises(ValueError):
        host.instances_closest_points(p, outputs=("hit", "colour"))
    mem = _DeviceBytes(65 * 16 + 1024)
    points, out = mem.ptr.value, mem.ptr.value + 65 * 16
    assert lib.rt_instances_closest_points_device(host._h, points + 4, 64, inf, 0, None, None) == INVALID
    hits = rt.api._HitArrays(None, out + 2, None, None, None, None)
    assert lib.rt_instances_closest_points_device(host._h, points, 64, inf, 0, C.byref(rt.api._InstanceHitArrays(hits, None)), None) == INVALID
    hits = rt.api._HitArrays(out + 1, out + 4, None, None, None, None)  # (the flags are bytes: any address)
    assert lib.rt_instances_closest_points_device(host._h, points, 64, inf, 0, C.byref(rt.api._InstanceHitArrays(hits, out + 514)), None) == INVALID
    assert lib.rt_instances_closest_points_device(host._h, points, 64, inf, 0, C.byref(rt.api._InstanceHitArrays(hits, out + 512)), None) == 0
    host.close()
    mem.free()
    ring = rt.FrameRing(rt.Options.defaults(width=32, height=32, ao_num_samples=3), hosts=2)
    ring.set_calibration(False)
    ring.upload_scene(mesh.scene)
    with pytest.raises(rt.RtError) as e:
        ring.host(0).instances_closest_points(p)
    assert e.value.code == STATE
    ring.close()


def test_pruning_on_the_grid(rt_knobs, scene_for_knobs):
    """`grid` (125 copies of blob), 4096 points in the top-level box: the counted kernel gives the product's words, and its
    triangle tests stay under a tenth of points x instances x leaves (tests/test_instance_nearest_cpu.py holds the host-side
    walk to the same cap for the same case); without pruning every pair is tested."""
    rt = rt_knobs
    mesh = inc.Mesh(scene_for_knobs("blob", "longest")[0])
    host, plan = posed(rt, mesh, mesh.family("grid"))
    points = inc.in_top_box(plan, 4096, 120, factor=1.0)
    want = mesh.oracle(plan, points)
    host.set_nearest_walk(count=True)
    ino.assert_same(host.instances_closest_points(points), want, "counted")
    boxes, triangles = host.last_nearest_counts()
    pairs = len(points) * 125 * mesh.leaves
    print(f"box tests per point {boxes / len(points):.1f}, triangle tests per point {triangles / len(points):.1f}, share {triangles / pairs:.5f}")
    assert 0 < triangles < pairs / 10, (triangles, pairs)
    host.set_nearest_walk(count=True, no_start=True)
    ino.assert_same(host.instances_closest_points(points[:512]), {k: v[:512] for k, v in want.items()}, "no starting bound")
    host.set_nearest_walk(count=True, no_prune=True)
    ino.assert_same(host.instances_closest_points(points[:256]), {k: v[:256] for k, v in want.items()}, "no pruning")
    assert host.last_nearest_counts()[1] == 256 * 125 * mesh.leaves
    host.set_nearest_walk()
    ino.assert_same(host.instances_closest_points(points), want, "product form")
    host.close()


def test_torch_path_equals_numpy_path():
    """A device tensor in and device tensors out on a non-default stream == the numpy path
    (tests/instance_nearest_torch_driver.py, a child process that brings torch's runtime up before it loads the library)."""
    driver = os.path.join(os.path.dirname(os.path.abspath(__file__)), "instance_nearest_torch_driver.py")
    r = subprocess.run([sys.executable, driver], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "INSTANCE_NEAREST_TORCH_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
