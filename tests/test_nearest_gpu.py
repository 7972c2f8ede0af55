"""GPU: closest-point queries (include/rt_hip_nearest.h) against the brute-force CPU oracle of tests/nearest_oracle.c, every
output word for word, and against the float64 comparator of tests/distance_reference.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import distance_reference as ref
import nearest_cases as cases
import nearest_oracle as orc_n
import orc
from conftest import bits

pytestmark = pytest.mark.gpu

FIELDS = orc_n.OUTPUTS
SORT_MIN = 16384  # RT_QUERY_SORT_MIN


def new_host(rt):
    return rt.Host(rt.Options.defaults(width=64, height=48, n_super_samples=1), 0)


def mixed_points(vertices, faces, n_box, n_surface, n_far, seed):
    return np.concatenate([cases.in_box(vertices, n_box, seed), cases.on_surface(vertices, faces, n_surface, seed + 1),
                           cases.far_away(vertices, n_far, seed + 2), cases.shell(vertices, n_far, seed + 3)])


def check(host, leaf_faces, vertices, normals, points, radius=np.inf, what="", **kw):
    got = host.closest_points(points, radius, **kw)
    want = orc_n.closest_points(leaf_faces, vertices, normals, points, radius)
    orc_n.assert_same(got, want, what)
    return got


@pytest.mark.parametrize("mesh,bvh", [("single", "longest"), ("ties", "longest"), ("ties", "sah"), ("blob", "longest"), ("blob", "sah")])
def test_uploaded_scenes_match_the_oracle(rt, scene_for, mesh, bvh):
    scene, _ = scene_for(mesh, bvh)
    host = new_host(rt)
    host.upload_scene(scene)
    v, n, f = scene.vertices, scene.vnormals, scene.faces.reshape(-1, 3)
    points = np.concatenate([mixed_points(v, f, 1500, 600, 100, 50), cases.odd_points(v)])
    for radius in cases.RADII + cases.ODD_RADII:
        got = check(host, scene.sorted_faces, v, n, points, radius, (mesh, bvh, radius))
    if mesh == "blob":  # the float64 comparator on the GPU's own answers
        for radius in (np.inf, 0.3):
            got = host.closest_points(points, radius)
            held = ref.compare(points, v, n, f, scene.face_of_leaf(), radius, got)
            assert not held["violations"], held["violations"][:5]
    host.close()


def test_handcrafted_mesh_and_the_lowest_leaf(rt):
    v, f = cases.handcrafted()
    for method in (0, 1):
        scene = rt.Scene.from_arrays(v, f).build_bvh(method)
        host = new_host(rt)
        host.upload_scene(scene)
        points = mixed_points(scene.vertices, f, 800, 300, 50, 60)
        got = check(host, scene.sorted_faces, scene.vertices, scene.vnormals, points, what=("handcrafted", method))
        assert got["hit"].all() and np.isfinite(got["distance"]).all()
        coincident = sorted(leaf for leaf, face in enumerate(scene.face_of_leaf()) if face in (0, 1, 2))
        above = host.closest_points(np.array([[0.25, 0.25, 0.3], [0.1, 0.2, -0.2]], dtype=np.float32))
        assert (above["leaf"] == coincident[0]).all()
        host.close()


def test_bunny(rt, scene_for):
    scene, _ = scene_for("bunny", "longest")
    host = new_host(rt)
    host.upload_scene(scene)
    v, f = scene.vertices, scene.faces.reshape(-1, 3)
    points = mixed_points(v, f, 1200, 500, 150, 70)
    assert len(points) == 2000
    check(host, scene.sorted_faces, v, scene.vnormals, points, what="bunny")
    check(host, scene.sorted_faces, v, scene.vnormals, points, 0.02, what="bunny 0.02")
    host.close()


def test_sorted_unsorted_and_every_output_subset(rt, scene_for):
    """Unsorted, and sorted with three copies of the points to pass RT_QUERY_SORT_MIN; every output left out in turn."""
    scene, _ = scene_for("blob", "sah")
    host = new_host(rt)
    host.upload_scene(scene)
    v, f = scene.vertices, scene.faces.reshape(-1, 3)
    one = mixed_points(v, f, 3500, 1500, 300, 80)
    points = np.concatenate([one, one, one])
    assert len(points) >= SORT_MIN
    want = orc_n.closest_points(scene.sorted_faces, v, scene.vnormals, one, 0.3)
    want = {k: np.concatenate([x, x, x]) for k, x in want.items()}
    for sort in (True, False):
        orc_n.assert_same(host.closest_points(points, 0.3, sort=sort), want, ("sort", sort))
        for left_out in FIELDS:
            names = tuple(k for k in FIELDS if k != left_out)
            got = host.closest_points(points, 0.3, outputs=names, sort=sort)
            assert set(got) == set(names)
            orc_n.assert_same(got, want, ("without", left_out, sort))
        for only in FIELDS:
            orc_n.assert_same(host.closest_points(points, 0.3, outputs=(only,), sort=sort), want, ("only", only, sort))
    assert host.last_query_ms > 0.0
    host.close()


def test_batch_sizes(rt, scene_for):
    scene, _ = scene_for("blob", "longest")
    host = new_host(rt)
    host.upload_scene(scene)
    points = cases.in_box(scene.vertices, 257, 90)
    for n in (0, 1, 63, 64, 65, 257):
        got = check(host, scene.sorted_faces, scene.vertices, scene.vnormals, points[:n], what=("batch", n))
        assert got["hit"].shape == (n,) and got["position"].shape == (n, 3)
    host.close()


def displaced(vertices):
    moved = vertices.copy()
    moved[:, :3] += np.float32(0.05) * np.sin(7.0 * vertices[:, [1, 2, 0]]).astype(np.float32)
    return moved


def test_after_update_vertices_and_after_build_scene(rt, scene_for):
    scene, _ = scene_for("blob", "longest")
    v, n, f = scene.vertices.copy(), scene.vnormals.copy(), scene.faces.reshape(-1, 3).copy()
    points = mixed_points(v, f, 1500, 500, 100, 100)
    host = new_host(rt)
    host.upload_scene(scene)
    moved = displaced(v)
    host.update_vertices(moved)  # (the normals stay as uploaded)
    check(host, scene.sorted_faces, moved, n, points, what="updated")
    check(host, scene.sorted_faces, moved, n, points, 0.02, what="updated 0.02")
    host.build_scene(v, f, n)
    leaf_faces = f[host.face_of_leaf()].reshape(-1)
    got = check(host, leaf_faces, v, n, points, what="built")
    held = ref.compare(points, v, n, f, host.face_of_leaf(), np.inf, got)
    assert not held["violations"], held["violations"][:5]
    host.update_vertices(moved)
    check(host, leaf_faces, moved, n, points, 0.3, what="built, then updated")
    host.close()


@pytest.mark.parametrize("damage", ["child_outside_parent", "leaf_box_beside_its_triangle", "nan_leaf_box", "inverted_box", "nan_vertex"])
def test_damaged_uploads_equal_brute_force(rt, scene_for, damage):
    """Arrays whose boxes promise nothing: the walk must not lean on them."""
    _, arrays = scene_for("blob", "longest")
    nodes, aabbs, verts, faces = arrays.nodes.copy(), arrays.aabbs.copy(), arrays.vertices.copy(), arrays.faces.copy()
    inner = int(np.flatnonzero(nodes > 8)[5])
    leaf = int(np.flatnonzero(nodes == 1)[40])
    if damage == "child_outside_parent":
        aabbs[2 * inner + 1, 0] = aabbs[2 * inner, 0] + 1.0e-3
    elif damage == "leaf_box_beside_its_triangle":  # (regular and nested still: only the packer's look at the vertices finds it)
        aabbs[2 * leaf + 1, :3] = aabbs[2 * leaf, :3] + (aabbs[2 * leaf + 1, :3] - aabbs[2 * leaf, :3]) * np.float32(0.25)
    elif damage == "nan_leaf_box":
        aabbs[2 * leaf, 1] = np.nan
    elif damage == "inverted_box":
        aabbs[2 * inner, 0], aabbs[2 * inner + 1, 0] = aabbs[2 * inner + 1, 0], aabbs[2 * inner, 0]
    elif damage == "nan_vertex":
        verts[int(arrays.faces[3 * 17]), 1] = np.nan
    host = new_host(rt)
    host.upload(faces, nodes, aabbs, verts, arrays.normals)
    points = mixed_points(arrays.vertices, arrays.faces.reshape(-1, 3), 1500, 500, 50, 110)
    check(host, faces, verts, arrays.normals, points, what=damage)
    check(host, faces, verts, arrays.normals, points, 0.02, what=damage)
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
    scene, _ = scene_for("blob", "longest")
    host = new_host(rt)
    p = np.zeros((4, 3), np.float32)
    with pytest.raises(rt.RtError) as e:
        host.closest_points(p)
    assert e.value.code == rt.api.RT_E_STATE
    host.upload_scene(scene)
    inf = float("inf")
    assert lib.rt_closest_points(host._h, None, 4, inf, 0, None) == rt.api.RT_E_INVALID
    assert lib.rt_closest_points_device(host._h, None, 4, inf, 0, None, None) == rt.api.RT_E_INVALID
    assert lib.rt_closest_points(host._h, None, 0, inf, 0, None) == 0
    p4 = np.zeros((4, 4), np.float32)
    assert lib.rt_closest_points(host._h, p4.ctypes.data, (1 << 27) + 1, inf, 0, None) == rt.api.RT_E_INVALID
    assert lib.rt_closest_points(host._h, p4.ctypes.data, 4, inf, 0, None) == 0  # (no outputs: nothing is written)
    assert lib.rt_closest_points(None, p4.ctypes.data, 4, inf, 0, None) == rt.api.RT_E_INVALID
    with pytest.raises(ValueError):
        host.closest_points(p.astype(np.float64))
    with pytest.raises(ValueError):
        host.closest_points(p, outputs=("hit", "colour"))
    mem = _DeviceBytes(65 * 16 + 1024)
    points, out = mem.ptr.value, mem.ptr.value + 65 * 16
    assert lib.rt_closest_points_device(host._h, points + 4, 64, inf, 0, None, None) == rt.api.RT_E_INVALID
    arrays = rt.api._HitArrays(None, out + 2, None, None, None, None)
    assert lib.rt_closest_points_device(host._h, points, 64, inf, 0, C.byref(arrays), None) == rt.api.RT_E_INVALID
    arrays = rt.api._HitArrays(out + 1, out + 4, None, None, None, None)  # (the flags are bytes: any address)
    assert lib.rt_closest_points_device(host._h, points, 64, inf, 0, C.byref(arrays), None) == 0
    # the walk's switches are the A/B build's
    assert lib.rt_debug_set_nearest_walk(host._h, 0) == 0
    assert lib.rt_debug_set_nearest_walk(host._h, 2) == rt.api.RT_E_STATE
    assert host.last_nearest_counts() == (0, 0)
    host.close()
    mem.free()
    ring = rt.FrameRing(rt.Options.defaults(width=32, height=32, ao_num_samples=3), hosts=2)
    ring.set_calibration(False)
    ring.upload_scene(scene)
    with pytest.raises(rt.RtError) as e:
        ring.host(0).closest_points(p)
    assert e.value.code == rt.api.RT_E_STATE
    ring.close()
    import torch  # (CPU tensors: the checks come before any device work)

    t = torch.zeros((65, 4), dtype=torch.float32)
    with pytest.raises(ValueError):
        host.closest_points(t[:, :3])  # not contiguous
    with pytest.raises(ValueError):
        host.closest_points(t.double())


def test_walk_switches_change_no_bit(rt_knobs, scene_for_knobs):
    """The A/B build's switches -- no starting bound, no pruning, the counted kernel -- give the product's words, and the
    counters say what each is worth."""
    rt = rt_knobs
    scene, _ = scene_for_knobs("blob", "sah")
    host = new_host(rt)
    host.upload_scene(scene)
    points = mixed_points(scene.vertices, scene.faces.reshape(-1, 3), 1500, 400, 50, 120)
    want = orc_n.closest_points(scene.sorted_faces, scene.vertices, scene.vnormals, points)
    counts = {}
    for name, kw in (("full", {}), ("no_start", {"no_start": True}), ("no_prune", {"no_prune": True})):
        host.set_nearest_walk(count=True, **kw)
        orc_n.assert_same(host.closest_points(points), want, name)
        counts[name] = host.last_nearest_counts()
    host.set_nearest_walk()
    orc_n.assert_same(host.closest_points(points), want, "product form")
    leaves = len(scene.sorted_faces) // 3
    assert counts["no_prune"][1] == leaves * len(points)
    assert counts["full"][1] < counts["no_start"][1] < counts["no_prune"][1], counts
    host.close()


def test_queries_leave_frames_alone(rt, oracle, scene_for):
    scene, arrays = scene_for("bunny", "longest")
    opt = rt.Options.defaults(width=96, height=64, n_super_samples=4, ao_num_samples=3)
    host = rt.Host(opt, 0)
    host.upload_scene(scene)
    host.render()
    before = host.download()
    stats = host.stats()
    points = cases.in_box(scene.vertices, 20000, 130)
    first = host.closest_points(points)
    assert host.stats() == stats
    host.render()
    assert np.array_equal(bits(host.download()), bits(before))
    host.render_async()  # a frame left in flight while a query runs
    during = host.closest_points(points, sort=False)
    host.sync()
    assert np.array_equal(bits(host.download()), bits(before))
    assert host.stats() == stats
    orc_n.assert_same(during, first, "beside a frame")
    assert host.last_query_ms > 0.0
    host.close()


def test_torch_path_equals_numpy_path():
    """A device tensor in and device tensors out on a non-default stream == the numpy path (tests/nearest_torch_driver.py, a
    child process that brings torch's runtime up before it loads the library)."""
    driver = os.path.join(os.path.dirname(os.path.abspath(__file__)), "nearest_torch_driver.py")
    r = subprocess.run([sys.executable, driver], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "NEAREST_TORCH_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
