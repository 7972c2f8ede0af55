"""GPU: signed distance queries (include/rt_hip_signed.h) against the brute-force CPU oracle of tests/signed_oracle.c -- the
sign table and every output, word for word --, the grid form against the point form, and the closest-point queries of the
same host.  The star has 28 leaves and the torus 576: the smallest shapes where a sort segment, a brick edge or a reflex
feature can go wrong."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import nearest_cases as ncases
import signed_cases as cases
import signed_oracle as orc_s

pytestmark = pytest.mark.gpu

SORT_MIN = 16384  # RT_QUERY_SORT_MIN
MESHES = {"torus": cases.torus, "star": cases.star}
GRIDS = ((9, 6, 5), (4, 4, 4), (1, 1, 1))


def new_host(rt):
    return rt.Host(rt.Options.defaults(width=64, height=48, n_super_samples=1), 0)


def scene_of(rt, mesh, method=0, reverse=False):
    v, f = MESHES[mesh]()
    return rt.Scene.from_arrays(v, cases.reversed_faces(f) if reverse else f).build_bvh(method)


def table_words(host):
    t = host.sign_table()
    return np.concatenate([t["edge"], t["vertex"]], axis=1)  # (leaves, 6, 4): the oracle's layout


def mixed_points(scene, n_box, seed):
    v, f = scene.vertices, scene.faces.reshape(-1, 3)
    return np.concatenate([ncases.in_box(v, n_box, seed), ncases.on_surface(v, f, 300, seed + 1), ncases.far_away(v, 50, seed + 2),
                           cases.per_feature(v, f)[0], ncases.odd_points(v)])


@pytest.mark.parametrize("mesh", ["torus", "star"])
def test_sign_table_equals_the_cpu_table(rt, mesh):
    """After an upload under both builders, after update_vertices to a sheared copy (the incidence is reused), and after
    build_scene (the CPU table in face_of_leaf order)."""
    for method in (0, 1):
        scene = scene_of(rt, mesh, method)
        host = new_host(rt)
        host.upload_scene(scene)
        assert host.last_sign_build_ms() == 0.0
        host.prepare_signed_distance()
        assert host.last_sign_build_ms() > 0.0
        assert orc_s.same_words(table_words(host), orc_s.table(scene.sorted_faces, scene.vertices)).all(), (mesh, method, "upload")
        moved = cases.sheared(scene.vertices)
        host.update_vertices(moved)
        assert orc_s.same_words(table_words(host), orc_s.table(scene.sorted_faces, moved)).all(), (mesh, method, "updated")
        v, f = scene.vertices, scene.faces.reshape(-1, 3)
        host.build_scene(v, f, scene.vnormals)
        leaf_faces = f[host.face_of_leaf()].reshape(-1)
        assert orc_s.same_words(table_words(host), orc_s.table(leaf_faces, v)).all(), (mesh, method, "built")
        host.update_vertices(moved)
        assert orc_s.same_words(table_words(host), orc_s.table(leaf_faces, moved)).all(), (mesh, method, "built, then updated")
        host.close()


@pytest.mark.parametrize("mesh,reverse", [("torus", False), ("star", False), ("star", True)])
def test_signed_distance_equals_the_oracle(rt, mesh, reverse):
    """Every output, every radius, odd points and radii; the record is closest_points' but for the sign of the distance."""
    scene = scene_of(rt, mesh, 1, reverse)
    host = new_host(rt)
    host.upload_scene(scene)
    v, n = scene.vertices, scene.vnormals
    points = mixed_points(scene, 1500, 50)
    table = orc_s.table(scene.sorted_faces, v)
    for radius in ncases.RADII + ncases.ODD_RADII:
        got = host.signed_distance(points, radius)
        orc_s.assert_same(got, orc_s.signed_distance(scene.sorted_faces, v, n, points, radius, sign_table=table), (mesh, reverse, radius))
        plain = host.closest_points(points, radius)
        for k in plain:
            mine = np.abs(got[k]) if k == "distance" else got[k]
            assert orc_s.same_words(mine, plain[k]).all(), (mesh, radius, k)
    free = host.signed_distance(points)
    found = free["hit"].astype(bool)
    assert (free["distance"][found] < 0).any() and (free["distance"][found] > 0).any()
    assert np.isposinf(free["distance"][~found]).all() and (free["feature"][~found] == orc_s.NO_FEATURE).all()
    assert set(np.unique(free["feature"][found])) == {0, 1, 2, 3, 4, 5, 6}
    host.close()


def test_sorted_unsorted_and_output_subsets(rt):
    scene = scene_of(rt, "torus", 0)
    host = new_host(rt)
    host.upload_scene(scene)
    one = mixed_points(scene, 2000, 80)
    points = np.concatenate([one] * (SORT_MIN // len(one) + 1))
    assert len(points) >= SORT_MIN
    want = orc_s.signed_distance(scene.sorted_faces, scene.vertices, scene.vnormals, one, 0.3)
    want = {k: np.concatenate([x] * (SORT_MIN // len(one) + 1)) for k, x in want.items()}
    for sort in (True, False):
        orc_s.assert_same(host.signed_distance(points, 0.3, sort=sort), want, ("sort", sort))
        for only in orc_s.OUTPUTS:
            got = host.signed_distance(points, 0.3, outputs=(only,), sort=sort)
            assert set(got) == {only}
            orc_s.assert_same(got, want, ("only", only, sort))
        names = tuple(k for k in orc_s.OUTPUTS if k not in ("distance", "pseudonormal"))
        orc_s.assert_same(host.signed_distance(points, 0.3, outputs=names, sort=sort), want, ("without", sort))
    assert host.last_query_ms > 0.0
    for n in (0, 1, 63, 64, 65):
        got = host.signed_distance(one[:n])
        assert got["distance"].shape == (n,) and got["pseudonormal"].shape == (n, 4)
        orc_s.assert_same(got, orc_s.signed_distance(scene.sorted_faces, scene.vertices, scene.vnormals, one[:n]), ("batch", n))
    host.close()


def grid_points(origin, spacing, shape):
    """The voxels' points as the header states them, in the output's order: [k, j, i] at origin + float32(i) * spacing."""
    o, s = np.float32(origin), np.float32(spacing)
    x = o[0] + np.arange(shape[0], dtype=np.float32) * s[0]
    y = o[1] + np.arange(shape[1], dtype=np.float32) * s[1]
    z = o[2] + np.arange(shape[2], dtype=np.float32) * s[2]
    assert x.dtype == np.float32
    zz, yy, xx = np.meshgrid(z, y, x, indexing="ij")
    return np.stack([xx, yy, zz], axis=-1).reshape(-1, 3).astype(np.float32)


@pytest.mark.parametrize("mesh", ["torus", "star"])
def test_grid_equals_the_point_form(rt, mesh):
    """Partial bricks on all three axes, one whole brick, one voxel; a spacing that puts voxels exactly on vertices."""
    scene = scene_of(rt, mesh, 0)
    host = new_host(rt)
    host.upload_scene(scene)
    on_vertices = 0
    # the first grid's voxel (5, 5, 2) IS vertex 0 -- (1.4, 0, 0) of the torus, the star's tip (1, 0, 0) --: the spacing is a
    # power of two, so that the origin and the way back from it are exact
    corner = scene.vertices[0, :3].astype(np.float32)
    through_vertex = corner - np.float32([5, 5, 2]) * np.float32([0.5, 0.25, 0.25])
    for shape in GRIDS:
        for origin, spacing in ((through_vertex, np.float32([0.5, 0.25, 0.25])), (np.float32([-1.3, -1.1, -0.61]), np.float32([0.31, 0.47, 0.33]))):
            points = grid_points(origin, spacing, shape)
            if origin is through_vertex and shape == GRIDS[0]:
                assert (points == corner).all(axis=1).sum() == 1
            for radius in (np.inf, 0.3):
                want = host.signed_distance(points, radius, sort=False)
                got, leaf = host.signed_distance_grid(origin, spacing, shape, radius, leaf=True)
                assert got.shape == shape[::-1] and got.dtype == np.float32 and leaf.dtype == np.uint32
                assert orc_s.same_words(got.reshape(-1), want["distance"]).all(), (mesh, shape, radius)
                assert orc_s.same_words(leaf.reshape(-1), want["leaf"]).all(), (mesh, shape, radius)
                alone = host.signed_distance_grid(origin, spacing, shape, radius)
                assert orc_s.same_words(alone, got).all()
            on_vertices += int((host.signed_distance(points)["distance"] == 0).sum())
            assert host.last_query_ms > 0.0
    assert on_vertices > 0, "no voxel of these grids lies on the surface"
    # the oracle on one grid, beside the point form
    points = grid_points(through_vertex, np.float32([0.5, 0.25, 0.25]), GRIDS[0])
    want = orc_s.signed_distance(scene.sorted_faces, scene.vertices, scene.vnormals, points)
    got = host.signed_distance_grid(through_vertex, np.float32([0.5, 0.25, 0.25]), GRIDS[0])
    assert orc_s.same_words(got.reshape(-1), want["distance"]).all()
    assert (got < 0).any() and (got > 0).any()
    host.close()


def test_an_update_invalidates_the_table(rt):
    """A signed query, update_vertices, a signed query: the answers of a fresh host on the moved mesh."""
    scene = scene_of(rt, "star", 0)
    moved = cases.sheared(scene.vertices)
    points = mixed_points(scene, 1000, 90)
    host = new_host(rt)
    host.upload_scene(scene)
    before = host.signed_distance(points)
    built = host.last_sign_build_ms()
    host.update_vertices(moved)
    after = host.signed_distance(points)
    assert host.last_sign_build_ms() > 0.0 and built > 0.0
    fresh = new_host(rt)
    fresh.upload_scene(scene.refit(moved))
    want = fresh.signed_distance(points)
    for k in ("hit", "distance", "leaf", "barycentric", "position", "feature", "pseudonormal"):  # (the shading normals stay the upload's)
        assert orc_s.same_words(after[k], want[k]).all(), k
    assert not orc_s.same_words(after["distance"], before["distance"]).all()
    grid = host.signed_distance_grid([-1.5, -1.5, -0.5], 0.3, (9, 9, 4))
    assert orc_s.same_words(grid, fresh.signed_distance_grid([-1.5, -1.5, -0.5], 0.3, (9, 9, 4))).all()
    host.close()
    fresh.close()


class _DeviceBytes:
    def __init__(self, size):
        self.hip, self.ptr = C.CDLL("libamdhip64.so"), C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.ptr), C.c_size_t(size)) == 0
        assert self.hip.hipMemset(self.ptr, 0, C.c_size_t(size)) == 0

    def free(self):
        self.hip.hipFree(self.ptr)


def test_error_paths(rt):
    lib = rt.load_library()
    scene = scene_of(rt, "star", 0)
    host = new_host(rt)
    p = np.zeros((4, 3), np.float32)
    state, invalid = rt.api.RT_E_STATE, rt.api.RT_E_INVALID
    for call in (lambda: host.signed_distance(p), lambda: host.signed_distance_grid([0, 0, 0], 0.1, (2, 2, 2)), host.prepare_signed_distance,
                 host.sign_table):
        with pytest.raises(rt.RtError) as e:
            call()
        assert e.value.code == state
    assert host.last_sign_build_ms() == 0.0
    host.upload_scene(scene)
    inf = float("inf")
    assert lib.rt_signed_distance(host._h, None, 4, inf, 0, None) == invalid
    assert lib.rt_signed_distance(host._h, None, 0, inf, 0, None) == 0
    p4 = np.zeros((4, 4), np.float32)
    assert lib.rt_signed_distance(host._h, p4.ctypes.data, (1 << 27) + 1, inf, 0, None) == invalid
    assert lib.rt_signed_distance(host._h, p4.ctypes.data, 4, inf, 0, None) == 0  # (no outputs: nothing is written)
    assert lib.rt_signed_distance(None, p4.ctypes.data, 4, inf, 0, None) == invalid
    with pytest.raises(ValueError):
        host.signed_distance(p, outputs=("hit", "colour"))
    for spacing in (0.0, -0.1, np.nan, np.inf, (0.1, 0.0, 0.1)):
        with pytest.raises(rt.RtError) as e:
            host.signed_distance_grid([0, 0, 0], spacing, (2, 2, 2))
        assert e.value.code == invalid, spacing
    for shape in ((0, 2, 2), (2, 0, 2), (2, 2, 0), (1 << 16, 1 << 16, 2)):
        with pytest.raises(rt.RtError) as e:
            host.signed_distance_grid([0, 0, 0], 0.1, shape)
        assert e.value.code == invalid, shape
    origin, spacing, dims = np.zeros(3, np.float32), np.full(3, 0.1, np.float32), np.array([2, 2, 2], np.uint32)
    assert lib.rt_signed_distance_grid(host._h, None, spacing.ctypes.data, dims.ctypes.data, inf, None, None) == invalid
    assert lib.rt_signed_distance_grid(host._h, origin.ctypes.data, spacing.ctypes.data, dims.ctypes.data, inf, None, None) == 0
    mem = _DeviceBytes(65 * 16 + 4096)
    points, out = mem.ptr.value, mem.ptr.value + 65 * 16
    assert lib.rt_signed_distance_device(host._h, points + 4, 64, inf, 0, None, None) == invalid
    arrays = rt.api._SignedArrays(rt.api._HitArrays(None, out + 2, None, None, None, None), None, None)
    assert lib.rt_signed_distance_device(host._h, points, 64, inf, 0, C.byref(arrays), None) == invalid
    arrays = rt.api._SignedArrays(rt.api._HitArrays(None, out, None, None, None, None), out + 1, out + 1024 + 8)
    assert lib.rt_signed_distance_device(host._h, points, 64, inf, 0, C.byref(arrays), None) == invalid  # (float4: 16 bytes)
    arrays = rt.api._SignedArrays(rt.api._HitArrays(out + 1, out + 4, None, None, None, None), out + 513, out + 1024)
    assert lib.rt_signed_distance_device(host._h, points, 64, inf, 0, C.byref(arrays), None) == 0
    assert lib.rt_signed_distance_grid_device(host._h, origin.ctypes.data, spacing.ctypes.data, dims.ctypes.data, inf, out + 2, None, None) == invalid
    assert lib.rt_signed_distance_grid_device(host._h, origin.ctypes.data, spacing.ctypes.data, dims.ctypes.data, inf, out, out + 6, None) == invalid
    assert lib.rt_signed_distance_grid_device(host._h, origin.ctypes.data, spacing.ctypes.data, dims.ctypes.data, inf, out, out + 64, None) == 0
    host.sync()
    host.close()
    mem.free()
    ring = rt.FrameRing(rt.Options.defaults(width=32, height=32, ao_num_samples=3), hosts=2)
    ring.set_calibration(False)
    ring.upload_scene(scene)
    for call in (lambda: ring.host(0).signed_distance(p), lambda: ring.host(0).signed_distance_grid([0, 0, 0], 0.1, (2, 2, 2)),
                 ring.host(0).prepare_signed_distance):
        with pytest.raises(rt.RtError) as e:
            call()
        assert e.value.code == state
    ring.close()


def test_open_and_degenerate_meshes(rt, scene_for):
    """blob, ties and single are open; ties has faces without area: the same rule, the oracle's words."""
    for mesh, bvh in (("blob", "sah"), ("ties", "longest"), ("single", "longest")):
        scene, _ = scene_for(mesh, bvh)
        host = new_host(rt)
        host.upload_scene(scene)
        assert orc_s.same_words(table_words(host), orc_s.table(scene.sorted_faces, scene.vertices)).all(), mesh
        points = np.concatenate([ncases.in_box(scene.vertices, 1500, 60), ncases.on_surface(scene.vertices, scene.faces.reshape(-1, 3), 300, 61)])
        orc_s.assert_same(host.signed_distance(points), orc_s.signed_distance(scene.sorted_faces, scene.vertices, scene.vnormals, points), mesh)
        host.close()


def test_torch_path_equals_numpy_path():
    """Device tensors in and out on a non-default stream == the numpy path (tests/signed_torch_driver.py, a child process that
    brings torch's runtime up before it loads the library)."""
    driver = os.path.join(os.path.dirname(os.path.abspath(__file__)), "signed_torch_driver.py")
    r = subprocess.run([sys.executable, driver], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "SIGNED_TORCH_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
