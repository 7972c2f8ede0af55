"""GPU: every size threshold of the builds, tables and lists crossed with a comparison behind it (DESIGN.md "Size
thresholds"; the shapes and the limits: tests/threshold_cases.py, held to their sides of the limits by
tests/test_thresholds_cpu.py).  Word for word throughout; no tolerance.

  A  device-side instance sets astride rocPRIM's single-block sort (1 024), astride the fused reductions (65 536
     instances: 256 partials), at RT_INSTANCES_MAX, and the refusal one past it -- the first onesweep size
  B  a device-side scene build past the merge limit of the sort (onesweep)
  C  the sign table past both limits for both key widths, and segments longer than a workgroup
  D  the slabs of the host form of the signed distance grid
  E  the hit list's scan past one turn of 1 024 blocks, and a views call past VIEWS_MAX_CHUNK"""
import ctypes as C

import numpy as np
import pytest

import instance_build_cases as ibc
import instance_cases as icases
import instance_nearest_cases as inc
import instance_nearest_oracle as ino
import instance_oracle as io
import instance_views_oracle as ivo
import layers_oracle as lo
import orc
import query_oracle as qo
import signed_cases as scases
import signed_oracle as orc_s
import threshold_cases as tc
from conftest import bits
from test_refit_gpu import make_host, same_bytes
from test_signed_gpu import grid_points, table_words

pytestmark = pytest.mark.gpu

EMPTY = np.zeros((0, 3, 4), np.float32)


def small_host(rt, scene=None, **over):
    host = rt.Host(rt.Options.defaults(width=64, height=48, n_super_samples=1, **over), 0)
    if scene is not None:
        host.upload_scene(scene)
    return host


class DeviceBytes:
    """Device memory of the test's own beside the library's (as tests/test_signed_gpu.py's _DeviceBytes), with the way back."""

    def __init__(self, size: int):
        self.hip, self.ptr, self.size = C.CDLL("libamdhip64.so"), C.c_void_p(), int(size)
        assert self.hip.hipMalloc(C.byref(self.ptr), C.c_size_t(self.size)) == 0
        assert self.hip.hipMemset(self.ptr, 0xA5, C.c_size_t(self.size)) == 0

    def at(self, offset: int) -> int:
        assert 0 <= offset < self.size
        return self.ptr.value + offset

    def read(self, offset: int, shape, dtype) -> np.ndarray:
        out = np.empty(shape, dtype)
        assert offset + out.nbytes <= self.size
        assert self.hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(self.ptr.value + offset), C.c_size_t(out.nbytes), 2) == 0
        return out

    def free(self):
        self.hip.hipFree(self.ptr)


# ---- A. device-side instance sets -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blob_host(rt, scene_for):
    scene, arrays = scene_for("blob", "longest")
    host = small_host(rt, scene)
    yield host, scene, arrays
    host.close()


def read_back(host) -> dict:
    plan = host.instances()
    plan["bounds"] = host.instance_bounds()
    return plan


def differing(a, b) -> int:
    return int((np.frombuffer(a.tobytes(), np.uint32) != np.frombuffer(b.tobytes(), np.uint32)).sum())


def assert_is_the_plan(got, want, fields, what):
    for f in fields:
        assert got[f].tobytes() == want[f].tobytes(), (what, f, differing(got[f], want[f]))


@pytest.mark.parametrize("n,place", [(n, place) for n in tc.INSTANCE_COUNTS for place in tc.special_places(n)])
def test_instance_set_astride_the_limits(rt, blob_host, n, place):
    """The set as the device holds it == rt.instance_plan_lbvh == the numpy restatement, every word.  1 024 | 1 025: the sort's
    single block | block sort and merge.  65 536 | 65 537: the reductions fused with all 256 partials | instance_reach_kernel
    and instance_root_kernel.  The copy that makes the root box and the set's reach lies in the first workgroup or in the
    last (at 65 537: index 65 536, alone in workgroup 256)."""
    host, _, arrays = blob_host
    W, _ = tc.instance_set(arrays, n, tc.special_places(n)[place])
    lo_, hi_ = icases.root_box(arrays)
    host.build_instances(W)
    got = read_back(host)
    host.build_instances(EMPTY)
    want = rt.instance_plan_lbvh(lo_, hi_, W)
    assert got["world_from_object"].tobytes() == W.tobytes(), (n, place)
    assert_is_the_plan(got, want, ("object_from_world", "nodes", "bounds"), (n, place, "planner"))
    restated = ibc.restated_plan(rt, lo_, hi_, W)
    assert_is_the_plan(got, restated, ("object_from_world", "nodes"), (n, place, "restatement"))
    ranks = got["nodes"]["leaf"][got["nodes"]["leaf"] != 0xFFFFFFFF]
    run = ranks[np.isin(ranks, np.arange(n - tc.RUN, n)) & (ranks != tc.special_places(n)[place])]
    assert np.array_equal(run, np.sort(run)) and len(run) >= tc.RUN - 1  # (equal keys: by instance index)


def test_instance_set_at_the_largest_size_and_the_refusal_past_it(rt, blob_host):
    """RT_INSTANCES_MAX = 2^20 instances: the largest set, the last size of the sort's merge path, 4 096 partials -- against
    the host planner alone (tests/test_thresholds_cpu.py holds the planner against the restatement at 65 537).  One more
    instance would be the first onesweep size: the library refuses it (include/rt_hip_instance_build.h), so an instance
    set never takes that path; the set before stays."""
    host, _, arrays = blob_host
    n = tc.INSTANCE_LARGEST
    W, _ = tc.instance_set(arrays, n, tc.INSTANCE_FUSED_LIMIT)
    host.build_instances(W)
    got = read_back(host)
    want = rt.instance_plan_lbvh(*icases.root_box(arrays), W)
    assert got["world_from_object"].tobytes() == W.tobytes()
    assert_is_the_plan(got, want, ("object_from_world", "nodes", "bounds"), "2^20")
    more = np.concatenate([W, W[:tc.INSTANCE_REFUSED - n]])
    assert len(more) == tc.INSTANCE_REFUSED == tc.SORT_MERGE_LIMIT + 1
    with pytest.raises(rt.RtError) as e:
        host.build_instances(more)
    assert e.value.code == rt.api.RT_E_INVALID and "RT_INSTANCES_MAX" in e.value.message
    with pytest.raises(rt.RtError) as e:
        host.set_instances(more)
    assert e.value.code == rt.api.RT_E_INVALID
    assert host.instances()["nodes"].tobytes() == got["nodes"].tobytes()
    host.build_instances(EMPTY)


def test_queries_through_65537_instances(rt, scene_for):
    """One closest-hit and one closest-point call of 2 000 queries through the un-fused set == the same calls on a host
    given the same transforms with set_instances (another tree over the same boxes); 256 of each against the CPU oracles.
    (`ties`, 13 leaves: the closest-point oracle is brute force over instances x leaves.)"""
    scene, arrays = scene_for("ties", "longest")
    n = tc.INSTANCE_FUSED_LIMIT + 1
    W, _ = tc.instance_set(arrays, n, tc.INSTANCE_FUSED_LIMIT)
    built_host, planned_host = small_host(rt, scene), small_host(rt, scene)
    try:
        built_host.build_instances(W)
        planned_host.set_instances(W)
        built = read_back(built_host)
        o, d = icases.rays(built["nodes"], 2000, seed=61)
        points = inc.in_top_box(built, 2000, 62)
        hits, near = built_host.trace_instances_closest(o, d, 1e5), built_host.instances_closest_points(points)
        other_hits, other_near = planned_host.trace_instances_closest(o, d, 1e5), planned_host.instances_closest_points(points)
        assert hits["hit"].any() and near["hit"].all()
        assert len(np.unique(hits["instance"][hits["hit"].astype(bool)])) > 100  # (not the covering copy alone)
        for f in hits:
            assert io.same_words(hits[f], other_hits[f]).all(), ("closest", f)
        for f in near:
            assert ino.same_words(near[f], other_near[f]).all(), ("closest points", f)
        io.assert_same({f: x[:256] for f, x in hits.items()}, io.closest(arrays, built, o[:256], d[:256], 1e5), "closest, 256")
        ino.assert_same({f: x[:256] for f, x in near.items()}, inc.Mesh(scene).oracle(built, points[:256]), "closest points, 256")
    finally:
        built_host.close()
        planned_host.close()


# ---- B. a scene build past the merge limit ----------------------------------------------------------------------------------
def test_scene_build_past_the_merge_limit(rt):
    """terrain(725) and 70 copies of one face, 1 051 320 faces: the (key, face) sort of the build runs onesweep.  The records
    of the built host == an upload of Scene.build_lbvh's arrays (tests/test_thresholds_cpu.py holds build_lbvh against the
    numpy restatement at terrain(200)); 2 000 rays against the query oracle over the CPU-built scene."""
    v, f = tc.big_terrain()
    assert len(f) == tc.TERRAIN_FACES + tc.TERRAIN_COPIES == 1051320 and tc.TERRAIN_FACES == 1051250 > tc.SORT_MERGE_LIMIT
    scene = rt.Scene.from_arrays(v, f).build_lbvh()
    host, _ = make_host(rt)
    fresh, _ = make_host(rt, scene)
    try:
        host.build_scene(v, f, scene.vnormals)
        got, want = host.records(), fresh.records()
        same_bytes(got, want, ("tris", "shade"), "terrain")
        # the node words against the CPU build's own arrays (an upload lays its nodes out otherwise): skips, leaves in rank
        # order, and every box
        skip = got["nodes"]["skip"]
        assert np.array_equal(skip, scene.nodes)
        assert np.array_equal(got["nodes"]["leaf"], np.where(skip == 1, np.cumsum(skip == 1) - 1, 0xFFFFFFFF).astype(np.uint32))
        assert np.array_equal(bits(got["nodes"]["lo"]), bits(scene.aabbs[0::2, :3])) and np.array_equal(bits(got["nodes"]["hi"]), bits(scene.aabbs[1::2, :3]))
        assert np.array_equal(host.face_of_leaf(), scene.triangles)
        copies = np.flatnonzero(scene.triangles >= tc.TERRAIN_FACES)
        assert len(copies) == tc.TERRAIN_COPIES and np.array_equal(np.diff(scene.triangles[copies]), np.ones(tc.TERRAIN_COPIES - 1, np.uint32))
        arrays = orc.SceneArrays.from_scene(scene)
        o4, d4 = tc.terrain_rays(v, 2000, 41)
        closest = host.trace_closest(o4, d4)
        oracle = qo.closest(arrays, o4, d4, 100000.0)
        assert oracle["hit"].mean() > 0.5 and not oracle["hit"].all()
        for name in rt.api.QUERY_OUTPUTS:
            ok = qo.same_words(closest[name], oracle[name])
            assert ok.all(), (name, int((~ok).sum()), np.argwhere(~ok)[:5].tolist())
    finally:
        host.close()
        fresh.close()


# ---- C. the sign table ------------------------------------------------------------------------------------------------------
_SIGN_MESHES = {}


def sign_mesh(name):
    if name not in _SIGN_MESHES:
        _SIGN_MESHES[name] = tc.sign_meshes()[name][0]()
    return _SIGN_MESHES[name]


@pytest.mark.parametrize("mesh", list(tc.sign_meshes()))
def test_sign_table_past_the_limits(rt, mesh):
    """host.sign_table() == signed_oracle.table under both CPU builders, after update_vertices to a sheared copy (the sums
    made again from the kept incidence) and after build_scene.  The corner sorts: 84 corners (one block), 2 016 (block sort
    and merge), 1 080 000 (onesweep, 32-bit vertex keys and 64-bit edge keys); segments of 400 (star_200's apexes) and of
    300 (the book's edge and its two vertices) under one thread of sign_sum_kernel each."""
    v, f = sign_mesh(mesh)
    moved = scases.sheared(v)
    for method in (0, 1):
        scene = rt.Scene.from_arrays(v, f).build_bvh(method)
        host = small_host(rt, scene)
        try:
            host.prepare_signed_distance()
            assert host.last_sign_build_ms() > 0.0
            assert orc_s.same_words(table_words(host), orc_s.table(scene.sorted_faces, scene.vertices)).all(), (mesh, method, "upload")
            host.update_vertices(moved)
            assert orc_s.same_words(table_words(host), orc_s.table(scene.sorted_faces, moved)).all(), (mesh, method, "updated")
            if method == 1:
                host.build_scene(scene.vertices, f, scene.vnormals)
                leaf_faces = f[host.face_of_leaf()].reshape(-1)
                assert orc_s.same_words(table_words(host), orc_s.table(leaf_faces, scene.vertices)).all(), (mesh, "built")
                host.update_vertices(moved)
                assert orc_s.same_words(table_words(host), orc_s.table(leaf_faces, moved)).all(), (mesh, "built, then updated")
        finally:
            host.close()


@pytest.mark.parametrize("mesh", list(tc.sign_meshes()))
def test_signed_distance_on_the_threshold_meshes(rt, mesh):
    """512 points (256 on the large torus: the oracle is brute force) == signed_oracle.signed_distance, every output."""
    _, _, count, features = tc.sign_meshes()[mesh]
    v, f = sign_mesh(mesh)
    scene = rt.Scene.from_arrays(v, f).build_bvh(1)
    points, _ = tc.signed_points(v, f, count, tc.SIGN_POINT_SEED, features)
    host = small_host(rt, scene)
    try:
        got = host.signed_distance(points)
        want = orc_s.signed_distance(scene.sorted_faces, scene.vertices, scene.vnormals, points)
        orc_s.assert_same(got, want, mesh)
        found = got["hit"].astype(bool)
        assert (got["distance"][found] < 0).any() and (got["distance"][found] > 0).any() and not found.all()
    finally:
        host.close()


# ---- D. the slabs of the grid form -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def star_host(rt):
    v, f = scases.star()
    scene = rt.Scene.from_arrays(v, f).build_bvh(0)
    host = small_host(rt, scene)
    yield host, scene
    host.close()


def device_grid(rt, host, origin, spacing, dims, leaf: bool):
    """The device form over the whole grid in ONE launch, into memory of the test's own."""
    voxels = int(dims[0]) * int(dims[1]) * int(dims[2])
    mem = DeviceBytes(voxels * 4 * (2 if leaf else 1))
    try:
        o, s, d = np.float32(origin), np.float32(spacing), np.array(dims, np.uint32)
        rc = rt.load_library().rt_signed_distance_grid_device(host._h, o.ctypes.data, s.ctypes.data, d.ctypes.data, float("inf"), mem.at(0),
                                                              mem.at(voxels * 4) if leaf else None, None)
        assert rc == 0
        host.sync()
        shape = (int(dims[2]), int(dims[1]), int(dims[0]))
        return mem.read(0, shape, np.float32), (mem.read(voxels * 4, shape, np.uint32) if leaf else None)
    finally:
        mem.free()


def test_grid_slabs_with_a_seam_inside_a_brick(rt, star_host):
    """(1024, 1639, 11): slabs of 9 and 2 slices -- the first ends inside a 4 x 4 x 4 brick, the second starts at z_first = 9
    and writes at an offset of 9 slices.  The host form == the device form over the whole grid in one launch == the point
    form at every voxel of slices 0, 8, 9 and 10."""
    host, scene = star_host
    dims = tc.GRID_SEAM
    assert tc.slabs(dims) == [(0, 9), (9, 2)]
    origin, spacing = tc.grid_over(scene.vertices, dims)
    assert not any(tc.is_power_of_two(x) for x in spacing)
    got, leaf = host.signed_distance_grid(origin, spacing, dims, leaf=True)
    whole, whole_leaf = device_grid(rt, host, origin, spacing, dims, True)
    assert got.shape == dims[::-1] == whole.shape
    for k in range(dims[2]):  # (slice by slice: a message that names the slab)
        assert orc_s.same_words(got[k], whole[k]).all() and np.array_equal(leaf[k], whole_leaf[k]), ("slice", k)
    assert (got < 0).any() and (got > 0).any()
    slice_ = dims[0] * dims[1]
    points = grid_points(origin, spacing, dims)
    for k in (0, 8, 9, 10):
        want = host.signed_distance(points[k * slice_:(k + 1) * slice_], outputs=("distance", "leaf"), sort=False)
        assert orc_s.same_words(got[k].reshape(-1), want["distance"]).all(), ("point form, slice", k)
        assert np.array_equal(leaf[k].reshape(-1), want["leaf"]), ("point form, slice", k)


@pytest.mark.parametrize("dims", [tc.GRID_THIN, tc.GRID_WIDE], ids=["thin", "wide"])
def test_grid_slabs_at_the_extremes(rt, star_host, dims):
    """(4, 4, 2^20 + 3): a slice of 16 voxels, slabs of 2^20 and 3 slices.  (4097, 4097, 2): a slice larger than a slab, one
    slice a slab.  The host form == the device form in one launch."""
    host, scene = star_host
    assert tc.slabs(dims) == ([(0, 1 << 20), (1 << 20, 3)] if dims == tc.GRID_THIN else [(0, 1), (1, 1)])
    origin, spacing = tc.grid_over(scene.vertices, dims)
    got, leaf = host.signed_distance_grid(origin, spacing, dims, leaf=True)
    whole, whole_leaf = device_grid(rt, host, origin, spacing, dims, True)
    assert orc_s.same_words(got, whole).all() and np.array_equal(leaf, whole_leaf)
    last = got[tc.slabs(dims)[-1][0]:]  # (above the star: outside)
    assert np.isfinite(got).all() and (last > 0).all() and not orc_s.same_words(got[0], got[-1]).all()


# ---- E. the hit list and the views chunk ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blob16(rt, scene_for):
    """The blob at 1 / 16 of its size (tests/test_geometry_cpu.py's `blob16`: a power of two, exact)."""
    base, _ = scene_for("blob", "longest")
    scene = rt.Scene.from_arrays(base.vertices[:, :3] / np.float32(16.0), base.faces.reshape(-1, 3)).build_bvh(0)
    return scene, orc.SceneArrays.from_scene(scene)


def view_host(rt, scene, size):
    opt = rt.Options.defaults(ao_num_samples=1, **size)
    host = rt.Host(opt, 0)
    host.upload_scene(scene)
    return host, opt


def assert_layers(got, want, names, what):
    for f in names:
        ok = lo.same_words(got[f], want[f])
        assert ok.all(), (what, f, int((~ok).sum()), np.argwhere(~ok)[:5].tolist())


def test_one_view_past_one_turn_of_the_scan(rt, blob16):
    """1100 x 960 sub-pixels with the ambient-occlusion step: 1 032 blocks of the hit list's counts, 8 of them in the second
    turn of views_scan_sums_kernel, behind the carry; the pose fills the image, so those blocks hold hits."""
    scene, arrays = blob16
    assert tc.scan_blocks(tc.ONE_VIEW) == 1032 > tc.VIEWS_SUMS
    host, opt = view_host(rt, scene, tc.ONE_VIEW)
    try:
        pose = tc.close_pose(rt)
        got = host.render_views([pose], ("hit", "ao", "value", "image"))
        assert host.last_views() == {"views": 1, "chunks": 1, "ao_points": int(got["hit"].sum())}
    finally:
        host.close()
    want = lo.render(orc.params_from_options(opt), arrays, pose)
    beyond = want["hit"].reshape(-1)[tc.VIEWS_TURN:]
    assert want["hit"].mean() > 0.9 and beyond.mean() > 0.9 and (want["ao"].reshape(-1)[tc.VIEWS_TURN:] < 1).any()
    assert_layers({f: got[f][0] for f in ("hit", "ao", "value")}, want, ("hit", "ao", "value"), "one view")
    assert np.array_equal(got["image"][0], rt.resize_cpu(opt, want["value"]))


def test_many_views_past_one_turn_of_the_scan(rt, blob16):
    """78 views of 37 x 23 at 4 x 4 supersamples (n_super_samples = 16): ONE chunk of 1 062 048 sub-pixels, 1 038 blocks.  View 75 looks away: its blocks
    are empty, a run of zero counts right before the carry (block 1 024 lies in view 77).  Every view against the oracle."""
    scene, arrays = blob16
    assert tc.sub_pixels(tc.MANY_VIEWS, tc.MANY_VIEWS_COUNT) == 1062048 and tc.scan_blocks(tc.MANY_VIEWS, tc.MANY_VIEWS_COUNT) == 1038
    host, opt = view_host(rt, scene, tc.MANY_VIEWS)
    poses = tc.orbit_poses(rt, tc.MANY_VIEWS_COUNT, tc.MANY_VIEWS_AWAY)
    try:
        got = host.render_views(poses, rt.VIEW_OUTPUTS)
        assert host.last_views() == {"views": tc.MANY_VIEWS_COUNT, "chunks": 1, "ao_points": int(got["hit"].sum())}
    finally:
        host.close()
    params = orc.params_from_options(opt)
    for v, pose in enumerate(poses):
        want = lo.render(params, arrays, pose)
        assert want["hit"].any() != (v == tc.MANY_VIEWS_AWAY), v
        assert_layers({f: got[f][v] for f in lo.NAMES}, want, lo.NAMES, ("view", v))
        assert np.array_equal(got["image"][v], rt.resize_cpu(opt, want["value"])), v
    assert (got["ao"][tc.MANY_VIEWS_COUNT - 1] < 1).any()  # (occlusion found behind the carry)


def test_instanced_view_past_one_turn_of_the_scan(rt, blob16):
    """The instanced views share the list: three copies, one view of 1100 x 960, against the composed oracle."""
    scene, arrays = blob16
    host, opt = view_host(rt, scene, tc.ONE_VIEW)
    try:
        host.set_instances(icases.many(arrays, 3, seed=3))
        plan = host.instances()
        pose = ivo.cameras(rt, plan)[0]
        got = host.render_instance_views([pose], ivo.LAYERS + ("image",))
        assert host.last_views() == {"views": 1, "chunks": 1, "ao_points": int(got["hit"].sum())}
    finally:
        host.close()
    want = ivo.view(orc.params_from_options(opt), arrays, plan, pose)
    assert want["hit"].reshape(-1)[tc.VIEWS_TURN:].sum() > 100 and (want["ao"].reshape(-1)[tc.VIEWS_TURN:] < 1).any()
    ivo.assert_layers({f: got[f][0] for f in ivo.LAYERS}, want, ivo.LAYERS, "instanced view")
    assert np.array_equal(got["image"][0], rt.resize_cpu(opt, want["value"]))


def device_views(rt, host, poses, names, per_view: int):
    """rt_render_views_device into memory of the test's own: ONE call, whose own loop cuts the chunks."""
    layout = {"hit": (np.uint8, 1), "distance": (np.float32, 1), "ao": (np.float32, 1)}
    views, offsets, at = len(poses), {}, 0
    for name in names:
        offsets[name] = at
        at += (views * per_view * np.dtype(layout[name][0]).itemsize + 255) // 256 * 256
    mem = DeviceBytes(at)
    try:
        fields = ("hit", "distance", "leaf", "barycentric", "position", "normal", "direction", "shade", "ao", "value")
        layers = rt.api._LayerArrays(*[mem.at(offsets[f]) if f in offsets else None for f in fields])
        arrays = rt.api._ViewArrays(layers, None)
        assert rt.load_library().rt_render_views_device(host._h, poses.ctypes.data, views, C.byref(arrays), None) == 0
        host.sync()
        return {name: mem.read(offsets[name], (views, per_view), layout[name][0]) for name in names}
    finally:
        mem.free()


def test_more_views_than_one_chunk_takes(rt, blob16):
    """65 537 views of 2 x 2 with `hit`, `distance` and `ao`: two chunks, VIEWS_MAX_CHUNK = 65 535 and 2, without the debug
    knob -- == the same call in chunks of 4 096, == the device form (one call, the chunk loop of RayQueries::viewsCall; the
    host form stages chunk by chunk and calls it once for each), and 64 views of both chunks, 65 534 .. 65 536 among them,
    against the oracle."""
    scene, arrays = blob16
    host, opt = view_host(rt, scene, tc.TINY_VIEW)
    names = ("hit", "distance", "ao")
    poses = tc.tiny_poses(tc.TINY_VIEWS_COUNT, tc.TINY_RADIUS)
    try:
        got = host.render_views(poses, names)
        done = host.last_views()
        assert done == {"views": tc.TINY_VIEWS_COUNT, "chunks": 2, "ao_points": int(got["hit"].sum())}
        on_device = device_views(rt, host, poses, names, 4)
        assert host.last_views() == done
        host.set_views_chunk(4096)
        again = host.render_views(poses, names)
        assert host.last_views()["chunks"] == (tc.TINY_VIEWS_COUNT + 4095) // 4096 == 17
    finally:
        host.close()
    for f in names:
        assert lo.same_words(again[f], got[f]).all(), ("chunks of 4096", f)
        assert lo.same_words(on_device[f].reshape(got[f].shape), got[f]).all(), ("device form", f)
    params = orc.params_from_options(opt)
    checked = tc.checked_views()
    assert len(checked) == tc.TINY_VIEWS_CHECKED and {tc.VIEWS_MAX_CHUNK - 1, tc.VIEWS_MAX_CHUNK, tc.VIEWS_MAX_CHUNK + 1} <= set(checked.tolist())
    hits = 0
    for v in checked:
        want = lo.render(params, arrays, poses[v])
        assert_layers({f: got[f][v] for f in names}, want, names, ("view", int(v)))
        hits += int(want["hit"].sum())
    assert 0 < hits < 4 * len(checked) and got["hit"][tc.VIEWS_MAX_CHUNK:].any() and (got["ao"] < 1).any()
