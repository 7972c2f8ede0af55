"""CPU: what tests/test_thresholds_gpu.py leans on (DESIGN.md "Size thresholds").  The limits of tests/threshold_cases.py
are the sources' own; every shape lies on the side of its limit that the GPU test claims; and the references the GPU tests
compare with are right at these sizes: the host planner of an instance set against the numpy restatement at 65 537,
Scene.build_lbvh against the numpy restatement at 80 000 faces, the sign oracle against the float64 pseudonormals and the
winding number on the meshes with a million corners and with segments of 400.  No GPU."""
import os
import re

import numpy as np
import pytest

import build_cases as bcs
import instance_build_cases as ibc
import instance_cases as icases
import instance_oracle as io
import instance_views_oracle as ivo
import layers_oracle as lo
import orc
import signed_cases as scases
import signed_oracle as orc_s
import signed_reference as sref
import threshold_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opencl_raytracer_amd", "csrc")


def source(*path) -> str:
    return open(os.path.join(*path)).read()


# ---- the limits -------------------------------------------------------------------------------------------------------------
def test_the_limits_are_the_sources_own():
    assert re.search(r"constexpr uint32_t BUILD_LANES = (\d+)u;", source(CSRC, "kernels", "build.hip.h")).group(1) == str(tc.BUILD_LANES)
    assert "constexpr uint32_t INSTANCE_FUSED_PARTIALS = BUILD_LANES;" in source(CSRC, "kernels", "instance_build.hip.h")
    assert tc.INSTANCE_FUSED_PARTIALS == tc.BUILD_LANES and tc.INSTANCE_FUSED_LIMIT == 65536
    assert re.search(r"#define RT_INSTANCES_MAX \(1u << (\d+)\)", source(ROOT, "include", "rt_hip_instances.h")).group(1) == "20"
    assert tc.INSTANCES_MAX == 1 << 20 == tc.SORT_MERGE_LIMIT
    views = source(CSRC, "kernels", "views.hip.h")
    assert f"constexpr uint32_t VIEWS_SCAN = {tc.VIEWS_SCAN}u, VIEWS_SUMS = {tc.VIEWS_SUMS}u;" in views
    queries = source(CSRC, "ray_query.cc")
    assert f"constexpr uint32_t VIEWS_MAX_CHUNK = {tc.VIEWS_MAX_CHUNK}u;" in queries
    assert "constexpr uint64_t SIGNED_GRID_CHUNK = (uint64_t) 1 << 24;" in queries and tc.SIGNED_GRID_CHUNK == 1 << 24
    # the sorts are rocPRIM's radix_sort_pairs, with its default configuration (the limits in threshold_cases.py are that one's)
    for name in ("build_sort.hip", "sign_sort.hip"):
        text = source(CSRC, name)
        assert "rocprim::radix_sort_pairs(" in text and "radix_sort_config" not in text, name
    assert "onesweep" in source(ROOT, "include", "rt_hip_instance_build.h")  # (the limit that keeps a set off that path is documented)


def test_every_shape_lies_on_its_side(rt):
    # A
    assert tc.INSTANCE_COUNTS == (1024, 1025, 65536, 65537)
    assert 1024 <= tc.SORT_SINGLE_BLOCK < 1025 and 65536 <= tc.INSTANCE_FUSED_LIMIT < 65537
    assert [tc.groups_of(n) for n in tc.INSTANCE_COUNTS] == [4, 5, 256, 257]
    assert tc.groups_of(65536) == tc.INSTANCE_FUSED_PARTIALS and tc.groups_of(65537) > tc.INSTANCE_FUSED_PARTIALS
    assert tc.INSTANCE_LARGEST == tc.INSTANCES_MAX <= tc.SORT_MERGE_LIMIT < tc.INSTANCE_REFUSED == 1048577 > tc.INSTANCES_MAX
    assert tc.RUN > tc.BUILD_LANES
    assert tc.special_places(65537) == {"first": 5, "last": 65536} and tc.special_places(1 << 20)["at_65536"] == 65536
    assert tc.special_places(65536)["last"] // tc.BUILD_LANES == 255 and tc.special_places(1025)["last"] // tc.BUILD_LANES == 4
    # B
    assert tc.TERRAIN_FACES == 1051250 > tc.SORT_MERGE_LIMIT >= 2 * (tc.TERRAIN - 1) ** 2
    assert 2 * tc.TERRAIN_RESTATED ** 2 == 80000
    # C: the corners of a mesh are the items of both sorts
    corners = {name: 3 * len(make()[1]) for name, (make, _, _, _) in tc.sign_meshes().items() if name != "torus_600x300"}
    corners["torus_600x300"] = 3 * 2 * 600 * 300
    assert corners == {"torus_600x300": 1080000, "torus_24x14": 2016, "star": 84, "star_200": 2400, "book": 900}
    assert corners["star"] <= tc.SORT_SINGLE_BLOCK < corners["torus_24x14"] <= tc.SORT_MERGE_LIMIT < corners["torus_600x300"]
    assert tc.segment_lengths(scases.star(points=200)[1]) == (400, 2) and 400 > tc.BUILD_LANES
    assert tc.segment_lengths(tc.book()[1]) == (tc.BOOK_PAGES, tc.BOOK_PAGES) and tc.BOOK_PAGES > tc.BUILD_LANES
    assert tc.segment_lengths(scases.star()[1]) == (14, 2)  # (the longest segments before this file)
    # D
    assert tc.GRID_SEAM[0] * tc.GRID_SEAM[1] == 1678336 and tc.SIGNED_GRID_CHUNK // 1678336 == 9 and 9 % tc.BRICK != 0
    assert tc.slabs(tc.GRID_SEAM) == [(0, 9), (9, 2)] and np.prod(tc.GRID_SEAM) == 18461696 > tc.SIGNED_GRID_CHUNK
    assert tc.slabs(tc.GRID_THIN) == [(0, 1 << 20), (1 << 20, 3)] and tc.GRID_THIN[2] == (1 << 24) // 16 + 3
    assert tc.GRID_WIDE[0] * tc.GRID_WIDE[1] > tc.SIGNED_GRID_CHUNK and tc.slabs(tc.GRID_WIDE) == [(0, 1), (1, 1)]
    assert tc.slabs((9, 6, 5)) == [(0, 5)]  # (the largest grid before this file: one slab)
    for dims in (tc.GRID_SEAM, tc.GRID_THIN, tc.GRID_WIDE):
        assert np.prod(dims, dtype=np.int64) <= 1 << 31
        origin, spacing = tc.grid_over(scases.star()[0], dims)
        assert not any(tc.is_power_of_two(x) for x in spacing), dims
    assert tc.is_power_of_two(0.25) and tc.is_power_of_two(2.0) and not tc.is_power_of_two(0.3)
    # E
    for size in (tc.ONE_VIEW, tc.MANY_VIEWS, tc.TINY_VIEW):  # (the library's own count: n_super_samples 16 is 4 x 4 a pixel)
        options = rt.Options.defaults(ao_num_samples=1, **size)
        assert options.total_width * options.total_height == tc.sub_pixels(size), size
    assert tc.sub_pixels(tc.ONE_VIEW) == 1056000 > tc.VIEWS_TURN == 1048576 and tc.scan_blocks(tc.ONE_VIEW) == 1032
    assert tc.sub_pixels(tc.MANY_VIEWS) == 13616 and tc.sub_pixels(tc.MANY_VIEWS, tc.MANY_VIEWS_COUNT) == 1062048 > tc.VIEWS_TURN
    first, last = tc.MANY_VIEWS_AWAY * 13616 // tc.VIEWS_SCAN, ((tc.MANY_VIEWS_AWAY + 1) * 13616 - 1) // tc.VIEWS_SCAN
    assert (first, last) == (997, 1010) and last < tc.VIEWS_SUMS  # (whole blocks 998 .. 1009 hold nothing: before the carry)
    assert tc.VIEWS_TURN // 13616 == 77 == tc.MANY_VIEWS_COUNT - 1
    assert tc.TINY_VIEWS_COUNT == 65537 > tc.VIEWS_MAX_CHUNK and -(-tc.TINY_VIEWS_COUNT // tc.VIEWS_MAX_CHUNK) == 2
    # (a chunk is as large as VIEWS_MAX_CHUNK only while its rays fit one query: 4 sub-pixels a view, few rays a point)
    host_options = rt.Options.defaults(ao_num_samples=1, **tc.TINY_VIEW)
    assert host_options.total_width * host_options.total_height == 4 and (1 << 27) // (4 * 512) >= tc.VIEWS_MAX_CHUNK
    checked = tc.checked_views()
    assert len(checked) == len(set(checked.tolist())) == 64 and checked.min() == 0 and checked.max() == 65536
    assert {65534, 65535, 65536} <= set(checked.tolist()) and (checked < 65535).sum() > 20 and np.array_equal(checked, np.sort(checked))


# ---- A ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blob(scene_for):
    return scene_for("blob", "longest")


@pytest.mark.parametrize("n,place", [(n, place) for n in (1025, 65537) for place in tc.special_places(n)])
def test_the_instance_sets_are_what_they_claim(rt, blob, n, place):
    """One copy has the largest reach and alone touches all six faces of the root box, where the case puts it; the run of
    equal keys is RUN long and crosses a workgroup; and the planner == the restatement at this size, which is what lets the
    GPU test of 2^20 instances lean on the planner alone."""
    _, arrays = blob
    at = tc.special_places(n)[place]
    W, side = tc.instance_set(arrays, n, at)
    assert W.shape == (n, 3, 4) and W.dtype == np.float32 and np.isfinite(W).all()
    reach = tc.reaches(arrays, W)
    assert reach.argmax() == at and reach[at] > 2.0 * np.delete(reach, at).max()
    lo_, hi_ = icases.root_box(arrays)
    plan = rt.instance_plan_lbvh(lo_, hi_, W)
    touch = tc.face_touchers(plan["nodes"], n)
    assert touch[:, at].all() and (touch.sum(axis=1) == 1).all()
    box_lo, box_hi = ibc.leaf_boxes_of(plan["nodes"], n)
    keys = ibc.keys_of(box_lo, box_hi)
    run = np.arange(n - tc.RUN, n)
    run = run[run != at]
    assert len(np.unique(keys[run])) == 1 and len(run) >= tc.RUN - 1 and run[0] // tc.BUILD_LANES != run[-1] // tc.BUILD_LANES
    assert tc.longest_run(np.sort(keys)) >= len(run)
    assert len(np.unique(keys)) > n // 8  # (the cover leaves the other copies their spread of cells)
    # without the cover's workgroup the reach and the root box are others: what a dropped partial would give
    group = np.arange(n) // tc.BUILD_LANES == at // tc.BUILD_LANES
    assert reach[~group].max() < 0.5 * reach[at]
    assert (box_lo[~group].min(axis=0) > plan["nodes"]["lo"][0]).all() and (box_hi[~group].max(axis=0) < plan["nodes"]["hi"][0]).all()
    restated = ibc.restated_plan(rt, lo_, hi_, W)
    assert restated["nodes"].tobytes() == plan["nodes"].tobytes()
    assert restated["object_from_world"].tobytes() == plan["object_from_world"].tobytes()


def test_instance_set_equals_many_in_kind(blob):
    """instance_set is instance_cases.many without the loop: the same scales, the same cube."""
    _, arrays = blob
    W, side = tc.instance_set(arrays, 1024, 5)
    rest = np.delete(W, 5, axis=0).astype(np.float64)
    det = np.linalg.det(rest[:, :, :3])
    assert (det > 0).all() and 0.5 ** 3 * 0.999 <= det.min() and det.max() <= 1.5 ** 3 * 1.001
    scale = np.cbrt(det)
    assert np.abs(np.einsum("nij,nkj->nik", rest[:, :, :3], rest[:, :, :3]) - np.eye(3) * scale[:, None, None] ** 2).max() < 1e-5
    many = icases.many(arrays, 1024)
    assert np.abs(rest[:, :, 3]).max() < 1.2 * np.abs(many[:, :, 3]).max() + side


def test_rays_through_the_65537_set_find_many_copies(rt, scene_for):
    """The rays and points of the GPU test's query calls: the oracle finds hits in many copies, not in the cover alone."""
    scene, arrays = scene_for("ties", "longest")
    W, _ = tc.instance_set(arrays, 65537, 65536)
    plan = rt.instance_plan_lbvh(*icases.root_box(arrays), W)
    plan["world_from_object"] = W
    o, d = icases.rays(plan["nodes"], 2000, seed=61)
    want = io.closest(arrays, plan, o, d, 1e5)
    hit = want["hit"].astype(bool)
    assert hit.mean() > 0.2 and len(np.unique(want["instance"][hit])) > 100


# ---- B ----------------------------------------------------------------------------------------------------------------------
def test_build_lbvh_equals_the_restatement_at_80000_faces(rt):
    from tools.big_meshes import terrain

    v, f = terrain(tc.TERRAIN_RESTATED)
    assert len(f) == 80000
    f = np.concatenate([f, np.repeat(f[4321:4322], tc.TERRAIN_COPIES, axis=0)])
    scene = rt.Scene.from_arrays(v, f).build_lbvh()
    tree = bcs.restate(bcs._pad4(v), f)
    assert np.array_equal(scene.triangles, tree["triangles"]) and np.array_equal(scene.nodes, tree["nodes"])
    assert tc.longest_run(tree["keys"]) > tc.TERRAIN_COPIES


def test_the_terrain_holds_a_run_of_equal_keys():
    """The field's own centroids share a key in pairs at the most: hence the copies, whose order among themselves and
    behind the face they copy is the stable sort's."""
    from tools.big_meshes import terrain

    v, f = terrain(tc.TERRAIN)
    assert len(f) == tc.TERRAIN_FACES
    assert tc.longest_run(np.sort(bcs.keys_of(bcs._pad4(v), f))) <= 4
    v, f = tc.big_terrain()
    assert len(f) == tc.TERRAIN_FACES + tc.TERRAIN_COPIES
    keys = bcs.keys_of(bcs._pad4(v), f)
    assert tc.longest_run(np.sort(keys)) > tc.TERRAIN_COPIES > 4 and len(np.unique(keys[tc.TERRAIN_FACES:])) == 1
    assert keys[tc.TERRAIN_COPIED] == keys[-1]


def test_the_terrain_rays_hit_and_miss(rt):
    from tools.big_meshes import terrain

    v, f = terrain(60)
    o4, d4 = tc.terrain_rays(v, 2000, 41)
    assert o4.shape == d4.shape == (2000, 4) and np.isfinite(o4).all() and np.isfinite(d4).all()
    import query_oracle as qo

    hit = qo.closest(orc.SceneArrays.from_scene(rt.Scene.from_arrays(v, f).build_lbvh()), o4, d4, 100000.0)["hit"]
    assert 0.5 < hit.mean() < 1.0


# ---- C ----------------------------------------------------------------------------------------------------------------------
def test_the_sign_meshes(rt):
    for around, across in ((600, 300), (24, 14)):
        v, f = scases.torus(around=around, across=across)
        assert len(f) == 2 * around * across and len(v) == around * across
        pairs = np.sort(np.concatenate([f[:, [0, 1]], f[:, [0, 2]], f[:, [1, 2]]]).astype(np.int64), axis=1)
        assert set(np.unique(pairs[:, 0] * len(v) + pairs[:, 1], return_counts=True)[1].tolist()) == {2}  # closed
        # outward: positive, and an inscribed polyhedron's -- below the torus's 2 pi^2 R r^2 = 3.158 (24 x 12: 2.98)
        assert 2.98 < scases.signed_volume(v, f) < 2.0 * np.pi ** 2 * 0.16
        assert tc.segment_lengths(f) == (6, 2)
    v, f = scases.star(points=200)
    assert len(f) == 800 and set(scases.edge_uses(f).values()) == {2} and scases.signed_volume(v, f) > 0
    v, f = tc.book()
    assert v.shape == (302, 3) and f.shape == (300, 3) and scases.edge_uses(f)[(0, 1)] == 300
    assert np.bincount(f.reshape(-1))[:3].tolist() == [300, 300, 1]
    tri = v[f].astype(np.float64)
    normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert (np.linalg.norm(normal, axis=1) > 1e-3).all()
    unit = normal / np.linalg.norm(normal, axis=1, keepdims=True)
    assert len(np.unique(np.round(unit, 6), axis=0)) == 300  # (no two pages in one plane)
    # the sums' order matters there: summed backwards, a float32 sum of the pages' normals differs
    forward, backward = np.float32(0), np.float32(0)
    for x in unit[:, 0].astype(np.float32):
        forward = np.float32(forward + x)
    for x in unit[::-1, 0].astype(np.float32):
        backward = np.float32(backward + x)
    assert forward != backward


def test_lazy_pseudonormals_are_the_reference_s():
    for v, f in (scases.torus(around=24, across=14), scases.star(points=200), tc.book()):
        whole, lazy = sref.Pseudonormals(v, f), tc.LazyPseudonormals(v, f)
        assert np.array_equal(whole.face, lazy.face)
        for x in whole.vertex:
            assert np.array_equal(whole.vertex[x], lazy.vertex[x]), x
        for key in whole.edge:
            assert np.array_equal(whole.edge[key], lazy.edge[key]), key


@pytest.mark.parametrize("mesh", ["torus_600x300", "star_200"])
def test_the_sign_oracle_against_both_truths_on_the_large_meshes(rt, mesh):
    """The points of the GPU test that the reference speaks about (finite, off the surface by construction): the oracle's
    sign is the float64 pseudonormal's and the winding number's, and the reference leaves out at most its own 1 %."""
    make, closed, count, features = tc.sign_meshes()[mesh]
    v, f = make()
    scene = rt.Scene.from_arrays(v, f).build_bvh(0)
    points, judged = tc.signed_points(v, f, count, tc.SIGN_POINT_SEED, features)
    assert len(points) == count and count * len(f) < 1e8 and judged.sum() > 0.7 * count
    got = orc_s.signed_distance(scene.sorted_faces, scene.vertices, scene.vnormals, points)
    assert np.isfinite(points[judged]).all() and got["hit"][judged].all()
    inside = (got["distance"] < 0)[judged]
    assert inside.sum() >= 20 and (~inside).sum() >= 20
    held = tc.compare_in_batches(points[judged], v, f, inside, closed, 8 if len(f) > 100000 else 128, normals=tc.LazyPseudonormals(v, f))
    print(f"{mesh}: judged {held['judged']} of {int(judged.sum())}, excluded {held['excluded']:.4%}")
    assert not held["violations"], held["violations"]
    assert held["excluded"] <= sref.EXCLUDED_CAP


def test_signed_points_of_every_mesh():
    for name, (make, _, count, features) in tc.sign_meshes().items():
        if name == "torus_600x300":
            continue  # (above)
        v, f = make()
        points, judged = tc.signed_points(v, f, count, tc.SIGN_POINT_SEED, features)
        assert points.shape == (count, 3) and points.dtype == np.float32 and np.isfinite(points[judged]).all()
        assert not np.isfinite(points).all() and count * len(f) < 1e8


# ---- E ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blob16(rt, scene_for):
    base, _ = scene_for("blob", "longest")
    scene = rt.Scene.from_arrays(base.vertices[:, :3] / np.float32(16.0), base.faces.reshape(-1, 3)).build_bvh(0)
    return scene, orc.SceneArrays.from_scene(scene)


def test_the_poses_put_hits_behind_the_carry(rt, blob16):
    _, arrays = blob16
    one = lo.render(orc.params_from_options(rt.Options.defaults(ao_num_samples=1, **tc.ONE_VIEW)), arrays, tc.close_pose(rt))
    flat = one["hit"].reshape(-1)
    assert flat.mean() > 0.9 and flat[tc.VIEWS_TURN:].mean() > 0.9 and (one["ao"].reshape(-1)[tc.VIEWS_TURN:] < 1).any()
    params = orc.params_from_options(rt.Options.defaults(ao_num_samples=1, **tc.MANY_VIEWS))
    poses = tc.orbit_poses(rt, tc.MANY_VIEWS_COUNT, tc.MANY_VIEWS_AWAY)
    hits = [int(lo.render(params, arrays, pose)["hit"].sum()) for pose in poses]
    assert hits[tc.MANY_VIEWS_AWAY] == 0 and all(h > 1000 for v, h in enumerate(hits) if v != tc.MANY_VIEWS_AWAY)
    last = lo.render(params, arrays, poses[-1])
    assert (last["ao"].reshape(-1)[tc.VIEWS_TURN - 77 * 13616:][last["hit"].reshape(-1)[tc.VIEWS_TURN - 77 * 13616:] != 0] < 1).any()


def test_the_instanced_pose_puts_hits_behind_the_carry(rt, blob16):
    _, arrays = blob16
    W = icases.many(arrays, 3, seed=3)
    plan = rt.instance_plan(*icases.root_box(arrays), W)
    plan["world_from_object"] = W
    want = ivo.view(orc.params_from_options(rt.Options.defaults(ao_num_samples=1, **tc.ONE_VIEW)), arrays, plan, ivo.cameras(rt, plan)[0])
    assert want["hit"].reshape(-1)[tc.VIEWS_TURN:].sum() > 100 and (want["ao"].reshape(-1)[tc.VIEWS_TURN:] < 1).any()


def test_the_tiny_views_hit_and_miss(rt, blob16):
    _, arrays = blob16
    poses = tc.tiny_poses(tc.TINY_VIEWS_COUNT, tc.TINY_RADIUS)
    assert poses.shape == (65537, 4, 3) and poses.dtype == np.float32
    frame = poses[:, 1:].astype(np.float64)
    assert np.abs(np.einsum("nij,nkj->nik", frame, frame) - np.eye(3)).max() < 1e-6
    assert np.abs(np.cross(frame[:, 2], frame[:, 1]) - frame[:, 0]).max() < 1e-6  # right = forward x up, as Camera.default's
    looks_at = (poses[:, 3].astype(np.float64) * -poses[:, 0]).sum(axis=1) > 0
    assert np.array_equal(~looks_at, np.arange(65537) % 7 == 6)
    params = orc.params_from_options(rt.Options.defaults(ao_num_samples=1, **tc.TINY_VIEW))
    hits = np.array([int(lo.render(params, arrays, poses[v])["hit"].sum()) for v in tc.checked_views()])
    assert (hits[~looks_at[tc.checked_views()]] == 0).all() and 0 < hits.sum() < 4 * len(hits) and (hits > 0).sum() > 20
