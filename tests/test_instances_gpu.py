"""GPU: instanced ray queries (include/rt_hip_instances.h) against the CPU oracle of tests/instance_oracle.c on the tree the
library built, every output word for word, and against the float64 comparator of tests/instance_reference.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import build_cases as bc
import instance_cases as cases
import instance_oracle as io
import instance_reference as ir
import orc
import refit_cases as rc
from conftest import bits

pytestmark = pytest.mark.gpu

SORT_MIN = 16384  # RT_QUERY_SORT_MIN
SIZES = (1, 63, 64, 65, 257, 2000)
NONE = 0xFFFFFFFF
_REF = {}


def new_host(rt, scene=None):
    host = rt.Host(rt.Options.defaults(width=64, height=48, n_super_samples=1), 0)
    if scene is not None:
        host.upload_scene(scene)
    return host


@pytest.fixture(scope="module")
def hosts(rt, scene_for):
    made = {}

    def get(mesh, bvh):
        if (mesh, bvh) not in made:
            scene, arrays = scene_for(mesh, bvh)
            made[(mesh, bvh)] = (new_host(rt, scene), scene, arrays)
        return made[(mesh, bvh)]

    yield get
    for host, _, _ in made.values():
        host.close()


def check(host, arrays, plan, o, d, max_distance, sort=True, what=""):
    """Both forms on the GPU == the oracle's on the tree read back, bit for bit; occluded == the closest form's hit."""
    got = host.trace_instances_closest(o, d, max_distance, sort=sort)
    assert tuple(got) == io.FIELDS
    io.assert_same(got, io.closest(arrays, plan, o, d, max_distance), (what, max_distance, sort))
    occ = host.trace_instances_occluded(o, d, max_distance, sort=sort)
    assert occ.dtype == np.uint8 and np.array_equal(occ, got["hit"]), (what, max_distance, sort)
    return got


def set_and_plan(rt, host, arrays, W):
    """Sets W; the plan as the host holds it, which must be the host-only planner's for the scene's root box."""
    host.set_instances(W)
    plan = host.instances()
    lo, hi = cases.root_box(arrays)
    want = rt.instance_plan(lo, hi, W)
    assert np.array_equal(plan["world_from_object"], W) and plan["nodes"].tobytes() == want["nodes"].tobytes()
    assert plan["object_from_world"].tobytes() == want["object_from_world"].tobytes()
    return plan


@pytest.mark.parametrize("mesh,bvh", [("single", "longest"), ("single", "sah"), ("ties", "longest"), ("ties", "sah"), ("blob", "longest"),
                                      ("blob", "sah"), ("bunny", "longest"), ("bunny", "sah")])
def test_both_forms_match_the_oracle(rt, hosts, mesh, bvh):
    host, _, arrays = hosts(mesh, bvh)
    hits = 0
    for count in cases.COUNTS:
        if count == 1000 and mesh != "blob":
            continue
        plan = set_and_plan(rt, host, arrays, cases.many(arrays, count, seed=3))
        o, d = cases.rays(plan["nodes"], max(SIZES), seed=41 + count)
        for n in SIZES:  # (every ray count under every instance count; the unsorted flag on every other call)
            max_distance = cases.MAX_DISTANCES[(n + count) % 3] if n != max(SIZES) else 1e5
            got = check(host, arrays, plan, o[:n], d[:n], max_distance, sort=bool((n + count) % 2), what=(mesh, bvh, count, n))
            assert got["hit"].shape == (n,) and got["position"].shape == (n, 3) and got["instance"].dtype == np.uint32
        hits += int(got["hit"].sum())
        assert (got["instance"][got["hit"].astype(bool)] < count).all()
    assert hits > 0 and host.last_query_ms > 0.0
    empty = host.trace_instances_closest(o[:0], d[:0])
    assert empty["hit"].shape == (0,) and empty["instance"].shape == (0,) and host.trace_instances_occluded(o[:0], d[:0]).shape == (0,)
    host.set_instances(np.zeros((0, 3, 4), np.float32))


@pytest.mark.parametrize("n", [SORT_MIN - 1, SORT_MIN + 37])
def test_around_the_sort_threshold_and_output_subsets(rt, hosts, n):
    host, _, arrays = hosts("blob", "sah")
    plan = set_and_plan(rt, host, arrays, cases.family("rotations", arrays))
    o, d = cases.rays(plan["nodes"], n, seed=47)
    want = io.closest(arrays, plan, o, d, 1e5)
    assert want["hit"].any() and not want["hit"].all()
    for sort in (True, False):
        io.assert_same(host.trace_instances_closest(o, d, sort=sort), want, (n, sort))
        assert np.array_equal(host.trace_instances_occluded(o, d, sort=sort), want["hit"])
        for subset in (("instance",), ("leaf", "normal"), ("hit", "instance", "position")):
            part = host.trace_instances_closest(o, d, outputs=subset, sort=sort)
            assert set(part) == set(subset)
            io.assert_same(part, want, (n, sort, subset))
        assert host.trace_instances_closest(o, d, outputs=(), sort=sort) == {}
    with pytest.raises(ValueError):
        host.trace_instances_closest(o, d, outputs=("hit", "colour"))
    host.set_instances(np.zeros((0, 3, 4), np.float32))


@pytest.mark.parametrize("mesh", ["blob", "ties"])
def test_tie_pair_and_odd_rays(rt, hosts, mesh):
    host, _, arrays = hosts(mesh, "longest")
    plan = set_and_plan(rt, host, arrays, cases.family("tie_pair", arrays))
    o, d = cases.rays(plan["nodes"], 2000, seed=51)
    got = check(host, arrays, plan, o, d, 1e5, what=(mesh, "tie pair"))
    assert got["hit"].sum() > 50 and (got["instance"][got["hit"].astype(bool)] == 0).all()
    # odd rays against the oracle: zero, NaN and infinite components, no direction; odd max_distance values too
    for family in ("rotations", "mirror", "shear"):
        plan = set_and_plan(rt, host, arrays, cases.family(family, arrays))
        oo, od = cases.odd_rays(plan["nodes"])
        for max_distance in cases.MAX_DISTANCES + (np.inf, np.nan, -1.0, 0.0):
            got = check(host, arrays, plan, oo, od, max_distance, what=(mesh, family, "odd rays"))
            quiet = (od == 0).all(axis=1) | np.isnan(oo).any(axis=1) | np.isnan(od).any(axis=1)
            assert not got["hit"][quiet].any()
    host.set_instances(np.zeros((0, 3, 4), np.float32))


def test_identity_relation_to_the_ray_queries(rt, hosts):
    """One identity instance, rays with finite components and no -0: trace_occluded's flags, and trace_closest's record word
    for word where its distance is below +inf, with instance 0 -- on the GPU."""
    for mesh in ("blob", "bunny"):
        host, _, arrays = hosts(mesh, "longest")
        plan = set_and_plan(rt, host, arrays, cases.family("identity", arrays))
        o, d = cases.rays(plan["nodes"], 3000, seed=53)
        oo, od = cases.odd_rays(plan["nodes"])
        o, d = cases.without_negative_zero(np.concatenate([o, oo]), np.concatenate([d, od]))
        for max_distance in (1e5, 0.3):
            got = host.trace_instances_closest(o, d, max_distance)
            want = host.trace_closest(o, d, max_distance)
            assert np.array_equal(host.trace_instances_occluded(o, d, max_distance), host.trace_occluded(o, d, max_distance)), mesh
            assert np.array_equal(got["hit"], want["hit"]) and want["hit"].any() and not want["hit"].all()
            at = want["distance"] < np.inf
            for f in want:
                assert io.same_words(got[f][at], want[f][at]).all(), (mesh, f)
            assert (got["instance"][at] == 0).all()
        host.set_instances(np.zeros((0, 3, 4), np.float32))


@pytest.mark.parametrize("family", cases.FAMILIES)
def test_float64_comparator_on_the_gpus_answers(rt, hosts, family):
    for bvh in ("longest", "sah"):
        host, scene, arrays = hosts("blob", bvh)
        W = cases.family(family, arrays)
        plan = set_and_plan(rt, host, arrays, W)
        o, d = cases.rays(plan["nodes"], 3000, seed=700 + cases.FAMILIES.index(family))
        max_distance = cases.MAX_DISTANCES[cases.FAMILIES.index(family) % 3]
        if family not in _REF:  # (the reference knows no tree: one answer for both builders)
            _REF[family] = ir.instanced(scene, W, o, d, max_distance)
        ref = _REF[family]
        got = host.trace_instances_closest(o, d, max_distance)
        for rep in (ir.compare_occluded(ref, host.trace_instances_occluded(o, d, max_distance)), ir.compare_closest(scene, ref, got)):
            print(f"INSTANCES GPU blob/{bvh} {family} max_distance {max_distance}: {rep}")
            assert not rep.failures(tol=ir.TOL), (family, bvh, rep.failures(tol=ir.TOL))
        host.set_instances(np.zeros((0, 3, 4), np.float32))


def test_after_update_vertices_and_after_build_scene(rt):
    scene = rc.fresh_scene(rt, "blob", "longest")
    host = new_host(rt, scene)
    arrays = orc.SceneArrays.from_scene(scene)
    W = cases.family("rotations", arrays)
    first = set_and_plan(rt, host, arrays, W)
    moved = rc.steps("twist", scene.vertices)[-1]
    scene.refit(moved)
    host.update_vertices(moved, scene.vnormals)
    arrays = orc.SceneArrays.from_scene(scene)
    plan = host.instances()  # (the set persists; the tree is made again from the new root box)
    lo, hi = cases.root_box(arrays)
    assert plan["nodes"].tobytes() != first["nodes"].tobytes() and plan["nodes"].tobytes() == rt.instance_plan(lo, hi, W)["nodes"].tobytes()
    assert np.array_equal(plan["world_from_object"], W)
    o, d = cases.rays(plan["nodes"], 2000, seed=59)
    assert check(host, arrays, plan, o, d, 1e5, what="updated")["hit"].any()
    # a build: the leaf order is the LBVH scene's
    v, f = bc.mesh("blob")
    built = bc.lbvh_scene(rt, "blob")
    host.build_scene(v, f, built.vnormals)
    arrays = orc.SceneArrays.from_scene(built)
    after = host.instances()
    lo, hi = cases.root_box(arrays)
    assert after["nodes"].tobytes() != plan["nodes"].tobytes() and after["nodes"].tobytes() == rt.instance_plan(lo, hi, W)["nodes"].tobytes()
    o, d = cases.rays(after["nodes"], 2000, seed=67)
    got = check(host, arrays, after, o, d, 1e5, what="built")

    class Built:  # what the float64 comparator needs of a scene the host built itself
        vertices, faces, vnormals = built.vertices, built.faces, built.vnormals

        @staticmethod
        def face_of_leaf(leaves):
            return host.face_of_leaf(np.ascontiguousarray(leaves, np.uint32))

    rep = ir.compare_closest(Built, ir.instanced(Built, W, o, d, 1e5), got)
    assert not rep.failures(tol=ir.TOL), rep.failures(tol=ir.TOL)
    # a new upload: the set is still there
    host.upload_scene(scene)
    arrays = orc.SceneArrays.from_scene(scene)
    again = host.instances()
    assert again["nodes"].tobytes() == plan["nodes"].tobytes()
    check(host, arrays, again, o, d, 1e5, what="uploaded again")
    host.close()


def test_replacing_and_clearing_the_set(rt, hosts):
    host, _, arrays = hosts("blob", "sah")
    one = set_and_plan(rt, host, arrays, cases.family("translations", arrays))
    o, d = cases.rays(one["nodes"], 2000, seed=61)
    first = check(host, arrays, one, o, d, 1e5, what="first set")
    two = set_and_plan(rt, host, arrays, cases.family("scales", arrays))
    second = check(host, arrays, two, o, d, 1e5, what="second set")
    assert not np.array_equal(first["distance"].view(np.uint32), second["distance"].view(np.uint32))
    lib = rt.load_library()
    assert lib.rt_instance_count(host._h) == 5 and lib.rt_instance_node_count(host._h) == 9
    host.set_instances(np.zeros((0, 3, 4), np.float32))
    assert lib.rt_instance_count(host._h) == 0 and lib.rt_instance_node_count(host._h) == 0
    for call in (lambda: host.trace_instances_closest(o, d), lambda: host.trace_instances_occluded(o, d), lambda: host.instances()):
        with pytest.raises(rt.RtError) as e:
            call()
        assert e.value.code == rt.api.RT_E_STATE


def test_queries_leave_frames_and_plain_queries_alone(rt, scene_for):
    scene, arrays = scene_for("bunny", "longest")
    host = rt.Host(rt.Options.defaults(width=96, height=64, n_super_samples=4, ao_num_samples=3), 0)
    host.upload_scene(scene)
    host.render()
    before = host.download()
    stats = host.stats()
    probe = rt.instance_plan(*cases.root_box(arrays), cases.family("grid", arrays))
    o, d = cases.rays(probe["nodes"], 20000, seed=71)
    plain = host.trace_closest(o, d)
    host.set_instances(cases.family("grid", arrays))
    plan = host.instances()
    first = host.trace_instances_closest(o, d)
    assert first["hit"].any() and host.stats() == stats
    io.assert_same(first, io.closest(arrays, plan, o, d, 1e5), "grid of bunnies")
    host.render()
    assert np.array_equal(bits(host.download()), bits(before))
    host.render_async()  # a frame left in flight while the queries run
    during = host.trace_instances_closest(o, d, sort=False)
    host.sync()
    assert np.array_equal(bits(host.download()), bits(before))
    assert host.stats() == stats
    io.assert_same(during, first, "beside a frame")
    io.assert_same(host.trace_closest(o, d), plain, "plain queries with a set")
    assert host.last_query_ms > 0.0
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
    scene, arrays = scene_for("blob", "longest")
    host = new_host(rt)
    p = np.zeros((4, 3), np.float32)
    STATE, INVALID = rt.api.RT_E_STATE, rt.api.RT_E_INVALID
    W = cases.family("rotations", arrays)
    for call in (lambda: host.trace_instances_occluded(p, p), lambda: host.trace_instances_closest(p, p)):
        with pytest.raises(rt.RtError) as e:
            call()
        assert e.value.code == STATE
    host.set_instances(W)  # (before an upload: kept, the tree comes with the scene)
    with pytest.raises(rt.RtError) as e:
        host.trace_instances_occluded(p, p)
    assert e.value.code == STATE
    with pytest.raises(rt.RtError) as e:
        host.instances()
    assert e.value.code == STATE
    host.upload_scene(scene)
    plan = host.instances()
    assert np.array_equal(plan["world_from_object"], W)
    host.set_instances(W[:0])
    with pytest.raises(rt.RtError) as e:  # an upload, no set
        host.trace_instances_closest(p, p)
    assert e.value.code == STATE
    host.set_instances(W)
    o, d = cases.rays(plan["nodes"], 500, seed=5)
    want = host.trace_instances_closest(o, d)
    # each odd transform is refused and the earlier set still answers
    for name, odd in cases.odd_transforms(arrays).items():
        with pytest.raises(rt.RtError) as e:
            host.set_instances(np.concatenate([W[:2], odd, W[2:]]))
        assert e.value.code == INVALID, name
        assert host.instances()["nodes"].tobytes() == plan["nodes"].tobytes(), name
        io.assert_same(host.trace_instances_closest(o, d), want, name)
    p4 = np.zeros((4, 4), np.float32)
    at = p4.ctypes.data
    assert lib.rt_set_instances(host._h, None, 3) == INVALID
    assert lib.rt_set_instances(host._h, W.ctypes.data, (1 << 20) + 1) == INVALID
    assert lib.rt_set_instances(None, W.ctypes.data, 1) == INVALID
    assert lib.rt_instance_count(host._h) == len(W)
    assert lib.rt_trace_instances_occluded(host._h, None, at, 4, 1.0, 0, None) == INVALID
    assert lib.rt_trace_instances_closest(host._h, at, None, 4, 1.0, 0, None) == INVALID
    assert lib.rt_trace_instances_closest_device(host._h, None, None, 4, 1.0, 0, None, None) == INVALID
    assert lib.rt_trace_instances_occluded(host._h, None, None, 0, 1.0, 0, None) == 0
    assert lib.rt_trace_instances_occluded(host._h, at, at, (1 << 27) + 1, 1.0, 0, None) == INVALID
    assert lib.rt_trace_instances_closest(host._h, at, at, 4, 1.0, 0, None) == 0  # (no outputs: nothing is written)
    assert lib.rt_trace_instances_occluded(None, at, at, 4, 1.0, 0, None) == INVALID
    with pytest.raises(ValueError):
        host.trace_instances_occluded(p.astype(np.float64), p)
    with pytest.raises(ValueError):
        host.trace_instances_occluded(p, p[:3])
    with pytest.raises(ValueError):
        host.set_instances(W.astype(np.float64))
    with pytest.raises(ValueError):
        host.set_instances(W.reshape(-1, 12))
    mem = _DeviceBytes(2 * 65 * 16 + 4096)
    a, b, out = mem.ptr.value, mem.ptr.value + 65 * 16, mem.ptr.value + 2 * 65 * 16
    assert lib.rt_trace_instances_occluded_device(host._h, a + 4, b, 64, 1.0, 0, out, None) == INVALID
    assert lib.rt_trace_instances_closest_device(host._h, a, b + 8, 64, 1.0, 0, None, None) == INVALID
    record = rt.api._HitArrays(None, out + 2, None, None, None, None)
    assert lib.rt_trace_instances_closest_device(host._h, a, b, 64, 1.0, 0, C.byref(rt.api._InstanceHitArrays(record, None)), None) == INVALID
    record = rt.api._HitArrays(out + 1, out + 4, None, None, None, None)  # (the flags are bytes: any address)
    assert lib.rt_trace_instances_closest_device(host._h, a, b, 64, 1.0, 0, C.byref(rt.api._InstanceHitArrays(record, out + 1026)), None) == INVALID
    assert lib.rt_trace_instances_closest_device(host._h, a, b, 64, 1.0, 0, C.byref(rt.api._InstanceHitArrays(record, out + 1024)), None) == 0
    assert lib.rt_trace_instances_occluded_device(host._h, a, b, 64, 1.0, 0, out + 3, None) == 0
    assert host.last_query_ms >= 0.0  # (waits for the query)
    host.close()
    mem.free()
    ring = rt.FrameRing(rt.Options.defaults(width=32, height=32, ao_num_samples=3), hosts=2)
    ring.set_calibration(False)
    ring.upload_scene(scene)
    for call in (lambda: ring.host(0).trace_instances_occluded(p, p), lambda: ring.host(0).set_instances(W), lambda: ring.host(0).instances()):
        with pytest.raises(rt.RtError) as e:
            call()
        assert e.value.code == STATE
    ring.close()


def test_torch_path_equals_numpy_path():
    """Device tensors in and device tensors out on a non-default stream == the numpy path (tests/instances_torch_driver.py, a
    child process that brings torch's runtime up before it loads the library)."""
    driver = os.path.join(os.path.dirname(os.path.abspath(__file__)), "instances_torch_driver.py")
    r = subprocess.run([sys.executable, driver], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "INSTANCES_TORCH_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
