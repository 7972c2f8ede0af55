"""GPU: device-side instance sets (include/rt_hip_instance_build.h) -- a set built on the device read back against the host
restatement (rt.instance_plan_lbvh) byte for byte, the device-tensor and numpy forms against each other, every instanced
query family on the built set against its CPU oracle on the tree read back and against the same rays under set_instances,
refusals, refreshes after update_vertices / build_scene / a new upload, switching between the two kinds of set, the plain
paths left alone, and the binding's errors."""
import os
import subprocess
import sys

import numpy as np
import pytest

import build_cases as bcs
import instance_build_cases as bc
import instance_cases as cases
import instance_multihit_oracle as imo
import instance_nearest_cases as inc
import instance_nearest_oracle as ino
import instance_oracle as io
import instance_segment_oracle as iso
import orc
import refit_cases as rc
from conftest import bits

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
EMPTY = np.zeros((0, 3, 4), np.float32)
SEGMENT_INTERVAL = (1e-4, 1 - 1e-4)  # (the segment queries' default)
READ_BACK_COUNTS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 65537)  # (the last: more partials than one workgroup has lanes)


def new_host(rt, scene=None):
    host = rt.Host(rt.Options.defaults(width=64, height=48, n_super_samples=1), 0)
    if scene is not None:
        host.upload_scene(scene)
    return host


@pytest.fixture(scope="module")
def hosts(rt, scene_for):
    made = {}

    def get(mesh):
        if mesh not in made:
            scene, arrays = scene_for(mesh, "longest")
            made[mesh] = (new_host(rt, scene), scene, arrays)
        return made[mesh]

    yield get
    for host, _, _ in made.values():
        host.close()


def read_back(host) -> dict:
    plan = host.instances()
    plan["bounds"] = host.instance_bounds()
    return plan


def assert_is_the_restatement(rt, host, arrays, W, what=""):
    """The set as the device holds it == rt.instance_plan_lbvh for the scene's root box, byte for byte."""
    got = read_back(host)
    lo, hi = cases.root_box(arrays)
    want = rt.instance_plan_lbvh(lo, hi, W)
    assert got["world_from_object"].tobytes() == np.ascontiguousarray(W, np.float32).tobytes(), what
    for f in ("object_from_world", "nodes", "bounds"):
        assert got[f].tobytes() == want[f].tobytes(), (what, f, int((np.frombuffer(got[f].tobytes(), np.uint32) != np.frombuffer(want[f].tobytes(), np.uint32)).sum()))
    return got


@pytest.mark.parametrize("mesh", ["single", "blob"])
@pytest.mark.parametrize("n", READ_BACK_COUNTS)
def test_read_back_equals_the_host_restatement(rt, hosts, mesh, n):
    host, _, arrays = hosts(mesh)
    W = cases.many(arrays, n, seed=n)
    host.build_instances(W)
    assert host.last_instance_build_ms() > 0.0
    assert_is_the_restatement(rt, host, arrays, W, (mesh, n))
    host.build_instances(EMPTY)


@pytest.mark.parametrize("name", ["identical70", "far_ill", "tiny_huge", "grid"])
def test_equal_keys_and_hard_families_read_back(rt, hosts, name):
    host, _, arrays = hosts("blob")
    W = bc.sets(arrays)[name]
    host.build_instances(W)
    got = assert_is_the_restatement(rt, host, arrays, W, name)
    if name == "identical70":
        assert np.array_equal(got["nodes"]["leaf"][got["nodes"]["leaf"] != NONE], np.arange(70))
    host.build_instances(EMPTY)


def test_tensor_form():
    """The device-tensor form and the numpy form give the same bytes, on the default and on a side stream; refusals and the
    binding's errors for tensors (tests/instance_build_torch_driver.py, a child process that brings torch's runtime up before
    it loads the library)."""
    driver = os.path.join(os.path.dirname(os.path.abspath(__file__)), "instance_build_torch_driver.py")
    r = subprocess.run([sys.executable, driver], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "INSTANCE_BUILD_TORCH_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def check_every_family(host, scene, arrays, plan, n_rays, seed, what):
    """Closest hit, occlusion, closest points, multi-hit and segments on the host's set == their oracles on `plan`, word for
    word; returns the GPU's answers."""
    o, d = cases.rays(plan["nodes"], n_rays, seed=seed)
    out = {}
    out["closest"] = host.trace_instances_closest(o, d, 1e5)
    io.assert_same(out["closest"], io.closest(arrays, plan, o, d, 1e5), (what, "closest"))
    out["occluded"] = host.trace_instances_occluded(o, d, 0.3)
    assert np.array_equal(out["occluded"], io.occluded(arrays, plan, o, d, 0.3)), (what, "occluded")
    mesh = inc.Mesh(scene)
    points = inc.in_top_box(plan, n_rays, seed + 1)
    out["nearest"] = host.instances_closest_points(points)
    ino.assert_same(out["nearest"], mesh.oracle(plan, points), (what, "closest points"))
    out["multihit"] = host.trace_instances_multihit(o, d, 1e5, k=4)
    imo.assert_same(out["multihit"], imo.first_slots(imo.multihit(arrays, plan, o, d, 1e5, imo.MAX_K), 4), (what, "multi-hit"))
    # segments: from each ray's origin along its direction, as long as the top-level box is wide
    top_lo, top_hi = cases.top_box(plan["nodes"])
    unit = d.astype(np.float64) / np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True)
    a, b = o, (o.astype(np.float64) + unit * float(np.linalg.norm(top_hi - top_lo))).astype(np.float32)
    out["segments"] = host.instances_segments_closest(a, b, SEGMENT_INTERVAL)
    iso.assert_same(out["segments"], iso.closest(arrays, plan, a, b, SEGMENT_INTERVAL), (what, "segments"))
    assert out["closest"]["hit"].any() and out["segments"]["hit"].any() and out["multihit"]["count"].max() >= 1
    return out


@pytest.mark.parametrize("n", [27, 257])
def test_queries_on_the_built_set(rt, hosts, n):
    host, scene, arrays = hosts("blob")
    W = cases.many(arrays, n, seed=11)
    host.build_instances(W)
    built = assert_is_the_restatement(rt, host, arrays, W, n)
    on_built = check_every_family(host, scene, arrays, built, 2000, 90 + n, ("built", n))
    # the same rays under set_instances of the same transforms: another tree over the same boxes, the same records
    host.set_instances(W)
    planned = host.instances()
    assert planned["nodes"].tobytes() != built["nodes"].tobytes()
    assert planned["object_from_world"].tobytes() == built["object_from_world"].tobytes()
    assert host.instance_bounds().tobytes() == built["bounds"].tobytes()  # (instance_bounds' numbers, from the host planner)
    o, d = cases.rays(built["nodes"], 2000, seed=90 + n)
    points = inc.in_top_box(built, 2000, 91 + n)
    got = host.trace_instances_closest(o, d, 1e5)
    for f in io.FIELDS:
        assert io.same_words(got[f], on_built["closest"][f]).all(), (n, f)
    assert np.array_equal(host.trace_instances_occluded(o, d, 0.3), on_built["occluded"])
    near = host.instances_closest_points(points)
    for f in near:
        assert ino.same_words(near[f], on_built["nearest"][f]).all(), (n, "closest points", f)
    many = host.trace_instances_multihit(o, d, 1e5, k=4)
    for f in many:
        assert imo.same_words(many[f], on_built["multihit"][f]).all(), (n, "multi-hit", f)
    host.set_instances(EMPTY)


@pytest.mark.parametrize("at", [0, 128, 256])
def test_a_refused_transform_leaves_the_set(rt, hosts, at):
    host, scene, arrays = hosts("blob")
    good = cases.many(arrays, 257, seed=13)
    host.build_instances(good)
    before = read_back(host)
    o, d = cases.rays(before["nodes"], 2000, seed=97)
    answer = host.trace_instances_closest(o, d, 1e5)
    for name, bad in bc.bad_transforms(arrays).items():
        W = good.copy()
        W[at] = bad
        with pytest.raises(rt.RtError) as e:
            host.build_instances(W)
        assert e.value.code == -1, name
        after = read_back(host)
        for f in before:
            assert before[f].tobytes() == after[f].tobytes(), (name, at, f)
    again = host.trace_instances_closest(o, d, 1e5)
    for f in io.FIELDS:
        assert io.same_words(again[f], answer[f]).all(), (at, f)
    # ... and a host-planned set stays as well
    host.set_instances(good[:5])
    planned = host.instances()
    with pytest.raises(rt.RtError):
        host.build_instances(W)
    assert host.instances()["nodes"].tobytes() == planned["nodes"].tobytes()
    assert np.array_equal(host.instances()["world_from_object"], good[:5])
    host.set_instances(EMPTY)


def test_refresh_after_update_vertices_build_scene_and_a_new_upload(rt):
    scene = rc.fresh_scene(rt, "blob", "longest")
    host = new_host(rt)
    W = cases.many(orc.SceneArrays.from_scene(scene), 27, seed=17)
    host.build_instances(W)  # before an upload: checked and kept, planned at the first use
    assert load_count(rt, host) == 27
    with pytest.raises(rt.RtError):
        host.build_instances(np.where(np.arange(27)[:, None, None] == 3, np.float32(np.nan), W))
    host.upload_scene(scene)
    arrays = orc.SceneArrays.from_scene(scene)
    first = assert_is_the_restatement(rt, host, arrays, W, "first use")
    moved = rc.steps("twist", scene.vertices)[-1]
    scene.refit(moved)
    host.update_vertices(moved, scene.vnormals)
    arrays = orc.SceneArrays.from_scene(scene)
    plan = assert_is_the_restatement(rt, host, arrays, W, "updated")
    assert plan["nodes"].tobytes() != first["nodes"].tobytes() and host.last_instance_build_ms() > 0.0
    check_every_family(host, scene, arrays, plan, 2000, 101, "updated")
    v, f = bcs.mesh("blob")
    built = bcs.lbvh_scene(rt, "blob")
    host.build_scene(v, f, built.vnormals)
    arrays = orc.SceneArrays.from_scene(built)
    after = assert_is_the_restatement(rt, host, arrays, W, "built")
    check_every_family(host, built, arrays, after, 2000, 103, "built")
    host.upload_scene(scene)
    arrays = orc.SceneArrays.from_scene(scene)
    again = assert_is_the_restatement(rt, host, arrays, W, "uploaded again")
    assert again["nodes"].tobytes() == plan["nodes"].tobytes()
    check_every_family(host, scene, arrays, again, 2000, 107, "uploaded again")
    host.close()


def load_count(rt, host) -> int:
    return int(rt.load_library().rt_instance_count(host._h))


def test_switching_between_the_two_kinds_of_set(rt, hosts):
    host, scene, arrays = hosts("blob")
    lo, hi = cases.root_box(arrays)
    A, B = cases.many(arrays, 27, seed=19), cases.family("grid", arrays)
    host.set_instances(A)
    assert host.instances()["nodes"].tobytes() == rt.instance_plan(lo, hi, A)["nodes"].tobytes()
    host.build_instances(B)
    assert load_count(rt, host) == len(B)
    assert_is_the_restatement(rt, host, arrays, B, "built over a planned set")
    host.set_instances(A)
    planned = host.instances()
    assert planned["nodes"].tobytes() == rt.instance_plan(lo, hi, A)["nodes"].tobytes() and np.array_equal(planned["world_from_object"], A)
    host.build_instances(A)
    assert_is_the_restatement(rt, host, arrays, A, "built again")
    host.build_instances(EMPTY)  # n = 0 clears the set
    assert load_count(rt, host) == 0
    o, d = cases.rays(planned["nodes"], 100, seed=3)
    with pytest.raises(rt.RtError) as e:
        host.trace_instances_closest(o, d)
    assert e.value.code == -4
    host.build_instances(A)
    host.set_instances(EMPTY)
    assert load_count(rt, host) == 0


def test_plain_queries_and_frames_are_left_alone(rt, scene_for):
    """A plain trace_closest and a rendered frame give the same bits before, during and after."""
    scene, arrays = scene_for("blob", "longest")
    host = rt.Host(rt.Options.defaults(width=96, height=64, n_super_samples=4, ao_num_samples=3), 0)
    host.upload_scene(scene)
    host.render()
    before, stats = host.download(), host.stats()
    W = cases.family("grid", arrays)
    probe = rt.instance_plan_lbvh(*cases.root_box(arrays), W)
    o, d = cases.rays(probe["nodes"], 20000, seed=71)
    plain = host.trace_closest(o, d)
    host.build_instances(W)
    assert host.stats() == stats
    for f in plain:
        assert io.same_words(host.trace_closest(o, d)[f], plain[f]).all(), ("plain, with a built set", f)
    host.render()
    assert np.array_equal(bits(host.download()), bits(before))
    host.render_async()  # a frame left in flight while the set is built again and queried
    host.build_instances(W)
    during = host.trace_instances_closest(o, d)
    plain_during = host.trace_closest(o, d)
    host.sync()
    assert np.array_equal(bits(host.download()), bits(before)) and host.stats() == stats
    io.assert_same(during, io.closest(arrays, host.instances(), o, d, 1e5), "beside a frame")
    for f in plain:
        assert io.same_words(plain_during[f], plain[f]).all(), ("plain, beside a frame", f)
    host.build_instances(EMPTY)
    for f in plain:
        assert io.same_words(host.trace_closest(o, d)[f], plain[f]).all(), ("plain, after", f)
    host.render()
    assert np.array_equal(bits(host.download()), bits(before))
    host.close()


def test_binding_errors(rt, hosts):
    """(the tensors' errors: tests/instance_build_torch_driver.py)"""
    host, _, arrays = hosts("blob")
    W = cases.many(arrays, 8)
    for bad in (W.astype(np.float64), W[:, :, :3], W.reshape(-1, 12), [[1.0]], W.tolist()):
        with pytest.raises(ValueError):
            host.build_instances(bad)
    # the library's own checks come before anything is read through the pointer: a misaligned one, a null one, too many
    lib = rt.load_library()
    assert lib.rt_build_instances_device(host._h, 0x10004, 8, None) == -1
    assert lib.rt_build_instances_device(host._h, None, 8, None) == -1 and lib.rt_build_instances(host._h, None, 8) == -1
    assert lib.rt_build_instances_device(host._h, 0x10000, (1 << 20) + 1, None) == -1
    assert lib.rt_build_instances_device(None, 0x10000, 8, None) == -1
    assert load_count(rt, host) == 0
    assert lib.rt_instance_bounds(host._h, None) == -4  # (no set)
