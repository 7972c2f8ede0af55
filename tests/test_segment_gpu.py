"""GPU: segment queries (include/rt_hip_segment.h) against the CPU oracle of tests/segment_oracle.c, every output word for
word, and against the float64 comparator of tests/segment_reference.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import build_cases as bc
import orc
import query_oracle as qo
import refit_cases as rc
import segment_cases as cases
import segment_oracle as so
import segment_reference as sr
from conftest import bits

pytestmark = pytest.mark.gpu

SORT_MIN = 16384  # RT_QUERY_SORT_MIN
SIZES = (1, 63, 64, 65, 257, 2000)
MASK_TARGETS = (1, 31, 32, 33, 63, 64, 65, 100)
MASK_POINTS = (1, 2, 3, 65)


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


def check_pairs(host, arrays, a, b, interval, sort=True, what=""):
    """Both pair forms on the GPU == the oracle's, bit for bit; occluded == the closest form's hit."""
    got = host.segments_closest(a, b, interval, sort=sort)
    assert tuple(got) == so.FIELDS
    so.assert_same(got, so.closest(arrays, a, b, interval), (what, interval, sort))
    occ = host.segments_occluded(a, b, interval, sort=sort)
    assert occ.dtype == np.uint8 and np.array_equal(occ, got["hit"]), (what, interval, sort)
    return got


def check_mask(host, arrays, points, targets, interval, sort=True, what=""):
    got = host.visibility(points, targets, interval, sort=sort)
    want = so.visibility(arrays, points, targets, interval)
    assert got["mask"].shape == want["mask"].shape and got["count"].shape == want["count"].shape, what
    so.assert_same(got, want, (what, interval, sort))
    return got


@pytest.mark.parametrize("mesh,bvh", [("single", "longest"), ("single", "sah"), ("ties", "longest"), ("ties", "sah"), ("blob", "longest"),
                                      ("blob", "sah"), ("bunny", "longest"), ("bunny", "sah")])
def test_pair_forms_match_the_oracle(hosts, mesh, bvh):
    host, _, arrays = hosts(mesh, bvh)
    a, b = cases.box_segments(arrays, max(SIZES), seed=41)
    blocked = 0
    for interval in cases.INTERVALS:
        for n in SIZES:
            got = check_pairs(host, arrays, a[:n], b[:n], interval, what=(mesh, bvh, n))
            assert got["hit"].shape == (n,) and got["position"].shape == (n, 3)
        blocked += int(got["hit"].sum())
    if mesh == "single":  # (its box is flat: the segments above lie in the triangle's plane.  These cross it.)
        normal = np.cross(arrays.vertices[1, :3] - arrays.vertices[0, :3], arrays.vertices[2, :3] - arrays.vertices[0, :3]).astype(np.float32)
        lift = normal * np.float32(0.3 / np.linalg.norm(normal))
        for interval in cases.INTERVALS:
            blocked += int(check_pairs(host, arrays, a + lift, b - lift, interval, what=(mesh, bvh, "crossing"))["hit"].sum())
    assert 0 < blocked < 3 * max(SIZES)
    if mesh in ("blob", "ties"):  # (the bunny's ground plane catches nearly every ray: too few pairs leave their own planes)
        sa, sb = cases.surface_segments(arrays, 500, seed=43)
        on = check_pairs(host, arrays, sa, sb, cases.SURFACE_INTERVAL, what=(mesh, bvh, "surface"))
        assert 0 < on["hit"].sum() < 500
        check_pairs(host, arrays, sa, sb, cases.DEFAULT, what=(mesh, bvh, "surface, default interval"))
    assert host.last_query_ms > 0.0
    empty = host.segments_closest(a[:0], b[:0])
    assert empty["hit"].shape == (0,) and empty["normal"].shape == (0, 3) and host.segments_occluded(a[:0], b[:0]).shape == (0,)


@pytest.mark.parametrize("n", [SORT_MIN - 1, SORT_MIN + 37])
def test_around_the_sort_threshold(hosts, n):
    host, _, arrays = hosts("blob", "sah")
    a, b = cases.box_segments(arrays, n, seed=47)
    want = so.closest(arrays, a, b, cases.DEFAULT)
    for sort in (True, False):
        got = host.segments_closest(a, b, sort=sort)
        so.assert_same(got, want, (n, sort))
        assert np.array_equal(host.segments_occluded(a, b, sort=sort), want["hit"])
        part = host.segments_closest(a, b, outputs=("leaf", "normal"), sort=sort)
        assert set(part) == {"leaf", "normal"}
        so.assert_same(part, want, (n, sort, "subset"))


@pytest.mark.parametrize("mesh", ["blob", "ties"])
def test_odd_inputs(hosts, mesh):
    host, _, arrays = hosts(mesh, "longest")
    a, b, nothing = cases.odd_segments(arrays)
    for interval in cases.INTERVALS + cases.ODD_INTERVALS:
        got = check_pairs(host, arrays, a, b, interval, what=(mesh, "odd"))
        quiet = np.ones(len(a), bool) if cases.blocks_nothing(interval) else nothing
        assert not got["hit"][quiet].any(), interval
    # the same odd points as a mask: rows of odd points, columns of odd targets
    for interval in (cases.DEFAULT, (-1.0, np.inf), (np.nan, 1.0), (0.75, 0.25)):
        check_mask(host, arrays, a[:70], b[:45], interval, what=(mesh, "odd mask"))


@pytest.mark.parametrize("nt", MASK_TARGETS)
def test_mask_form(rt, hosts, nt):
    """The packets that straddle points and words; np * nt is no multiple of 64 in most of them."""
    host, _, arrays = hosts("blob", "longest")
    some = False
    for n_points in MASK_POINTS:
        points, targets = cases.mask_inputs(arrays, n_points, nt, seed=100 * nt + n_points)
        for interval in (cases.DEFAULT, (-1.0, np.inf)):
            got = check_mask(host, arrays, points, targets, interval, what=(n_points, nt))
            # padding bits are 0, the count is the popcount, and the mask is the pair form on the same P x T segments
            flags = rt.unpack_visibility_mask(got["mask"], nt)
            assert np.array_equal(got["count"], cases.popcount(got["mask"])) and np.array_equal(got["count"], flags.sum(axis=1))
            pa, pb = cases.pairs_of(points, targets)
            assert np.array_equal(flags.reshape(-1), host.segments_occluded(pa, pb, interval).astype(bool)), (n_points, nt)
            some |= bool(flags.any()) and not flags.all()
    assert some or nt == 1
    assert (3 * 31) % 64 and (65 * 33) % 64 and (3 * 100) % 64


@pytest.mark.parametrize("n_points,nt", [(131, 1000), (3, 4099), (1025, 127)])
def test_mask_form_with_many_targets(hosts, n_points, nt):
    """Rows of many words, and the ray-index division at target counts of other sizes."""
    host, _, arrays = hosts("blob", "sah")
    points, targets = cases.mask_inputs(arrays, n_points, nt, seed=nt)
    got = check_mask(host, arrays, points, targets, cases.DEFAULT, what=(n_points, nt))
    assert got["count"].any() and np.array_equal(got["count"], cases.popcount(got["mask"]))


def test_mask_outputs_and_sorted_points(rt, hosts):
    host, _, arrays = hosts("blob", "sah")
    points, targets = cases.mask_inputs(arrays, SORT_MIN + 5, 3, seed=7)
    want = so.visibility(arrays, points, targets, cases.DEFAULT)
    assert want["count"].any() and not (want["count"] == 3).all()
    for sort in (True, False):
        so.assert_same(host.visibility(points, targets, sort=sort), want, ("sorted points", sort))
        only_count = host.visibility(points, targets, outputs=("count",), sort=sort)
        assert set(only_count) == {"count"} and np.array_equal(only_count["count"], want["count"])
        only_mask = host.visibility(points, targets, outputs=("mask",), sort=sort)
        assert set(only_mask) == {"mask"} and np.array_equal(only_mask["mask"], want["mask"])
    assert host.visibility(points, targets, outputs=()) == {}
    # no points, no targets: nothing is launched
    none = host.visibility(points[:0], targets)
    assert none["mask"].shape == (0, 1) and none["count"].shape == (0,)
    none = host.visibility(points[:5], targets[:0])
    assert none["mask"].shape == (5, 0) and np.array_equal(none["count"], np.zeros(5, np.uint32))
    with pytest.raises(ValueError):
        host.visibility(points, targets, outputs=("mask", "colour"))


def test_relation_to_the_ray_queries(hosts):
    """t_lo < 0, t_hi = +inf: rt_trace_occluded and rt_trace_closest of (a, b - a) with max_distance +inf, on the GPU."""
    for mesh in ("blob", "bunny"):
        host, _, arrays = hosts(mesh, "longest")
        a, b = cases.box_segments(arrays, 3000, seed=53)
        o, d = sr.rays_of(a, b)
        got = host.segments_closest(a, b, (-1.0, np.inf))
        want = host.trace_closest(o, d, np.inf)
        assert np.array_equal(host.segments_occluded(a, b, (-1.0, np.inf)), host.trace_occluded(o, d, np.inf)), mesh
        assert np.array_equal(got["hit"], want["hit"]) and want["hit"].any() and not want["hit"].all()
        at = want["distance"] < np.inf
        for f in so.FIELDS:
            assert so.same_words(got[f][at], want[f][at]).all(), (mesh, f)


@pytest.mark.parametrize("bvh", ["longest", "sah"])
def test_float64_comparator_on_the_gpus_answers(rt, hosts, bvh):
    host, scene, arrays = hosts("blob", bvh)
    a, b = cases.box_segments(arrays, 3000, seed=301)
    for interval in cases.INTERVALS:
        ref = sr.segments(scene, a, b, interval)
        got = host.segments_closest(a, b, interval)
        for rep in (sr.compare_occluded(ref, host.segments_occluded(a, b, interval)), sr.compare_closest(scene, ref, got)):
            print(f"SEGMENT GPU blob/{bvh} {interval}: {rep}")
            assert not rep.failures(tol=sr.TOL), (interval, rep.failures(tol=sr.TOL))
    sa, sb = cases.surface_segments(arrays, 1000, seed=77)
    ref = sr.segments(scene, sa, sb, cases.SURFACE_INTERVAL)
    rep = sr.compare_closest(scene, ref, host.segments_closest(sa, sb, cases.SURFACE_INTERVAL))
    assert not rep.failures(tol=sr.TOL), rep.failures(tol=sr.TOL)
    # the mask form's bits, judged the same way
    points, targets = cases.mask_inputs(arrays, 60, 50, seed=9)
    pa, pb = cases.pairs_of(points, targets)
    flags = host.visibility(points, targets)["mask"]
    rep = sr.compare_occluded(sr.segments(scene, pa, pb, cases.DEFAULT), rt.unpack_visibility_mask(flags, 50).reshape(-1))
    assert not rep.failures(), rep.failures()


class _Built:
    """What the float64 comparator needs of a scene the host built itself: the mesh in file order, and leaves through
    host.face_of_leaf()."""

    def __init__(self, host, vertices, faces, vnormals):
        self.vertices, self.faces, self.vnormals, self.host = vertices, faces, vnormals, host

    def face_of_leaf(self, leaves):
        return self.host.face_of_leaf(np.ascontiguousarray(leaves, np.uint32))


def test_after_update_vertices_and_after_build_scene(rt):
    scene = rc.fresh_scene(rt, "blob", "longest")
    host = new_host(rt, scene)
    moved = rc.steps("twist", scene.vertices)[-1]
    scene.refit(moved)
    host.update_vertices(moved, scene.vnormals)
    arrays = orc.SceneArrays.from_scene(scene)
    a, b = cases.box_segments(arrays, 2000, seed=59)
    points, targets = cases.mask_inputs(arrays, 40, 70, seed=61)
    for interval in cases.INTERVALS:
        assert check_pairs(host, arrays, a, b, interval, what="updated")["hit"].any()
    check_mask(host, arrays, points, targets, cases.DEFAULT, what="updated")
    # a build: the leaf order is the LBVH scene's
    v, f = bc.mesh("blob")
    built = bc.lbvh_scene(rt, "blob")
    host.build_scene(v, f, built.vnormals)
    arrays = orc.SceneArrays.from_scene(built)
    a, b = cases.box_segments(arrays, 2000, seed=67)
    for interval in cases.INTERVALS:
        got = check_pairs(host, arrays, a, b, interval, what="built")
    check_mask(host, arrays, points, targets, cases.DEFAULT, what="built")
    view = _Built(host, built.vertices, built.faces, built.vnormals)
    ref = sr.segments(view, a, b, cases.INTERVALS[-1])
    rep = sr.compare_closest(view, ref, got)
    assert not rep.failures(tol=sr.TOL), rep.failures(tol=sr.TOL)
    host.close()


def test_queries_leave_frames_alone(rt, scene_for):
    scene, arrays = scene_for("bunny", "longest")
    host = rt.Host(rt.Options.defaults(width=96, height=64, n_super_samples=4, ao_num_samples=3), 0)
    host.upload_scene(scene)
    host.render()
    before = host.download()
    stats = host.stats()
    a, b = cases.box_segments(arrays, 20000, seed=71)
    points, targets = cases.mask_inputs(arrays, 300, 70, seed=73)
    first = host.segments_closest(a, b)
    mask = host.visibility(points, targets)
    assert host.stats() == stats
    host.render()
    assert np.array_equal(bits(host.download()), bits(before))
    host.render_async()  # a frame left in flight while the queries run
    during = host.segments_closest(a, b, sort=False)
    during_mask = host.visibility(points, targets, sort=False)
    host.sync()
    assert np.array_equal(bits(host.download()), bits(before))
    assert host.stats() == stats
    so.assert_same(during, first, "beside a frame")
    so.assert_same(during_mask, mask, "beside a frame")
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
    scene, _ = scene_for("blob", "longest")
    host = new_host(rt)
    p = np.zeros((4, 3), np.float32)
    for call in (lambda: host.segments_occluded(p, p), lambda: host.segments_closest(p, p), lambda: host.visibility(p, p)):
        with pytest.raises(rt.RtError) as e:
            call()
        assert e.value.code == rt.api.RT_E_STATE
    host.upload_scene(scene)
    INVALID = rt.api.RT_E_INVALID
    p4 = np.zeros((4, 4), np.float32)
    at = p4.ctypes.data
    assert lib.rt_segments_occluded(host._h, None, at, 4, 0.0, 1.0, 0, None) == INVALID
    assert lib.rt_segments_closest(host._h, at, None, 4, 0.0, 1.0, 0, None) == INVALID
    assert lib.rt_segments_closest_device(host._h, None, None, 4, 0.0, 1.0, 0, None, None) == INVALID
    assert lib.rt_visibility_masks(host._h, None, 4, at, 4, 0.0, 1.0, 0, None) == INVALID
    assert lib.rt_segments_occluded(host._h, None, None, 0, 0.0, 1.0, 0, None) == 0
    assert lib.rt_visibility_masks(host._h, None, 0, None, 7, 0.0, 1.0, 0, None) == 0
    assert lib.rt_visibility_masks(host._h, None, 7, None, 0, 0.0, 1.0, 0, None) == 0
    assert lib.rt_segments_occluded(host._h, at, at, (1 << 27) + 1, 0.0, 1.0, 0, None) == INVALID
    assert lib.rt_visibility_masks(host._h, at, 1 << 14, at, (1 << 13) + 1, 0.0, 1.0, 0, None) == INVALID  # np * nt
    assert lib.rt_visibility_masks(host._h, at, 1 << 20, at, 1 << 20, 0.0, 1.0, 0, None) == INVALID       # (no 32-bit wrap)
    assert lib.rt_segments_closest(host._h, at, at, 4, 0.0, 1.0, 0, None) == 0  # (no outputs: nothing is written)
    assert lib.rt_visibility_masks(host._h, at, 4, at, 4, 0.0, 1.0, 0, None) == 0
    assert lib.rt_segments_occluded(None, at, at, 4, 0.0, 1.0, 0, None) == INVALID
    with pytest.raises(ValueError):
        host.segments_occluded(p.astype(np.float64), p)
    with pytest.raises(ValueError):
        host.segments_occluded(p, p[:3])
    with pytest.raises(ValueError):
        host.segments_closest(p, p, outputs=("hit", "colour"))
    mem = _DeviceBytes(2 * 65 * 16 + 4096)
    a, b, out = mem.ptr.value, mem.ptr.value + 65 * 16, mem.ptr.value + 2 * 65 * 16
    assert lib.rt_segments_occluded_device(host._h, a + 4, b, 64, 0.0, 1.0, 0, out, None) == INVALID
    assert lib.rt_segments_closest_device(host._h, a, b + 8, 64, 0.0, 1.0, 0, None, None) == INVALID
    assert lib.rt_visibility_masks_device(host._h, a + 4, 8, b, 8, 0.0, 1.0, 0, None, None) == INVALID
    arrays = rt.api._HitArrays(None, out + 2, None, None, None, None)
    assert lib.rt_segments_closest_device(host._h, a, b, 64, 0.0, 1.0, 0, C.byref(arrays), None) == INVALID
    arrays = rt.api._HitArrays(out + 1, out + 4, None, None, None, None)  # (the flags are bytes: any address)
    assert lib.rt_segments_closest_device(host._h, a, b, 64, 0.0, 1.0, 0, C.byref(arrays), None) == 0
    assert lib.rt_segments_occluded_device(host._h, a, b, 64, 0.0, 1.0, 0, out + 3, None) == 0
    rows = rt.api._VisibilityArrays(out + 2, None)
    assert lib.rt_visibility_masks_device(host._h, a, 8, b, 8, 0.0, 1.0, 0, C.byref(rows), None) == INVALID
    rows = rt.api._VisibilityArrays(out, out + 1024)
    assert lib.rt_visibility_masks_device(host._h, a, 8, b, 8, 0.0, 1.0, 0, C.byref(rows), None) == 0
    assert host.last_query_ms >= 0.0  # (waits for the query)
    host.close()
    mem.free()
    ring = rt.FrameRing(rt.Options.defaults(width=32, height=32, ao_num_samples=3), hosts=2)
    ring.set_calibration(False)
    ring.upload_scene(scene)
    for call in (lambda: ring.host(0).segments_occluded(p, p), lambda: ring.host(0).visibility(p, p)):
        with pytest.raises(rt.RtError) as e:
            call()
        assert e.value.code == rt.api.RT_E_STATE
    ring.close()
    import torch  # (CPU tensors: the checks come before any device work)

    t = torch.zeros((65, 4), dtype=torch.float32)
    with pytest.raises(ValueError):
        host.segments_occluded(t[:, :3], t[:, :3])  # not contiguous
    with pytest.raises(ValueError):
        host.visibility(t, p)  # a tensor and an array


def test_torch_path_equals_numpy_path():
    """Device tensors in and device tensors out on a non-default stream == the numpy path (tests/segment_torch_driver.py, a
    child process that brings torch's runtime up before it loads the library)."""
    driver = os.path.join(os.path.dirname(os.path.abspath(__file__)), "segment_torch_driver.py")
    r = subprocess.run([sys.executable, driver], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "SEGMENT_TORCH_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
