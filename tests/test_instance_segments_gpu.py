"""GPU: instanced segment queries (include/rt_hip_instance_segments.h) against the CPU oracle of
tests/instance_segment_oracle.c on the plan read back from the host, every output word for word, and against the float64
comparator of tests/instance_segment_reference.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import build_cases as bc
import instance_cases
import instance_segment_cases as cases
import instance_segment_oracle as iso
import instance_segment_reference as isr
import orc
import refit_cases as rc
import segment_cases
import segment_oracle as so
import segment_reference as sr
from conftest import bits

pytestmark = pytest.mark.gpu

SORT_MIN = 16384  # RT_QUERY_SORT_MIN
QUERY_WAVES = 4   # kernels/query.hip.h: 64 * QUERY_WAVES segments per workgroup
SIZES = (1, 63, 64, 65, 64 * QUERY_WAVES + 1, SORT_MIN - 1, SORT_MIN + 37)
N_BOX = 3000
MASK_TARGETS = (1, 31, 32, 33, 63, 64, 65, 100)
MASK_POINTS = (3, 65)  # np * nt is no multiple of 64 for every nt but 64 itself (asserted below)
NO_SET = np.zeros((0, 3, 4), np.float32)
NONE = 0xFFFFFFFF


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


def set_and_plan(host, W):
    """Sets W; the plan as the host holds it, read back."""
    host.set_instances(W)
    plan = host.instances()
    assert np.array_equal(plan["world_from_object"], W)
    return plan


def check_pairs(host, arrays, plan, a, b, interval, sort=True, what=""):
    """Both pair forms on the GPU == the oracle's on the plan read back, bit for bit; occluded == the closest form's hit."""
    got = host.instances_segments_closest(a, b, interval, sort=sort)
    assert tuple(got) == iso.FIELDS
    iso.assert_same(got, iso.closest(arrays, plan, a, b, interval), (what, interval, sort))
    occ = host.instances_segments_occluded(a, b, interval, sort=sort)
    assert occ.dtype == np.uint8 and np.array_equal(occ, got["hit"]), (what, interval, sort)
    return got


def check_mask(rt, host, arrays, plan, points, targets, interval, sort=True, what=""):
    """The mask form == the occluded pair form of the oracle on the pairs written out; padding 0; count = popcount."""
    got = host.instances_visibility(points, targets, interval, sort=sort)
    want = iso.mask_of(arrays, plan, points, targets, interval)
    assert got["mask"].shape == want["mask"].shape and got["mask"].dtype == np.uint32 and got["count"].shape == want["count"].shape, what
    assert np.array_equal(got["mask"], want["mask"]), (what, interval, sort, np.argwhere(got["mask"] != want["mask"])[:5].tolist())
    assert np.array_equal(got["count"], want["count"]) and np.array_equal(got["count"], segment_cases.popcount(got["mask"])), (what, interval, sort)
    nt = len(targets)
    if nt % 32:
        assert (got["mask"][:, -1] >> (nt % 32) == 0).all(), what  # padding bits
    assert np.array_equal(rt.unpack_visibility_mask(got["mask"], nt), want["flags"])
    return got, want


@pytest.mark.parametrize("family", instance_cases.FAMILIES)
@pytest.mark.parametrize("mesh,bvh", [("single", "longest"), ("single", "sah"), ("ties", "longest"), ("ties", "sah"), ("blob", "longest"),
                                      ("blob", "sah")])
def test_pair_forms_match_the_oracle(hosts, mesh, bvh, family):
    host, _, arrays = hosts(mesh, bvh)
    plan = set_and_plan(host, instance_cases.family(family, arrays))
    a, b = cases.box_segments(plan["nodes"], N_BOX, seed=41 + instance_cases.FAMILIES.index(family))
    blocked = 0
    for interval in cases.INTERVALS:
        got = check_pairs(host, arrays, plan, a, b, interval, what=(mesh, bvh, family))
        assert got["hit"].shape == (N_BOX,) and got["position"].shape == (N_BOX, 3) and got["instance"].dtype == np.uint32
        assert (got["instance"][got["hit"].astype(bool)] < len(plan["object_from_world"])).all()
        blocked += int(got["hit"].sum())
    assert (0 < blocked < 3 * N_BOX) or mesh == "single"  # (one flat triangle per copy: few segments cross it)
    if mesh == "blob" and family in ("overlap_pair", "rotations", "grid"):
        sa, sb = cases.surface_segments(arrays, plan, 500, seed=43)
        on = check_pairs(host, arrays, plan, sa, sb, cases.SURFACE_INTERVAL, what=(mesh, bvh, family, "surface"))
        assert 0 < on["hit"].sum() < 500
    assert host.last_query_ms > 0.0
    host.set_instances(NO_SET)


@pytest.mark.parametrize("count", instance_cases.COUNTS)
def test_packet_and_sort_edges(hosts, count):
    """Every segment count under every instance count; sort=False gives sort=True's words; subsets write what was asked for."""
    host, _, arrays = hosts("blob", "sah")
    plan = set_and_plan(host, instance_cases.many(arrays, count, seed=3))
    a, b = cases.box_segments(plan["nodes"], max(SIZES), seed=47 + count)
    want = iso.closest(arrays, plan, a, b, cases.INTERVALS[0])
    assert want["hit"].any() and not want["hit"].all()
    for n in SIZES:
        part = {f: v[:n] for f, v in want.items()}
        for sort in (True, False):
            got = host.instances_segments_closest(a[:n], b[:n], sort=sort)
            iso.assert_same(got, part, (count, n, sort))
            assert np.array_equal(host.instances_segments_occluded(a[:n], b[:n], sort=sort), part["hit"]), (count, n, sort)
    for sort in (True, False):
        for subset in (("instance",), ("leaf", "normal"), ("hit", "instance", "position")):
            got = host.instances_segments_closest(a, b, outputs=subset, sort=sort)
            assert set(got) == set(subset)
            iso.assert_same(got, want, (count, sort, subset))
        assert host.instances_segments_closest(a, b, outputs=(), sort=sort) == {}
    empty = host.instances_segments_closest(a[:0], b[:0])
    assert empty["hit"].shape == (0,) and empty["instance"].shape == (0,) and host.instances_segments_occluded(a[:0], b[:0]).shape == (0,)
    with pytest.raises(ValueError):
        host.instances_segments_closest(a, b, outputs=("hit", "colour"))
    host.set_instances(NO_SET)


@pytest.mark.parametrize("nt", MASK_TARGETS)
def test_mask_form(rt, hosts, nt):
    """The packets that straddle points and mask words, under two sets."""
    host, _, arrays = hosts("blob", "longest")
    some = False
    for family, n_points in zip(("rotations", "grid"), MASK_POINTS):
        assert (n_points * nt) % 64 or nt == 64
        plan = set_and_plan(host, instance_cases.family(family, arrays))
        points = cases.box_points(plan["nodes"], n_points, 100 * nt + n_points)
        targets = cases.box_points(plan["nodes"], nt, 100 * nt + n_points + 500)
        for interval in (cases.INTERVALS[0], (-1.0, np.inf)):
            got, want = check_mask(rt, host, arrays, plan, points, targets, interval, what=(family, n_points, nt))
            pa, pb = segment_cases.pairs_of(points, targets)
            assert np.array_equal(want["flags"].reshape(-1), host.instances_segments_occluded(pa, pb, interval).astype(bool)), (family, nt)
            some |= bool(want["flags"].any()) and not want["flags"].all()
    assert some or nt == 1
    host.set_instances(NO_SET)


@pytest.mark.parametrize("n_points,nt", [(131, 1000), (3, 4099)])
def test_mask_form_with_many_targets(rt, hosts, n_points, nt):
    """Rows of many words, and the ray-index division at target counts of other sizes."""
    host, _, arrays = hosts("blob", "sah")
    plan = set_and_plan(host, instance_cases.family("rotations", arrays))
    points, targets = cases.box_points(plan["nodes"], n_points, nt), cases.box_points(plan["nodes"], nt, nt + 500)
    got, _ = check_mask(rt, host, arrays, plan, points, targets, cases.INTERVALS[0], what=(n_points, nt))
    assert got["count"].any()
    host.set_instances(NO_SET)


def test_mask_outputs_and_sorted_points(rt, hosts):
    host, _, arrays = hosts("blob", "sah")
    plan = set_and_plan(host, instance_cases.family("translations", arrays))
    points, targets = cases.box_points(plan["nodes"], SORT_MIN + 5, 7), cases.box_points(plan["nodes"], 3, 8)
    want = iso.mask_of(arrays, plan, points, targets, cases.INTERVALS[0])
    assert want["count"].any() and not (want["count"] == 3).all()
    for sort in (True, False):
        check_mask(rt, host, arrays, plan, points, targets, cases.INTERVALS[0], sort=sort, what=("sorted points", sort))
        only_count = host.instances_visibility(points, targets, outputs=("count",), sort=sort)
        assert set(only_count) == {"count"} and np.array_equal(only_count["count"], want["count"])
        only_mask = host.instances_visibility(points, targets, outputs=("mask",), sort=sort)
        assert set(only_mask) == {"mask"} and np.array_equal(only_mask["mask"], want["mask"])
    assert host.instances_visibility(points, targets, outputs=()) == {}
    # no points, no targets: nothing is launched
    none = host.instances_visibility(points[:0], targets)
    assert none["mask"].shape == (0, 1) and none["count"].shape == (0,)
    none = host.instances_visibility(points[:5], targets[:0])
    assert none["mask"].shape == (5, 0) and np.array_equal(none["count"], np.zeros(5, np.uint32))
    with pytest.raises(ValueError):
        host.instances_visibility(points, targets, outputs=("mask", "colour"))
    host.set_instances(NO_SET)


@pytest.mark.parametrize("family", ["tie_pair", "shear"])
def test_odd_inputs(rt, hosts, family):
    host, _, arrays = hosts("blob", "longest")
    plan = set_and_plan(host, instance_cases.family(family, arrays))
    a, b, _ = cases.odd_segments(arrays)
    some = False
    for interval in cases.INTERVALS + cases.ODD_INTERVALS:
        got = check_pairs(host, arrays, plan, a, b, interval, what=(family, "odd"))
        quiet = cases.nothing_blocks(a, b, plan["nodes"], interval)
        assert not got["hit"][quiet].any(), interval
        some |= bool(got["hit"].any())
        if family == "tie_pair":
            assert (got["instance"][got["hit"].astype(bool)] == 0).all()
    assert some
    # the same odd points as a mask: rows of odd points, columns of odd targets
    for interval in (cases.INTERVALS[0], (-1.0, np.inf), (np.nan, 1.0), (0.75, 0.25)):
        check_mask(rt, host, arrays, plan, a[:70], b[:45], interval, what=(family, "odd mask"))
    host.set_instances(NO_SET)


def without_negative_zero(a, b):
    o, d = sr.rays_of(a, b)
    ok = np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & ~(np.signbit(o) & (o == 0)).any(axis=1) & ~(np.signbit(d) & (d == 0)).any(axis=1)
    return np.ascontiguousarray(np.asarray(a)[ok]), np.ascontiguousarray(np.asarray(b)[ok])


def test_identity_relation_to_the_segment_queries(rt, hosts):
    """One identity instance, a and b - a finite without -0: the library's own segments_* and visibility, word for word."""
    for mesh, bvh in (("blob", "longest"), ("ties", "sah")):
        host, _, arrays = hosts(mesh, bvh)
        plan = set_and_plan(host, instance_cases.family("identity", arrays))
        a, b = cases.box_segments(plan["nodes"], N_BOX, seed=811)
        oa, ob, _ = cases.odd_segments(arrays)
        a, b = without_negative_zero(np.concatenate([a, oa]), np.concatenate([b, ob]))
        for interval in cases.INTERVALS + (cases.SURFACE_INTERVAL,):
            got = host.instances_segments_closest(a, b, interval)
            want = host.segments_closest(a, b, interval)
            assert np.array_equal(host.instances_segments_occluded(a, b, interval), host.segments_occluded(a, b, interval)), (mesh, interval)
            assert np.array_equal(got["hit"], want["hit"]) and want["hit"].any() and not want["hit"].all()
            at = want["distance"] < np.inf
            for f in so.FIELDS:
                assert so.same_words(got[f][at], want[f][at]).all(), (mesh, interval, f)
            assert (got["instance"][at] == 0).all()
        points, targets = a[:67], b[:45]
        mask, plain = host.instances_visibility(points, targets), host.visibility(points, targets)
        assert np.array_equal(mask["mask"], plain["mask"]) and np.array_equal(mask["count"], plain["count"]) and plain["count"].any()
        host.set_instances(NO_SET)


def test_relation_to_the_instanced_ray_queries(rt, hosts):
    """t_lo < 0, t_hi = +inf: the library's own trace_instances_* of (a, b - a) with max_distance +inf."""
    host, _, arrays = hosts("blob", "longest")
    for family in ("rotations", "shear", "grid"):
        plan = set_and_plan(host, instance_cases.family(family, arrays))
        a, b = cases.box_segments(plan["nodes"], N_BOX, seed=53)
        o, d = sr.rays_of(a, b)
        want = host.trace_instances_closest(o, d, np.inf)
        assert want["hit"].any() and not want["hit"].all()
        at = want["distance"] < np.inf
        for t_lo in (-1.0, -np.inf):
            got = host.instances_segments_closest(a, b, (t_lo, np.inf))
            assert np.array_equal(host.instances_segments_occluded(a, b, (t_lo, np.inf)), host.trace_instances_occluded(o, d, np.inf)), family
            assert np.array_equal(got["hit"], want["hit"])
            for f in iso.FIELDS:
                assert iso.same_words(got[f][at], want[f][at]).all(), (family, f)
    host.set_instances(NO_SET)


@pytest.mark.parametrize("family", instance_cases.FAMILIES)
def test_float64_comparator_on_the_gpus_answers(rt, hosts, family):
    host, scene, arrays = hosts("blob", "sah")
    W = instance_cases.family(family, arrays)
    plan = set_and_plan(host, W)
    a, b = cases.box_segments(plan["nodes"], N_BOX, seed=900 + instance_cases.FAMILIES.index(family))
    interval = cases.INTERVALS[instance_cases.FAMILIES.index(family) % 3]
    ref = isr.segments(scene, W, a, b, interval)
    got = host.instances_segments_closest(a, b, interval)
    for rep in (isr.compare_occluded(ref, host.instances_segments_occluded(a, b, interval)), isr.compare_closest(scene, ref, got)):
        print(f"INSTANCE SEGMENTS GPU blob/sah {family} {interval}: {rep}")
        bad = rep.failures(tol=isr.TOL, max_unjudged=0.01)
        assert not bad, (family, interval, bad)
    if family == "rotations":  # the mask form's bits, judged the same way
        points, targets = cases.box_points(plan["nodes"], 60, 9), cases.box_points(plan["nodes"], 50, 10)
        pa, pb = segment_cases.pairs_of(points, targets)
        flags = host.instances_visibility(points, targets)["mask"]
        rep = isr.compare_occluded(isr.segments(scene, W, pa, pb, cases.INTERVALS[0]), rt.unpack_visibility_mask(flags, 50).reshape(-1))
        assert not rep.failures(), rep.failures()
    host.set_instances(NO_SET)


def test_after_update_build_upload_replacing_and_clearing(rt):
    scene = rc.fresh_scene(rt, "blob", "longest")
    host = new_host(rt, scene)
    arrays = orc.SceneArrays.from_scene(scene)
    W = instance_cases.family("rotations", arrays)
    first = set_and_plan(host, W)
    a, b = cases.box_segments(first["nodes"], 2000, seed=59)
    points, targets = cases.box_points(first["nodes"], 40, 61), cases.box_points(first["nodes"], 70, 62)
    before = check_pairs(host, arrays, first, a, b, cases.INTERVALS[0], what="first")
    moved = rc.steps("twist", scene.vertices)[-1]
    scene.refit(moved)
    host.update_vertices(moved, scene.vnormals)
    arrays = orc.SceneArrays.from_scene(scene)
    # the set persists; the tree is made again from the new root box BY the query (no host.instances() in between)
    got = host.instances_segments_closest(a, b, cases.INTERVALS[0])
    plan = host.instances()
    assert plan["nodes"].tobytes() != first["nodes"].tobytes() and np.array_equal(plan["world_from_object"], W)
    iso.assert_same(got, iso.closest(arrays, plan, a, b, cases.INTERVALS[0]), "updated")
    assert got["hit"].any() and not np.array_equal(bits(got["distance"]), bits(before["distance"]))
    check_mask(rt, host, arrays, plan, points, targets, cases.INTERVALS[0], what="updated")
    # a build: the leaf order is the LBVH scene's
    v, f = bc.mesh("blob")
    built = bc.lbvh_scene(rt, "blob")
    host.build_scene(v, f, built.vnormals)
    arrays = orc.SceneArrays.from_scene(built)
    mask = host.instances_visibility(points, targets)
    after = host.instances()
    assert after["nodes"].tobytes() != plan["nodes"].tobytes()
    want = iso.mask_of(arrays, after, points, targets, cases.INTERVALS[0])
    assert np.array_equal(mask["mask"], want["mask"]) and np.array_equal(mask["count"], want["count"])
    for interval in cases.INTERVALS:
        check_pairs(host, arrays, after, a, b, interval, what="built")
    # a new upload: the set is still there
    host.upload_scene(scene)
    arrays = orc.SceneArrays.from_scene(scene)
    got = host.instances_segments_closest(a, b, cases.INTERVALS[0])
    again = host.instances()
    assert again["nodes"].tobytes() == plan["nodes"].tobytes()
    iso.assert_same(got, iso.closest(arrays, again, a, b, cases.INTERVALS[0]), "uploaded again")
    # another set in its place, then none
    two = set_and_plan(host, instance_cases.family("scales", arrays))
    second = check_pairs(host, arrays, two, a, b, cases.INTERVALS[0], what="second set")
    assert not np.array_equal(bits(second["distance"]), bits(got["distance"]))
    host.set_instances(NO_SET)
    for call in (lambda: host.instances_segments_closest(a, b), lambda: host.instances_segments_occluded(a, b),
                 lambda: host.instances_visibility(points, targets)):
        with pytest.raises(rt.RtError) as e:
            call()
        assert e.value.code == rt.api.RT_E_STATE
    host.close()


def test_plain_families_and_frames_ignore_the_set(rt, scene_for):
    """segments_occluded, segments_closest, visibility and a rendered frame: the same bits without a set, with one, and
    after the new calls; the new calls leave a frame in flight alone."""
    scene, arrays = scene_for("blob", "longest")
    host = rt.Host(rt.Options.defaults(width=96, height=64, n_super_samples=4, ao_num_samples=3), 0)
    host.upload_scene(scene)
    host.render()
    frame = host.download()
    stats = host.stats()
    W = instance_cases.family("grid", arrays)
    probe = cases.plan_for(rt, arrays, W)
    a, b = cases.box_segments(probe["nodes"], SORT_MIN + 100, seed=71)
    sa, sb = segment_cases.box_segments(arrays, 3000, seed=72)
    a, b = np.concatenate([a, sa]), np.concatenate([b, sb])
    points, targets = segment_cases.mask_inputs(arrays, 300, 70, seed=73)

    def plain():
        return host.segments_closest(a, b), {"hit": host.segments_occluded(a, b)}, host.visibility(points, targets)

    without = plain()
    assert without[0]["hit"].any() and without[2]["count"].any()
    plan = set_and_plan(host, W)
    with_set = plain()
    first = host.instances_segments_closest(a, b)
    mask = host.instances_visibility(points, targets)
    iso.assert_same(first, iso.closest(arrays, plan, a, b, cases.INTERVALS[0]), "grid")
    assert first["hit"].any() and not np.array_equal(first["hit"], without[0]["hit"]) and host.stats() == stats
    after_calls = plain()
    for other in (with_set, after_calls):
        for got, want in zip(other, without):
            so.assert_same(got, want, "plain families with a set")
    host.render()
    assert np.array_equal(bits(host.download()), bits(frame))
    host.render_async()  # a frame left in flight while the queries run
    during = host.instances_segments_closest(a, b, sort=False)
    during_mask = host.instances_visibility(points, targets, sort=False)
    host.sync()
    assert np.array_equal(bits(host.download()), bits(frame)) and host.stats() == stats
    iso.assert_same(during, first, "beside a frame")
    assert np.array_equal(during_mask["mask"], mask["mask"]) and np.array_equal(during_mask["count"], mask["count"])
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
    W = instance_cases.family("rotations", arrays)
    host = new_host(rt)
    p = np.zeros((4, 3), np.float32)
    calls = (lambda h: h.instances_segments_occluded(p, p), lambda h: h.instances_segments_closest(p, p), lambda h: h.instances_visibility(p, p))
    STATE, INVALID = rt.api.RT_E_STATE, rt.api.RT_E_INVALID
    host.set_instances(W)  # (a set, but no upload yet)
    for call in calls:
        with pytest.raises(rt.RtError) as e:
            call(host)
        assert e.value.code == STATE
    host.set_instances(NO_SET)
    host.upload_scene(scene)
    for call in calls:  # (an upload, but no set)
        with pytest.raises(rt.RtError) as e:
            call(host)
        assert e.value.code == STATE
    p4 = np.zeros((4, 4), np.float32)
    at = p4.ctypes.data
    assert lib.rt_instances_segments_occluded(host._h, None, None, 0, 0.0, 1.0, 0, None) == STATE  # (the set comes first)
    host.set_instances(W)
    assert lib.rt_instances_segments_occluded(host._h, None, at, 4, 0.0, 1.0, 0, None) == INVALID
    assert lib.rt_instances_segments_closest(host._h, at, None, 4, 0.0, 1.0, 0, None) == INVALID
    assert lib.rt_instances_segments_closest_device(host._h, None, None, 4, 0.0, 1.0, 0, None, None) == INVALID
    assert lib.rt_instances_visibility_masks(host._h, None, 4, at, 4, 0.0, 1.0, 0, None) == INVALID
    assert lib.rt_instances_segments_occluded(host._h, None, None, 0, 0.0, 1.0, 0, None) == 0
    assert lib.rt_instances_visibility_masks(host._h, None, 0, None, 7, 0.0, 1.0, 0, None) == 0
    assert lib.rt_instances_visibility_masks(host._h, None, 7, None, 0, 0.0, 1.0, 0, None) == 0
    assert lib.rt_instances_segments_occluded(host._h, at, at, (1 << 27) + 1, 0.0, 1.0, 0, None) == INVALID
    assert lib.rt_instances_visibility_masks(host._h, at, 1 << 14, at, (1 << 13) + 1, 0.0, 1.0, 0, None) == INVALID  # np * nt
    assert lib.rt_instances_visibility_masks(host._h, at, 1 << 20, at, 1 << 20, 0.0, 1.0, 0, None) == INVALID       # (no 32-bit wrap)
    assert lib.rt_instances_segments_closest(host._h, at, at, 4, 0.0, 1.0, 0, None) == 0  # (no outputs: nothing is written)
    assert lib.rt_instances_visibility_masks(host._h, at, 4, at, 4, 0.0, 1.0, 0, None) == 0
    assert lib.rt_instances_segments_occluded(None, at, at, 4, 0.0, 1.0, 0, None) == INVALID
    with pytest.raises(ValueError):
        host.instances_segments_occluded(p.astype(np.float64), p)
    with pytest.raises(ValueError):
        host.instances_segments_occluded(p, p[:3])
    mem = _DeviceBytes(2 * 65 * 16 + 4096)
    a, b, out = mem.ptr.value, mem.ptr.value + 65 * 16, mem.ptr.value + 2 * 65 * 16
    assert lib.rt_instances_segments_occluded_device(host._h, a + 4, b, 64, 0.0, 1.0, 0, out, None) == INVALID
    assert lib.rt_instances_segments_closest_device(host._h, a, b + 8, 64, 0.0, 1.0, 0, None, None) == INVALID
    assert lib.rt_instances_visibility_masks_device(host._h, a + 4, 8, b, 8, 0.0, 1.0, 0, None, None) == INVALID
    arrays_ = rt.api._InstanceHitArrays(rt.api._HitArrays(None, out + 2, None, None, None, None), None)
    assert lib.rt_instances_segments_closest_device(host._h, a, b, 64, 0.0, 1.0, 0, C.byref(arrays_), None) == INVALID
    arrays_ = rt.api._InstanceHitArrays(rt.api._HitArrays(None, None, None, None, None, None), out + 2)
    assert lib.rt_instances_segments_closest_device(host._h, a, b, 64, 0.0, 1.0, 0, C.byref(arrays_), None) == INVALID
    arrays_ = rt.api._InstanceHitArrays(rt.api._HitArrays(out + 1, out + 4, None, None, None, None), out + 512)  # (the flags are bytes)
    assert lib.rt_instances_segments_closest_device(host._h, a, b, 64, 0.0, 1.0, 0, C.byref(arrays_), None) == 0
    assert lib.rt_instances_segments_occluded_device(host._h, a, b, 64, 0.0, 1.0, 0, out + 3, None) == 0
    rows = rt.api._VisibilityArrays(out + 2, None)
    assert lib.rt_instances_visibility_masks_device(host._h, a, 8, b, 8, 0.0, 1.0, 0, C.byref(rows), None) == INVALID
    rows = rt.api._VisibilityArrays(out, out + 1024)
    assert lib.rt_instances_visibility_masks_device(host._h, a, 8, b, 8, 0.0, 1.0, 0, C.byref(rows), None) == 0
    assert host.last_query_ms >= 0.0  # (waits for the query)
    host.close()
    mem.free()
    ring = rt.FrameRing(rt.Options.defaults(width=32, height=32, ao_num_samples=3), hosts=2)
    ring.set_calibration(False)
    ring.upload_scene(scene)
    for call in calls:
        with pytest.raises(rt.RtError) as e:
            call(ring.host(0))
        assert e.value.code == STATE
    ring.close()


def test_torch_path_equals_numpy_path():
    """Device tensors in and device tensors out on a non-default stream == the numpy path
    (tests/instance_segments_torch_driver.py, a child process that brings torch's runtime up before it loads the library)."""
    driver = os.path.join(os.path.dirname(os.path.abspath(__file__)), "instance_segments_torch_driver.py")
    r = subprocess.run([sys.executable, driver], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "INSTANCE_SEGMENTS_TORCH_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
