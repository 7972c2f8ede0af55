"""CPU: the segment queries' contract (include/rt_hip_segment.h) -- the C oracle (tests/segment_oracle.c: the tree's walk with
the oracle's box test at max_distance = t_hi, the triangle test with the interval) against the BVH-free float64 reference
(tests/segment_reference.py), the header and the binding, the relation to the ray queries, odd inputs.  No GPU.

What is asserted: on judged segments the flags and faces are equal and the float fields lie within segment_reference.TOL; at
most 1 % of the segments go unjudged; the floors keep a case from passing vacuously; doctored answers are reported.  Every
test prints its shares and its worst difference per field (pytest -s)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import geometry_reference as gr
import multihit_oracle as mo
import query_oracle as qo
import segment_cases as cases
import segment_oracle as so
import segment_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("rt_segments_occluded", "rt_segments_closest", "rt_visibility_masks", "rt_segments_occluded_device",
                "rt_segments_closest_device", "rt_visibility_masks_device")
MESHES = ("blob", "ties", "layered")
BVHS = ("longest", "sah")
N_BOX, N_SURFACE = 3000, 1000
MAX_UNJUDGED = 0.01
# Floors on the clearly blocked and the clearly open share of the 3000 box segments, per interval in the order of
# cases.INTERVALS.  blob: the 10 % the contract of these tests names.  ties (7 faces) and layered (a stack of plates): half of
# what the float64 reference alone gives for these endpoints (printed below: ties 25.6 / 17.1 / 29.4 % blocked, 74.4 / 82.8 /
# 70.6 % open; layered 87.3 / 81.4 / 89.3 % blocked, 12.7 / 18.6 / 10.7 % open).  (blob itself: 25.5 / 13.4 / 33.8 % blocked.)
FLOORS = {"blob": ((0.10, 0.10), (0.10, 0.10), (0.10, 0.10)),
          "ties": ((0.12, 0.37), (0.085, 0.41), (0.145, 0.35)),
          "layered": ((0.43, 0.06), (0.40, 0.09), (0.44, 0.05))}

_SCENES, _REF = {}, {}


def scene_of(rt, scene_for, mesh, bvh):
    key = (mesh, bvh)
    if key not in _SCENES:
        _SCENES[key] = mo.layered_scene(rt, bvh) if mesh == "layered" else scene_for(mesh, bvh)
    return _SCENES[key]


def box_segments(mesh, arrays):
    return cases.box_segments(arrays, N_BOX, seed=301 + MESHES.index(mesh))


def reference(key, scene, a, b, interval):
    """The reference's answer, once per (case, interval): it knows no tree."""
    key = (key, float(interval[0]), float(interval[1]))
    if key not in _REF:
        _REF[key] = sr.segments(scene, a, b, interval)
        for v in _REF[key].values():
            v.setflags(write=False)
    return _REF[key]


def passes(report, what, max_unjudged=MAX_UNJUDGED):
    print(f"SEGMENT {what}: {report}")
    bad = report.failures(tol=sr.TOL, max_unjudged=max_unjudged)
    assert not bad, (what, bad)


def test_header_library_and_binding(rt):
    header = os.path.join(ROOT, "include", "rt_hip_segment.h")
    assert os.path.exists(header), "include/rt_hip_segment.h is missing"
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(ENTRY_POINTS)
    lib = C.CDLL(rt.lib_path())
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in rt.api._SIGNATURES, name
    for method in ("segments_occluded", "segments_closest", "visibility"):
        assert hasattr(rt.Host, method), method
    assert rt.SEGMENT_INTERVAL == cases.DEFAULT and rt.VISIBILITY_OUTPUTS == ("mask", "count")
    # the oracle restates the triangle test on the oracle's own file, as the ray queries' does
    assert '#include "../oracle/rt_oracle.c"' in open(os.path.join(ROOT, "tests", "segment_oracle.c")).read()
    words = np.array([[0x80000001, 0x2], [0, 0x1]], np.uint32)
    flags = rt.unpack_visibility_mask(words, 34)
    assert flags.shape == (2, 34) and flags[0, 0] and flags[0, 31] and flags[0, 33] and flags[1, 32] and flags.sum() == 4


@pytest.mark.parametrize("interval", cases.INTERVALS)
@pytest.mark.parametrize("bvh", BVHS)
@pytest.mark.parametrize("mesh", MESHES)
def test_oracle_against_the_reference(rt, scene_for, mesh, bvh, interval):
    scene, arrays = scene_of(rt, scene_for, mesh, bvh)
    a, b = box_segments(mesh, arrays)
    ref = reference(mesh, scene, a, b, interval)
    what = f"{mesh}/{bvh} interval {interval}"
    blocked, open_, unsure = ref["blocked"].mean(), ref["open"].mean(), 1.0 - ref["judged_any"].mean()
    print(f"SEGMENT {what}: reference shares: blocked {blocked:.4f}, open {open_:.4f}, borderline {unsure:.4f}; "
          f"closest judged {ref['judged'].mean():.4f}")
    floor = FLOORS[mesh][cases.INTERVALS.index(interval)]
    assert blocked >= floor[0] and open_ >= floor[1], (what, blocked, open_, floor)
    got = so.closest(arrays, a, b, interval)
    occ = so.occluded(arrays, a, b, interval)
    assert np.array_equal(occ, got["hit"]), what
    passes(sr.compare_occluded(ref, occ), what + " occluded")
    passes(sr.compare_closest(scene, ref, got), what + " closest")
    # without a blocker: the fill values, word for word
    free = ~got["hit"].astype(bool)
    assert np.isposinf(got["distance"][free]).all() and (got["leaf"][free] == so.NONE).all()
    for f in ("barycentric", "position", "normal"):
        assert (got[f][free].view(np.uint32) == 0).all(), (what, f)


@pytest.mark.parametrize("bvh", BVHS)
def test_surface_endpoints(rt, scene_for, bvh):
    """Segments between points ON the surface, interval (1e-3, 1 - 1e-3): the triangles the endpoints lie on are at r ~ 0 and
    r ~ 1, outside the interval by a clear margin, so line of sight along the surface is judged -- and often open."""
    scene, arrays = scene_of(rt, scene_for, "blob", bvh)
    a, b = cases.surface_segments(arrays, N_SURFACE, seed=77)
    ref = reference("blob surface", scene, a, b, cases.SURFACE_INTERVAL)
    what = f"blob/{bvh} surface endpoints"
    print(f"SEGMENT {what}: reference shares: blocked {ref['blocked'].mean():.4f}, open {ref['open'].mean():.4f}, "
          f"borderline {1.0 - ref['judged_any'].mean():.4f}")
    assert ref["blocked"].mean() >= 0.10 and ref["open"].mean() >= 0.10
    got = so.closest(arrays, a, b, cases.SURFACE_INTERVAL)
    passes(sr.compare_occluded(ref, so.occluded(arrays, a, b, cases.SURFACE_INTERVAL)), what + " occluded")
    passes(sr.compare_closest(scene, ref, got), what + " closest")
    # with no lower bound every one of them finds the triangle it starts on
    assert so.occluded(arrays, a, b, (-1.0, 1 - 1e-3)).mean() > 0.4


def test_relation_to_the_ray_queries(rt, scene_for):
    """t_lo < 0, t_hi = +inf: the occluded form is rt_trace_occluded of (a, b - a) with max_distance +inf, and where that
    ray's closest hit has a distance below +inf the closest form is rt_trace_closest's record, word for word."""
    for mesh in MESHES:
        for bvh in BVHS:
            scene, arrays = scene_of(rt, scene_for, mesh, bvh)
            a, b = box_segments(mesh, arrays)
            o, d = sr.rays_of(a, b)
            for t_lo in (-1.0, -np.inf, -1e-30):
                got = so.closest(arrays, a, b, (t_lo, np.inf))
                want = qo.closest(arrays, o, d, np.inf)
                assert np.array_equal(so.occluded(arrays, a, b, (t_lo, np.inf)), qo.occluded(arrays, o, d, np.inf)), (mesh, bvh)
                assert want["hit"].any()
                at = want["distance"] < np.inf
                for f in so.FIELDS:
                    assert so.same_words(got[f][at], want[f][at]).all(), (mesh, bvh, f)
                assert np.array_equal(got["hit"], want["hit"])


def test_the_interval_is_on_the_plane_parameter(rt, scene_for):
    """A wrong interval rule shows: with (t_lo, t_hi) inside (0, 1) the blockers are those of the ray whose r lies inside, so
    the closest blocker of the interval is the first of the ray's hits (multi-hit, in distance order = r order) with
    t_lo < r < t_hi, r = distance / |d| up to rounding -- checked away from the interval's ends."""
    scene, arrays = scene_of(rt, scene_for, "layered", "longest")
    a, b = box_segments("layered", arrays)
    o, d = sr.rays_of(a, b)
    multi = mo.multihit(arrays, o, d, np.inf, mo.MAX_K)
    length = np.linalg.norm(d.astype(np.float64), axis=1)
    r = multi["distance"].astype(np.float64) / length[:, None]
    t_lo, t_hi = 0.25, 0.75
    inside = (r > t_lo + 1e-4) & (r < t_hi - 1e-4)
    near_end = ((np.abs(r - t_lo) <= 1e-4) | (np.abs(r - t_hi) <= 1e-4)).any(axis=1)
    usable = ~near_end & (multi["count"] <= mo.MAX_K)
    got = so.closest(arrays, a, b, (t_lo, t_hi))
    assert usable.mean() > 0.8 and inside.any(axis=1)[usable].mean() > 0.2
    assert np.array_equal(got["hit"].astype(bool)[usable], inside.any(axis=1)[usable])
    first = inside.argmax(axis=1)
    rows = np.flatnonzero(usable & inside.any(axis=1))
    assert np.array_equal(got["leaf"][rows], multi["leaf"][rows, first[rows]])
    assert np.array_equal(got["distance"][rows].view(np.uint32), multi["distance"][rows, first[rows]].view(np.uint32))


def test_odd_inputs_block_nothing_where_the_header_says_so(rt, scene_for):
    scene, arrays = scene_of(rt, scene_for, "blob", "longest")
    a, b, nothing = cases.odd_segments(arrays)
    assert nothing.sum() > 150
    some = False
    for interval in cases.INTERVALS + (cases.SURFACE_INTERVAL,) + cases.ODD_INTERVALS:
        got = so.closest(arrays, a, b, interval)
        assert np.array_equal(so.occluded(arrays, a, b, interval), got["hit"]), interval
        quiet = np.ones(len(a), bool) if cases.blocks_nothing(interval) else nothing
        assert not got["hit"][quiet].any(), interval
        assert np.isposinf(got["distance"][quiet]).all() and (got["leaf"][quiet] == so.NONE).all(), interval
        for f in ("barycentric", "position", "normal"):
            assert (got[f][quiet].view(np.uint32) == 0).all(), (interval, f)
        some |= bool(got["hit"].any())
    assert some
    # a far end at infinity is no ray: t_hi = +inf is
    ordinary_a, ordinary_b = cases.box_segments(arrays, 500, 12)
    assert so.occluded(arrays, ordinary_a, ordinary_b, (-1.0, np.inf)).sum() > so.occluded(arrays, ordinary_a, ordinary_b, (-1.0, 1.0)).sum()


def test_mask_form_of_the_oracle_is_the_pair_form(rt, scene_for):
    scene, arrays = scene_of(rt, scene_for, "blob", "sah")
    points, targets = cases.mask_inputs(arrays, 37, 45, seed=5)
    got = so.visibility(arrays, points, targets, cases.DEFAULT)
    pa, pb = cases.pairs_of(points, targets)
    flags = so.occluded(arrays, pa, pb, cases.DEFAULT).reshape(37, 45).astype(bool)
    assert np.array_equal(rt.unpack_visibility_mask(got["mask"], 45), flags)
    assert np.array_equal(got["count"], flags.sum(axis=1)) and np.array_equal(got["count"], cases.popcount(got["mask"]))
    assert flags.any() and not flags.all()
    assert (got["mask"][:, 1] >> 13 == 0).all()  # padding bits


def test_doctored_answers_are_reported(rt, scene_for):
    """A flipped flag, and the blocker swapped for a farther one, must each be named by the comparators."""
    scene, arrays = scene_of(rt, scene_for, "layered", "longest")
    a, b = box_segments("layered", arrays)
    interval = cases.INTERVALS[0]
    ref = reference("layered", scene, a, b, interval)
    good = so.closest(arrays, a, b, interval)
    assert not sr.compare_occluded(ref, good["hit"]).failures() and not sr.compare_closest(scene, ref, good).failures(tol=sr.TOL)
    judged = np.flatnonzero(ref["judged"] & ref["judged_any"])
    flipped = good["hit"].copy()
    flipped[judged[:10]] ^= 1
    rep = sr.compare_occluded(ref, flipped)
    assert rep["mismatches"]["occluded"] == 10 and rep.failures()
    # the second blocker of a segment that has two clearly apart: the multi-hit oracle's second slot inside the interval
    two = judged[(ref["count"][judged] >= 2) & (ref["distance"][judged, 1] > ref["distance"][judged, 0] + 1e-3)][:10]
    assert len(two) == 10
    o, d = sr.rays_of(a, b)
    multi = mo.multihit(arrays, o[two], d[two], np.inf, mo.MAX_K)
    swapped = {f: v.copy() for f, v in good.items()}
    for row, i in enumerate(two):
        slot = int(np.flatnonzero(multi["leaf"][row] == good["leaf"][i])[0]) + 1
        for f in ("distance", "leaf", "barycentric", "position", "normal"):
            swapped[f][i] = multi[f][row, slot]
    rep = sr.compare_closest(scene, ref, swapped)
    assert rep["mismatches"]["leaf"] == 10 and rep.failures(tol=sr.TOL), str(rep)
    # ... and a flipped `hit` of the closest form
    swapped = {f: v.copy() for f, v in good.items()}
    swapped["hit"][judged[:10]] ^= 1
    assert sr.compare_closest(scene, ref, swapped)["mismatches"]["hit"] == 10
