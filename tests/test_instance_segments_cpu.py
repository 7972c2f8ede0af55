"""CPU: the instanced segment queries' contract (include/rt_hip_instance_segments.h) -- the header, the library and the
binding; the C oracle (tests/instance_segment_oracle.c) against the BVH-free float64 reference
(tests/instance_segment_reference.py); the header's two relations, oracle against oracle; odd segments and odd intervals.
No GPU.

What is asserted: on judged segments the flags, faces and instances are equal and the float fields lie within
instance_segment_reference.TOL (instance_reference.TOL, but for the barycentrics: that module says why); at most 1 % of a
case's segments go unjudged.  Every case prints its shares and its worst difference
per field (pytest -s)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import instance_cases
import instance_oracle as io
import instance_segment_cases as cases
import instance_segment_oracle as iso
import instance_segment_reference as isr
import segment_oracle as so
import segment_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("rt_instances_segments_occluded", "rt_instances_segments_closest", "rt_instances_visibility_masks",
                "rt_instances_segments_occluded_device", "rt_instances_segments_closest_device",
                "rt_instances_visibility_masks_device")
METHODS = ("instances_segments_occluded", "instances_segments_closest", "instances_visibility")
MESHES = ("blob", "ties")
BVHS = ("longest", "sah")
N_BOX = 3000
MAX_UNJUDGED = 0.01
NONE = 0xFFFFFFFF
_REF = {}


def box_segments(plan, family):
    return cases.box_segments(plan["nodes"], N_BOX, seed=900 + instance_cases.FAMILIES.index(family))


def test_header_library_and_binding(rt):
    header = os.path.join(ROOT, "include", "rt_hip_instance_segments.h")
    assert os.path.exists(header), "include/rt_hip_instance_segments.h is missing"
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(ENTRY_POINTS)
    lib = C.CDLL(rt.lib_path())
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in rt.api._SIGNATURES, name
    plain = {"rt_instances_segments_occluded": "rt_segments_occluded", "rt_instances_segments_closest": "rt_segments_closest",
             "rt_instances_visibility_masks": "rt_visibility_masks"}
    for name, model in plain.items():  # argument order follows rt_hip_segment.h
        for suffix in ("", "_device"):
            assert rt.api._SIGNATURES[name + suffix] == rt.api._SIGNATURES[model + suffix], name + suffix
    mine = [m for m in dir(rt.Host) if m.startswith("instances_") and ("segments" in m or "visibility" in m)]
    assert sorted(mine) == sorted(METHODS)
    assert '#include "../oracle/rt_oracle.c"' in open(os.path.join(ROOT, "tests", "instance_segment_oracle.c")).read()
    # the paragraph of rt_hip_instances.h that lists the families names the new forms
    listing = open(os.path.join(ROOT, "include", "rt_hip_instances.h")).read()
    assert "rt_hip_instance_segments.h" in listing and "rt_instances_visibility_masks" in listing


@pytest.mark.parametrize("interval", cases.INTERVALS)
@pytest.mark.parametrize("family", instance_cases.FAMILIES)
@pytest.mark.parametrize("bvh", BVHS)
@pytest.mark.parametrize("mesh", MESHES)
def test_oracle_against_the_reference(rt, scene_for, mesh, bvh, family, interval):
    scene, arrays = scene_for(mesh, bvh)
    W = instance_cases.family(family, arrays)
    plan = cases.plan_for(rt, arrays, W)
    a, b = box_segments(plan, family)
    key = (mesh, family, float(interval[0]), float(interval[1]))
    if key not in _REF:  # (the reference knows no tree: one answer for both builders)
        _REF[key] = isr.segments(scene, W, a, b, interval)
        for v in _REF[key].values():
            v.setflags(write=False)
    ref = _REF[key]
    what = f"{mesh}/{bvh} {family} ({len(W)} instances) interval {interval}"
    blocked, open_, unsure = ref["blocked"].mean(), ref["open"].mean(), 1.0 - ref["judged_any"].mean()
    print(f"INSTANCE SEGMENTS {what}: reference shares: blocked {blocked:.4f}, open {open_:.4f}, borderline {unsure:.4f}; "
          f"closest judged {ref['judged'].mean():.4f}")
    assert blocked >= 0.05 and open_ >= 0.05, (what, blocked, open_)  # (both answers are populated)
    got = iso.closest(arrays, plan, a, b, interval)
    occ = iso.occluded(arrays, plan, a, b, interval)
    assert np.array_equal(occ, got["hit"]), what
    for rep in (isr.compare_occluded(ref, occ), isr.compare_closest(scene, ref, got)):
        print(f"INSTANCE SEGMENTS {what}: {rep}")
        bad = rep.failures(tol=isr.TOL, max_unjudged=MAX_UNJUDGED)
        assert not bad, (what, bad)
    if family == "tie_pair":
        assert (got["instance"][got["hit"].astype(bool)] == 0).all()
    # without a blocker: the fill values, word for word
    free = ~got["hit"].astype(bool)
    assert np.isposinf(got["distance"][free]).all() and (got["leaf"][free] == NONE).all() and (got["instance"][free] == NONE).all()
    for f in ("barycentric", "position", "normal"):
        assert (got[f][free].view(np.uint32) == 0).all(), (what, f)


def without_negative_zero(a, b):
    """The segments of the identity relation: a and b - a finite, no -0 in either."""
    o, d = sr.rays_of(a, b)
    ok = np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & ~(np.signbit(o) & (o == 0)).any(axis=1) & ~(np.signbit(d) & (d == 0)).any(axis=1)
    return np.ascontiguousarray(np.asarray(a)[ok]), np.ascontiguousarray(np.asarray(b)[ok])


def test_identity_relation_on_the_oracles(rt, scene_for):
    """One identity instance, a and b - a finite without -0: the instanced oracle is the segment oracle; word for word where
    the blocker's distance is below +inf, with instance 0."""
    for mesh in MESHES:
        for bvh in BVHS:
            _, arrays = scene_for(mesh, bvh)
            W = instance_cases.family("identity", arrays)
            plan = cases.plan_for(rt, arrays, W)
            assert np.array_equal(plan["object_from_world"][0], np.eye(3, 4, dtype=np.float32))
            a, b = cases.box_segments(plan["nodes"], N_BOX, seed=811)
            oa, ob, _ = cases.odd_segments(arrays)
            a, b = without_negative_zero(np.concatenate([a, oa]), np.concatenate([b, ob]))
            for interval in cases.INTERVALS + (cases.SURFACE_INTERVAL,):
                got = iso.closest(arrays, plan, a, b, interval)
                want = so.closest(arrays, a, b, interval)
                assert np.array_equal(iso.occluded(arrays, plan, a, b, interval), so.occluded(arrays, a, b, interval)), (mesh, bvh, interval)
                assert np.array_equal(got["hit"], want["hit"]) and want["hit"].any()
                at = want["distance"] < np.inf
                for f in so.FIELDS:
                    assert iso.same_words(got[f][at], want[f][at]).all(), (mesh, bvh, interval, f)
                assert (got["instance"][at] == 0).all()


def test_relation_to_the_instanced_ray_queries(rt, scene_for):
    """t_lo < 0, t_hi = +inf: the occluded form is the instanced ray oracle's of (a, b - a) with max_distance +inf, and where
    that ray's closest hit has a distance below +inf the closest form is its record, word for word."""
    for mesh in MESHES:
        for bvh in BVHS:
            _, arrays = scene_for(mesh, bvh)
            for family in ("rotations", "shear", "overlap_pair", "grid"):
                plan = cases.plan_for(rt, arrays, instance_cases.family(family, arrays))
                a, b = box_segments(plan, family)
                o, d = sr.rays_of(a, b)
                want = io.closest(arrays, plan, o, d, np.inf)
                want_occluded = io.occluded(arrays, plan, o, d, np.inf)
                assert want["hit"].any()
                at = want["distance"] < np.inf
                for t_lo in (-1.0, -np.inf, -1e-30):
                    got = iso.closest(arrays, plan, a, b, (t_lo, np.inf))
                    assert np.array_equal(iso.occluded(arrays, plan, a, b, (t_lo, np.inf)), want_occluded), (mesh, bvh, family)
                    assert np.array_equal(got["hit"], want["hit"])
                    for f in iso.FIELDS:
                        assert iso.same_words(got[f][at], want[f][at]).all(), (mesh, bvh, family, f)


@pytest.mark.parametrize("family", ("tie_pair", "shear", "identity", "grid"))
def test_odd_inputs_block_nothing_where_the_header_derives_it(rt, scene_for, family):
    _, arrays = scene_for("blob", "longest")
    plan = cases.plan_for(rt, arrays, instance_cases.family(family, arrays))
    a, b, _ = cases.odd_segments(arrays)
    some = False
    for interval in cases.INTERVALS + (cases.SURFACE_INTERVAL,) + cases.ODD_INTERVALS:
        got = iso.closest(arrays, plan, a, b, interval)
        assert np.array_equal(iso.occluded(arrays, plan, a, b, interval), got["hit"]), interval
        quiet = cases.nothing_blocks(a, b, plan["nodes"], interval)
        assert quiet.sum() > 150
        assert not got["hit"][quiet].any(), (interval, np.flatnonzero(got["hit"].astype(bool) & quiet)[:5])
        assert np.isposinf(got["distance"][quiet]).all() and (got["leaf"][quiet] == NONE).all() and (got["instance"][quiet] == NONE).all()
        for f in ("barycentric", "position", "normal"):
            assert (got[f][quiet].view(np.uint32) == 0).all(), (interval, f)
        some |= bool(got["hit"].any())
    assert some


def test_mask_expectation_is_the_pair_form(rt, scene_for):
    """mask_of, the mask form's expectation: bit layout, padding and counts, on the occluded pair form."""
    _, arrays = scene_for("blob", "sah")
    plan = cases.plan_for(rt, arrays, instance_cases.family("rotations", arrays))
    points, targets = cases.box_points(plan["nodes"], 37, 5), cases.box_points(plan["nodes"], 45, 6)
    want = iso.mask_of(arrays, plan, points, targets, cases.INTERVALS[0])
    assert want["mask"].shape == (37, 2) and np.array_equal(rt.unpack_visibility_mask(want["mask"], 45), want["flags"])
    for i, j in ((0, 0), (3, 31), (7, 32), (36, 44)):
        one = iso.occluded(arrays, plan, points[i:i + 1], targets[j:j + 1], cases.INTERVALS[0])[0]
        assert bool(want["mask"][i, j >> 5] >> (j & 31) & 1) == bool(one)
    assert np.array_equal(want["count"], want["flags"].sum(axis=1)) and want["flags"].any() and not want["flags"].all()
    assert (want["mask"][:, 1] >> 13 == 0).all()  # padding bits
