"""CPU: is the margin of the top-level leaf boxes (csrc/instances.cc, instance_margin) enough?  test_planner checks that the
library computes the formula; this sweep checks the formula, on the sets that push its terms (instance_cases.HARD_FAMILIES,
with `shear` and `grid`) and with rays made to graze the boxes (instance_cases.margin_rays).

The property, in the contract's own binary32 arithmetic: no top-level box culls a copy in which the lane would have found
a hit clearly inside a triangle.  It is stated with two plans of the same set (instance_cases.margin_plans): `real`, the
boxes the library makes, and `open`, whose boxes are (-inf, +inf) so that every copy is entered.  Both answers come from the
C oracle (tests/instance_oracle.c), whose tie rule (distance, instance, leaf) makes the `open` answer independent of its
tree's shape.  C is the set of rays whose `open` answer is a hit at a finite distance with every returned barycentric
>= B = geometry_reference.M, the project's "clearly inside" margin, here applied to the lane's own binary32 barycentrics.  On
C the `real` closest answer must equal the `open` one word for word and `real` occluded must be 1: with max_distance 3e38
(the box and sign clauses of the slab test alone) and with max_distance = 2 r per ray (the t_min < max_distance clause).

The float64 comparator (tests/instance_reference.py) is NOT applied to these sets: its thresholds were measured on
well-conditioned maps, and legitimate binary32 differences exceed them when the inverse's entries are large."""
import ctypes as C

import numpy as np
import pytest

import geometry_reference as gr
import instance_cases as cases
import instance_oracle as io
from test_instances_cpu import check_tree

MESHES = ("blob", "single", "ties")
BVHS = ("longest", "sah")
SWEPT = cases.HARD_FAMILIES + ("shear", "grid")
N_RAYS = 6000
B = gr.M
FAR = 3e38
LEAST_C = 1000      # |C| per (mesh, family) at N_RAYS rays
LEAST_OF_GRID = 60  # instances of `grid` (125 copies) that are the hit of a ray of C; every other family: all of them


def closest_each(arrays, plan, o, d, max_distance, rows):
    """io.closest and io.occluded for the rays `rows`, each with a max_distance of its own: one call per ray."""
    nodes, inverse = io._plan(plan)
    o4, d4 = io.as4(o), io.as4(d)
    n = len(o4)
    out = {"hit": np.zeros(n, np.uint8), "distance": np.zeros(n, np.float32), "leaf": np.zeros(n, np.uint32),
           "barycentric": np.zeros((n, 3), np.float32), "position": np.zeros((n, 3), np.float32),
           "normal": np.zeros((n, 3), np.float32), "instance": np.zeros(n, np.uint32)}
    occluded = np.zeros(n, np.uint8)
    lib, scene = io.lib(), arrays.c_struct()
    at = [(out[f].ctypes.data, out[f].strides[0]) for f in io.FIELDS]
    for i in rows:
        i = int(i)
        rays = (o4.ctypes.data + 16 * i, d4.ctypes.data + 16 * i, 1, float(max_distance[i]))
        lib.io_closest(C.byref(scene), nodes.ctypes.data, len(nodes), inverse.ctypes.data, *rays, *[p + s * i for p, s in at])
        lib.io_occluded(C.byref(scene), nodes.ctypes.data, len(nodes), inverse.ctypes.data, *rays, occluded.ctypes.data + i)
    return out, occluded


def slab_report(plan, count, o, d, instance):
    """The slab parameters of one ray at one instance's leaf box, as box_hit forms them, in numpy binary32."""
    lo, hi = cases.leaf_boxes(plan["nodes"], count)
    lo, hi = lo[instance].astype(np.float32), hi[instance].astype(np.float32)
    with np.errstate(all="ignore"):
        div = np.float32(1.0) / d
        t_lo, t_hi = (lo - o) * div, (hi - o) * div
    near, far = np.where(div >= 0, t_lo, t_hi), np.where(div >= 0, t_hi, t_lo)
    return {"lo": lo.tolist(), "hi": hi.tolist(), "near": near.tolist(), "far": far.tolist()}


def offenders(what, real_plan, count, o, d, C_rows, opened, real, occluded, max_distance=None):
    """The rays of C on which the real plan's answer is not the open plan's, the first five described."""
    same = np.ones(len(o), bool)
    for f in io.FIELDS:
        ok = io.same_words(real[f], opened[f])
        same &= ok if ok.ndim == 1 else ok.all(axis=1)
    bad = np.flatnonzero(C_rows & ~(same & (occluded == 1)))
    lines = []
    for i in bad[:5]:
        k = int(opened["instance"][i])
        lines.append({"case": what, "ray": int(i), "instance": k, "origin": cases.ORIGIN_CLASSES[int(cases.origin_class(len(o))[i])],
                      "o": o[i].tolist(), "d": d[i].tolist(), "open distance": float(opened["distance"][i]),
                      "open barycentric": opened["barycentric"][i].tolist(), "real hit": int(real["hit"][i]),
                      "real instance": int(real["instance"][i]), "real occluded": int(occluded[i]),
                      "max_distance": None if max_distance is None else float(max_distance[i]), **slab_report(real_plan, count, o[i], d[i], k)})
    return bad, lines


def sweep(rt, arrays, family, what, n=N_RAYS):
    """Both passes for one scene and one family: {"C", "C2", "instances", "classes", "bad", "bad2", "lines"}."""
    W = cases.family(family, arrays)
    real_plan, open_plan = cases.margin_plans(rt, arrays, W)
    check_tree(real_plan["nodes"], len(W))
    check_tree(open_plan["nodes"], len(W))
    o, d = cases.margin_rays(arrays, real_plan, W, n, seed=4100 + SWEPT.index(family))
    opened = io.closest(arrays, open_plan, o, d, FAR)
    real, occluded = io.closest(arrays, real_plan, o, d, FAR), io.occluded(arrays, real_plan, o, d, FAR)
    C_rows = cases.clearly_inside(opened, B)
    bad, lines = offenders(what, real_plan, len(W), o, d, C_rows, opened, real, occluded)
    # the second pass: max_distance = 2 r, r the open hit's parameter (its distance over the direction's length)
    r = opened["distance"].astype(np.float64) / np.linalg.norm(d.astype(np.float64), axis=1)
    max_distance = np.where(C_rows, 2.0 * r, 0.0).astype(np.float32)
    rows = np.flatnonzero(C_rows)
    opened2, _ = closest_each(arrays, open_plan, o, d, max_distance, rows)
    real2, occluded2 = closest_each(arrays, real_plan, o, d, max_distance, rows)
    C2_rows = C_rows & cases.clearly_inside(opened2, B)
    bad2, lines2 = offenders(what + " max_distance 2r", real_plan, len(W), o, d, C2_rows, opened2, real2, occluded2, max_distance)
    return {"C": int(C_rows.sum()), "C2": int(C2_rows.sum()), "count": len(W), "instances": len(np.unique(opened["instance"][C_rows])),
            "classes": sorted(set(cases.origin_class(n)[C_rows].tolist())), "bad": len(bad), "bad2": len(bad2), "lines": lines + lines2}


@pytest.mark.parametrize("family", SWEPT)
@pytest.mark.parametrize("bvh", BVHS)
@pytest.mark.parametrize("mesh", MESHES)
def test_no_box_culls_a_clear_hit(rt, scene_for, mesh, bvh, family):
    _, arrays = scene_for(mesh, bvh)
    what = f"{mesh}/{bvh} {family}"
    got = sweep(rt, arrays, family, what)
    print(f"MARGIN {what}: |C| = {got['C']} of {N_RAYS} (second pass {got['C2']}), instances hit {got['instances']} of {got['count']}, "
          f"origin classes {got['classes']}, violations {got['bad']} + {got['bad2']}")
    # no case passes on emptiness
    assert got["C"] >= LEAST_C and got["C2"] >= LEAST_C, (what, got["C"], got["C2"])
    assert got["instances"] >= (LEAST_OF_GRID if family == "grid" else got["count"]), (what, got["instances"], got["count"])
    assert got["classes"] == [0, 1, 2], (what, got["classes"])
    assert got["bad"] == 0 and got["bad2"] == 0, (what, got["bad"], got["bad2"], got["lines"])


def test_hard_families_are_what_they_say(rt, scene_for):
    """The singular-value ratios, the negative determinant, the scales and the distances the families are named for."""
    _, arrays = scene_for("blob", "longest")
    lo, hi = cases.mo.box_of(arrays)
    centre, diag = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    ill = cases.family("ill", arrays).astype(np.float64)
    s = np.linalg.svd(ill[:, :, :3], compute_uv=False)
    assert np.allclose(sorted(s[:, 0] / s[:, 2]), [1e2, 1e2, 1e3, 1e4, 1e4], rtol=1e-3)
    assert (np.linalg.det(ill[:, :, :3]) < 0).sum() == 1
    far_ill = cases.family("far_ill", arrays).astype(np.float64)
    assert np.allclose(np.linalg.svd(far_ill[:, :, :3], compute_uv=False)[:, 0] / s[:, 0], 1.0, rtol=1e-3)
    moved = np.linalg.norm(np.einsum("nij,j->ni", far_ill[:, :, :3], centre) + far_ill[:, :, 3] - centre, axis=1) / diag
    assert (moved > 900).all() and (moved < 1300).all()
    tiny_huge = cases.family("tiny_huge", arrays).astype(np.float64)
    assert np.allclose(np.linalg.svd(tiny_huge[:, :, :3], compute_uv=False)[:, 0], [1e-3, 1e-2, 1e2, 1e3], rtol=1e-3)
    for name, wanted in (("far", [1e2, 1e2, 1e3, 1e3, 1e4, 1e4]), ("wide", [0.0] + [1e4] * 6)):
        W = cases.family(name, arrays).astype(np.float64)
        assert np.allclose(np.linalg.svd(W[:, :, :3], compute_uv=False), 1.0, atol=1e-6)  # rigid
        moved = np.linalg.norm(np.einsum("nij,j->ni", W[:, :, :3], centre) + W[:, :, 3] - centre, axis=1) / diag
        assert np.allclose(moved, wanted, rtol=1e-3, atol=1e-6), (name, moved)
    for name in cases.HARD_FAMILIES:
        cases.margin_plans(rt, arrays, cases.family(name, arrays))  # (accepted by rt_instance_plan)
