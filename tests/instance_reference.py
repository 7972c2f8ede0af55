"""Geometric ground truth for the instanced ray queries (include/rt_hip_instances.h): every ray against every triangle of
every instance, in numpy float64, on geometry_reference.Mesh.  No tree of either level, no float32 arithmetic, no C.
TEST INFRASTRUCTURE ONLY.

The CPU oracle (tests/instance_oracle.c) walks both trees in the kernels' float32 arithmetic with the library's own rounded
inverses, so it can only say that kernel and oracle agree; this module says whether they are RIGHT wherever the answer does
not hang on a rounding.  Per instance the world ray (o, d), float32 inputs taken to float64, is mapped to the object's frame
with the BINARY64 inverse of the binary32 world_from_object (numpy's, not the library's formula), and
geometry_reference._pairs judges it against the mesh in file order: the contract's thresholds live in object space, and an
affine map keeps ray parameters, so `max_distance` is the call's.  A clearly accepted pair has the world position o + r d,
the distance r |d|, the barycentrics of the object-space test and the normal normalize(inverse-transpose raw).  The pairs of
all instances are merged by (distance, instance, file-order face).  A ray is JUDGED when none of its pairs, in any instance,
is borderline; geometry_reference's classes, Report and failures(max_unjudged=0.01) are taken over as they are.
"""
import numpy as np

import geometry_reference as gr

KEEP = 4  # slots kept per ray: the nearest, and neighbours for the comparator's look at ties

# Worst difference of each float field between the CPU oracle (tests/instance_oracle.c) and this reference over the cases of
# tests/test_instances_cpu.py (blob and ties, both builders, every family of tests/instance_cases.py, 3000 rays each, a
# max_distance of 1e5, 5 or 0.3 per case), printed by that file's tests; the measures are geometry_reference's (distance and
# position relative to max(1, distance)).  The factor 8 and its reason are geometry_reference's: the GPU's differences are
# the oracle's, the factor only absorbs another ray sample.
# Measured (rounded up to two digits), all four on blob's 5 x 5 x 5 grid, where a ray's origin lies several boxes away from the
# copy it hits and the rounding of the object ray's origin (an ulp of the WORLD coordinate) is large against the triangle:
# distance 1.93e-5, barycentric 1.79e-4, position 1.64e-5, normal 3.25e-5; the families of a few nearby copies stay within
# 3.8e-6, 1.1e-4, 2.9e-6, 1.7e-5.  That is 30 x, 9 x, 35 x and 5 x geometry_reference.MEASURED and outside its TOL, so this
# module has tolerances of its own.
MEASURED = {"distance": 2.0e-5, "barycentric": 1.8e-4, "position": 1.7e-5, "normal": 3.3e-5}
TOL = {f: 8.0 * v for f, v in MEASURED.items()}


def instanced(scene, transforms, origins, directions, max_distance) -> dict:
    """geometry_reference.multihit's answer over all instances, KEEP slots, and "instance" (N, KEEP) beside "face"."""
    m = gr.mesh_of(scene)
    W = np.asarray(transforms, np.float32).astype(np.float64)
    inverse = [np.linalg.inv(w[:, :3]) for w in W]
    o = np.asarray(origins, np.float32)[:, :3].astype(np.float64)
    d = np.asarray(directions, np.float32)[:, :3].astype(np.float64)
    n = o.shape[0]
    out = {"count": np.zeros(n, np.uint32), "judged": np.zeros(n, bool), "distance": np.full((n, KEEP), np.inf),
           "face": np.full((n, KEEP), gr.NONE, np.uint32), "instance": np.full((n, KEEP), gr.NONE, np.uint32),
           "barycentric": np.zeros((n, KEEP, 3)), "position": np.zeros((n, KEEP, 3)), "normal": np.zeros((n, KEEP, 3))}
    scope = gr.in_scope(o, d)
    dlen = np.linalg.norm(d, axis=1)

    def work(span):
        i0, i1 = span
        oc, dc = o[i0:i1], d[i0:i1]
        unsure = np.zeros(i1 - i0, bool)
        found = []
        for k, (w, inv) in enumerate(zip(W, inverse)):
            acc, bord, r, s, t = gr._pairs(m, (oc - w[:, 3]) @ inv.T, dc @ inv.T, max_distance)
            unsure |= bord.any(axis=1)
            rows, cols = np.nonzero(acc)
            found.append((rows, cols, np.full(len(rows), k), r[rows, cols], s[rows, cols], t[rows, cols]))
        out["judged"][i0:i1] = ~unsure & scope[i0:i1]
        rows, cols, inst, rr, ss, tt = (np.concatenate(x) for x in zip(*found))
        dist = rr * dlen[i0:i1][rows]
        order = np.lexsort((cols, inst, dist, rows))
        rows, cols, inst, rr, ss, tt, dist = (x[order] for x in (rows, cols, inst, rr, ss, tt, dist))
        count = np.bincount(rows, minlength=i1 - i0)
        out["count"][i0:i1] = count
        slot = np.arange(len(rows)) - (np.cumsum(count) - count)[rows]
        keep = slot < KEEP
        rows, cols, inst, rr, ss, tt, dist, slot = (x[keep] for x in (rows, cols, inst, rr, ss, tt, dist, slot))
        g = rows + i0
        out["distance"][g, slot] = dist
        out["face"][g, slot] = cols
        out["instance"][g, slot] = inst
        wgt = np.stack([1.0 - ss - tt, ss, tt], axis=1)
        out["barycentric"][g, slot] = wgt
        out["position"][g, slot] = oc[rows] + rr[:, None] * dc[rows]
        f = m.faces[cols]
        raw = wgt[:, 0, None] * m.vnormals[f[:, 0]] + wgt[:, 1, None] * m.vnormals[f[:, 1]] + wgt[:, 2, None] * m.vnormals[f[:, 2]]
        inv_all = np.stack(inverse) if len(inverse) else np.zeros((0, 3, 3))
        nrm = np.einsum("nji,nj->ni", inv_all[inst], raw)  # transpose(inverse) raw
        with np.errstate(all="ignore"):
            out["normal"][g, slot] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)

    gr._map(work, gr._chunks(n, len(m.faces)))  # (a chunk's pairs are one instance's at a time)
    return out


def compare_closest(scene, ref: dict, got: dict, tol=None) -> gr.Report:
    """A closest-form answer in the library's form against instanced(), on the judged rays: geometry_reference.compare_closest's
    checks, and the instance: it must be that of a reference slot with the answer's face within the distance tolerance of the
    nearest."""
    tol = TOL if tol is None else tol
    rep = gr.compare_closest(scene, ref, {f: got[f] for f in ("hit", "distance", "leaf", "barycentric", "position", "normal")}, tol)
    hit = np.asarray(got["hit"]).astype(bool)
    both = ref["judged"] & hit & (ref["count"] > 0)
    face = scene.face_of_leaf(np.ascontiguousarray(got["leaf"], np.uint32))
    rd = ref["distance"]
    with np.errstate(invalid="ignore"):
        near = np.abs(rd - rd[:, :1]) <= tol["distance"] * np.maximum(1.0, rd[:, :1])
    match = near & (ref["face"] == face[:, None]) & (ref["instance"] == np.asarray(got["instance"], np.uint32)[:, None])
    rep["mismatches"]["instance"] = int((both & ~match.any(axis=1)).sum())
    rep["mismatches"]["instance_fill"] = int((ref["judged"] & ~hit & (np.asarray(got["instance"]) != gr.NONE)).sum())
    return rep


def compare_occluded(ref: dict, got) -> gr.Report:
    return gr.compare_flags(ref, got, "occluded")
