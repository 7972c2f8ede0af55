"""Geometric ground truth for the instanced multi-hit queries (include/rt_hip_instance_multihit.h): instance_reference's
float64 answer -- every ray against every triangle of every instance, no tree of either level, no float32 arithmetic, no C --
with RT_MULTIHIT_MAX_K + 1 slots kept, and the comparator of a multi-hit answer with an instance per slot.  TEST
INFRASTRUCTURE ONLY.

What is judged, what a pair is and how the pairs of all instances are merged -- by (distance, instance, file-order face) -- are
instance_reference's, restated here with the slots as a parameter (that module keeps four).  The tolerances are
instance_reference.TOL, the project's figure for instanced records (8 x the measured oracle - reference).
"""
import numpy as np

import geometry_reference as gr
import instance_reference as ir

KEEP = gr.KEEP  # 17: RT_MULTIHIT_MAX_K and one more (the neighbour of slot 15)
TOL = ir.TOL
RECORD_FIELDS = ("count", "distance", "leaf", "barycentric", "position", "normal")


def instanced(scene, transforms, origins, directions, max_distance, keep: int = KEEP) -> dict:
    """instance_reference.instanced's answer with `keep` slots: {"count", "judged": (N,), "distance", "face", "instance":
    (N, keep), "barycentric", "position", "normal": (N, keep, 3)}."""
    m = gr.mesh_of(scene)
    W = np.asarray(transforms, np.float32).astype(np.float64)
    inverse = [np.linalg.inv(w[:, :3]) for w in W]
    o = np.asarray(origins, np.float32)[:, :3].astype(np.float64)
    d = np.asarray(directions, np.float32)[:, :3].astype(np.float64)
    n = o.shape[0]
    out = {"count": np.zeros(n, np.uint32), "judged": np.zeros(n, bool), "distance": np.full((n, keep), np.inf),
           "face": np.full((n, keep), gr.NONE, np.uint32), "instance": np.full((n, keep), gr.NONE, np.uint32),
           "barycentric": np.zeros((n, keep, 3)), "position": np.zeros((n, keep, 3)), "normal": np.zeros((n, keep, 3))}
    scope = gr.in_scope(o, d)
    dlen = np.linalg.norm(d, axis=1)
    inv_all = np.stack(inverse)

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
        kept = slot < keep
        rows, cols, inst, rr, ss, tt, dist, slot = (x[kept] for x in (rows, cols, inst, rr, ss, tt, dist, slot))
        g = rows + i0
        out["distance"][g, slot] = dist
        out["face"][g, slot] = cols
        out["instance"][g, slot] = inst
        wgt = np.stack([1.0 - ss - tt, ss, tt], axis=1)
        out["barycentric"][g, slot] = wgt
        out["position"][g, slot] = oc[rows] + rr[:, None] * dc[rows]
        f = m.faces[cols]
        raw = wgt[:, 0, None] * m.vnormals[f[:, 0]] + wgt[:, 1, None] * m.vnormals[f[:, 1]] + wgt[:, 2, None] * m.vnormals[f[:, 2]]
        nrm = np.einsum("nji,nj->ni", inv_all[inst], raw)  # transpose(inverse) raw
        with np.errstate(all="ignore"):
            out["normal"][g, slot] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)

    gr._map(work, gr._chunks(n, len(m.faces)))  # (a chunk's pairs are one instance's at a time)
    return out


def compare_multihit(scene, ref: dict, got: dict, k: int, tol=None) -> gr.Report:
    """An instanced multi-hit answer in the library's form (k slots, "instance" beside the record's fields) against
    instanced(), on the judged rays: geometry_reference.compare_multihit's checks -- the count, the fill values, every used
    slot a reference pair's face within the distance tolerance of the reference's slot, the float fields against that pair --
    with the INSTANCE part of what a slot must match, the instance's fill value, and the contract's order (distance, instance,
    leaf) on the answer itself."""
    tol = TOL if tol is None else tol
    j = ref["judged"]
    n_ref = np.minimum(ref["count"], k)
    count = np.asarray(got["count"])
    mism = {"count": int((count != ref["count"])[j].sum())}
    ok = j & (count == ref["count"])  # the slots are compared where the counts agree
    used = (np.arange(k)[None, :] < n_ref[:, None]) & ok[:, None]
    free = (np.arange(k)[None, :] >= n_ref[:, None]) & ok[:, None]
    leaf = np.asarray(got["leaf"], np.uint32).reshape(-1, k)
    inst = np.asarray(got["instance"], np.uint32).reshape(-1, k)
    gd = np.asarray(got["distance"], np.float64).reshape(-1, k)
    fill_bad = free & ~((leaf == gr.NONE) & (inst == gr.NONE) & np.isposinf(gd))
    for f in ("barycentric", "position", "normal"):
        fill_bad |= free & (np.asarray(got[f]).reshape(-1, k, 3) != 0).any(axis=2)
    mism["fill"] = int(fill_bad.sum())
    mism["unused_slot"] = int((used & ((leaf == gr.NONE) | (inst == gr.NONE))).sum())
    face = scene.face_of_leaf(leaf.reshape(-1)).reshape(-1, k)
    rd = ref["distance"]
    with np.errstate(invalid="ignore"):
        near = np.abs(rd[:, None, :] - rd[:, :k, None]) <= tol["distance"] * np.maximum(1.0, rd[:, :k, None])
    same_face = near & (ref["face"][:, None, :] == face[:, :, None]) & (face[:, :, None] != gr.NONE)
    match = same_face & (ref["instance"][:, None, :] == inst[:, :, None])
    mism["leaf"] = int((used & ~same_face.any(axis=2)).sum())
    found = match.any(axis=2)
    mism["instance"] = int((used & same_face.any(axis=2) & ~found).sum())
    at = np.where(found, match.argmax(axis=2), np.arange(k)[None, :])  # the reference slot a slot stands for
    rows = np.arange(len(rd))[:, None]
    cmp = used & found
    rdist = rd[rows, at]
    scale = np.maximum(1.0, np.where(cmp, rdist, 1.0))
    worst = {}
    with np.errstate(invalid="ignore"):
        worst["distance"] = gr._worst((np.abs(gd - rdist) / scale)[cmp])
        for f in ("barycentric", "position", "normal"):
            delta = np.abs(np.asarray(got[f], np.float64).reshape(-1, k, 3) - ref[f][rows, at]).max(axis=2)
            worst[f] = gr._worst((delta / scale if f == "position" else delta)[cmp])
    if k > 1:
        both = used[:, :-1] & used[:, 1:]
        a, b = inst.astype(np.int64), leaf.astype(np.int64)
        lower = (a[:, :-1] < a[:, 1:]) | ((a[:, :-1] == a[:, 1:]) & (b[:, :-1] < b[:, 1:]))
        asc = (gd[:, :-1] < gd[:, 1:]) | ((gd[:, :-1] == gd[:, 1:]) & lower)
        mism["order"] = int((both & ~asc).sum())
    return gr.Report(rays=len(j), judged_share=float(j.mean()), hit_share=float((ref["count"] > 0).mean()), mismatches=mism, worst=worst)
