"""Geometric ground truth for the segment queries (include/rt_hip_segment.h): every segment against every triangle of the
mesh in FILE order, in numpy float64, on geometry_reference.Mesh.  No BVH, no float32 arithmetic, no C.
TEST INFRASTRUCTURE ONLY.

The CPU oracle (tests/segment_oracle.c) walks the tree in the kernels' float32 arithmetic, so it can only say that kernel
and oracle agree; this module says whether they are RIGHT wherever the answer does not hang on a rounding.  It follows
geometry_reference's three-way verdict.  The segment (a, b) is the ray o = a, d = b - a -- the subtraction in float32, as
the contract makes it, everything after it in float64 -- and per (segment, triangle) pair geometry_reference._pairs gives
"clearly accepted", "clearly rejected" (which holds the term "the triangle's own box begins behind t_hi by the margin": its
max_distance is t_hi) or neither, and the plane parameter r.  With the margin on r of  M_R max(1, |r|)  the pair is
    clearly blocking      when  clearly accepted  and  t_lo + margin < r < t_hi - margin;
    clearly not blocking  when  clearly rejected,  or  r < t_lo - margin,  or  r > t_hi + margin;
    borderline            otherwise (a NaN anywhere lands here).
A segment is
    clearly blocked  when some pair is clearly blocking,
    clearly open     when every pair is clearly not blocking,
    borderline       otherwise,
and its closest record is judged only when none of its pairs is borderline.  Segments with a non-finite coordinate or of
no length are outside this reference (the odd-input tests own them).
"""
import numpy as np

import geometry_reference as gr

M_R = gr.M  # margin on the plane parameter, relative to max(1, |r|): 1e-4, the margin of the barycentrics
KEEP = 4    # blockers kept per segment: the nearest, and neighbours for the comparator's look at ties

# The closest record is compared within geometry_reference.TOL: the same arithmetic as a closest hit.  Measured on the cases
# of tests/test_segment_cpu.py (oracle against this reference; printed by its tests): distance 1.0e-6 (the surface endpoints;
# 6.1e-7 in the box), barycentric 2.2e-5, position 8.8e-7, normal 5.3e-6 -- up to 1.9 x geometry_reference.MEASURED and well
# inside its TOL = 8 x MEASURED (4.7e-6, 1.5e-4, 3.8e-6, 5.2e-5), so its tolerances stand.
TOL = gr.TOL


def rays_of(a, b):
    """(o, d) float32: o = a, d = b - a, one float32 subtraction per component."""
    a = np.asarray(a, np.float32)[:, :3]
    b = np.asarray(b, np.float32)[:, :3]
    d = b - a
    assert d.dtype == np.float32
    return np.ascontiguousarray(a), d


def segments(scene, a, b, interval) -> dict:
    """{"blocked": (N,) bool -- clearly blocked --, "open": (N,) bool -- clearly open --, "judged_any": blocked | open,
    "judged": (N,) bool, no pair borderline, "count": (N,) clearly blocking pairs, "distance" / "face": (N, KEEP),
    "barycentric" / "position" / "normal": (N, KEEP, 3): the first KEEP clearly blocking pairs by (distance, file-order
    face), distance = r |d|; unused slots hold +inf / NONE / 0.  Float fields are float64.}"""
    m = gr.mesh_of(scene)
    t_lo, t_hi = float(interval[0]), float(interval[1])
    o32, d32 = rays_of(a, b)
    o, d = o32.astype(np.float64), d32.astype(np.float64)
    n = o.shape[0]
    out = {"blocked": np.zeros(n, bool), "open": np.zeros(n, bool), "judged": np.zeros(n, bool), "count": np.zeros(n, np.uint32),
           "distance": np.full((n, KEEP), np.inf), "face": np.full((n, KEEP), gr.NONE, np.uint32),
           "barycentric": np.zeros((n, KEEP, 3)), "position": np.zeros((n, KEEP, 3)), "normal": np.zeros((n, KEEP, 3))}
    scope = gr.in_scope(o, d) & np.isfinite(np.asarray(b, np.float32)[:, :3]).all(axis=1)
    dlen = np.linalg.norm(d, axis=1)

    def work(span):
        i0, i1 = span
        oc, dc = o[i0:i1], d[i0:i1]
        acc, bord, r, s, t = gr._pairs(m, oc, dc, t_hi)
        rej = ~(acc | bord)
        with np.errstate(all="ignore"):
            margin = M_R * np.maximum(1.0, np.abs(r))
            blocking = acc & (r > t_lo + margin) & (r < t_hi - margin)
            not_blocking = rej | (r < t_lo - margin) | (r > t_hi + margin)
        unsure = ~(blocking | not_blocking)
        sc = scope[i0:i1]
        out["blocked"][i0:i1] = blocking.any(axis=1) & sc
        out["open"][i0:i1] = not_blocking.all(axis=1) & sc
        out["judged"][i0:i1] = ~unsure.any(axis=1) & sc
        rows, cols = np.nonzero(blocking)
        dist = r[rows, cols] * dlen[i0:i1][rows]
        order = np.lexsort((cols, dist, rows))
        rows, cols, dist = rows[order], cols[order], dist[order]
        count = np.bincount(rows, minlength=i1 - i0)
        out["count"][i0:i1] = count
        slot = np.arange(len(rows)) - (np.cumsum(count) - count)[rows]
        keep = slot < KEEP
        rows, cols, dist, slot = rows[keep], cols[keep], dist[keep], slot[keep]
        rr, ss, tt = r[rows, cols], s[rows, cols], t[rows, cols]
        g = rows + i0
        out["distance"][g, slot] = dist
        out["face"][g, slot] = cols
        w = np.stack([1.0 - ss - tt, ss, tt], axis=1)
        out["barycentric"][g, slot] = w
        out["position"][g, slot] = oc[rows] + rr[:, None] * dc[rows]
        f = m.faces[cols]
        nrm = w[:, 0, None] * m.vnormals[f[:, 0]] + w[:, 1, None] * m.vnormals[f[:, 1]] + w[:, 2, None] * m.vnormals[f[:, 2]]
        with np.errstate(all="ignore"):
            out["normal"][g, slot] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)

    gr._map(work, gr._chunks(n, len(m.faces)))
    out["judged_any"] = out["blocked"] | out["open"]
    return out


def compare_occluded(ref: dict, got) -> gr.Report:
    """An occlusion answer against segments(): on the clearly blocked and the clearly open segments."""
    j = ref["judged_any"]
    bad = int((np.asarray(got).astype(bool) != ref["blocked"])[j].sum())
    return gr.Report(rays=len(j), judged_share=float(j.mean()), hit_share=float(ref["blocked"].mean()), mismatches={"occluded": bad}, worst={})


def compare_closest(scene, ref: dict, got: dict, tol=None) -> gr.Report:
    """A closest-form answer in the library's form against segments(), on the segments none of whose pairs is borderline:
    geometry_reference.compare_closest's checks (the hit flag, the face within the distance tolerance of the nearest
    blocker, every float field, +inf / NONE / 0 without a blocker)."""
    return gr.compare_closest(scene, ref, got, TOL if tol is None else tol)
