"""Two float64 truths for the SIGN of the signed distance queries (include/rt_hip_signed.h), and the comparator that holds
an answer's signs against them.  numpy float64 on the float32 inputs, over the mesh's faces in FILE order; no line is
shared with csrc/signed_point.h.

  (i)  The angle-weighted pseudonormal in float64: face normals by np.cross, corner angles by math.atan2(|a x b|, a . b),
       vertex and edge sums over dictionaries keyed by vertex ids.  For a point, the faces are
       distance_reference.pair_distances' nearest face set -- those within the (c) tolerance TOL["leaf"] * scale of the
       minimum --; for each of them the nearest point and the feature it lies on come from the plane projection and the
       three edges as parametrised segments, and the sign is that of (q - p) . N.  On a closed mesh the set agrees with
       itself; where it does not (coincident faces of an open mesh, unwelded duplicates) either sign is a nearest face's.
  (ii) For closed meshes, the generalised winding number: the sum of the faces' solid angles (Van Oosterom, Strackee) over
       4 pi, rounded.  Outward-oriented: 1 inside, 0 outside; reversed: -1 inside.

A point is judged unless the reference distance is below distance_reference's (b) tolerance TOL["distance"] * scale_of(q, d):
there the sign is the surface's own rounding.  At most EXCLUDED_CAP of a set may be left out that way.

MEASURED["angle"]: the worst |sp_angle - float64 angle| over the sweep of tests/test_signed_cpu.py (corner shapes from
equilateral to slivers of 1e-6), against THIS reference; the tolerance is 8 x it, as in distance_reference.py.
"""
import math

import numpy as np

import distance_reference as ref

MEASURED = {"angle": 2.5e-7}
TOL = {k: 8.0 * v for k, v in MEASURED.items()}
EXCLUDED_CAP = 0.01
ON_FEATURE = 1e-12  # a segment parameter this close to 0 or 1 is the vertex (float64, unit-sized meshes)


def angle64(a, b) -> float:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    c = np.cross(a, b)
    return math.atan2(math.sqrt(float(c @ c)), float(a @ b))


class Pseudonormals:
    """Face, edge and vertex pseudonormals of a mesh (file order), float64."""

    def __init__(self, vertices, faces):
        self.v = np.asarray(vertices, np.float64)[:, :3]
        self.f = np.asarray(faces, np.int64).reshape(-1, 3)
        tri = self.v[self.f]
        n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        length = np.linalg.norm(n, axis=1)
        self.face = np.where(length[:, None] > 0.0, n / np.where(length > 0.0, length, 1.0)[:, None], 0.0)
        self.vertex, self.edge = {}, {}
        for k, (a, b, c) in enumerate(self.f):
            ids = (int(a), int(b), int(c))
            for corner in range(3):
                x, y, z = ids[corner], ids[(corner + 1) % 3], ids[(corner + 2) % 3]
                w = angle64(self.v[y] - self.v[x], self.v[z] - self.v[x]) if length[k] > 0.0 else 0.0
                self.vertex[x] = self.vertex.get(x, np.zeros(3)) + w * self.face[k]
                key = (min(x, y), max(x, y))
                self.edge[key] = self.edge.get(key, np.zeros(3)) + self.face[k]

    def edges(self):
        return sorted(self.edge)

    def of_nearest(self, q, face: int):
        """(nearest point of `face` to q, its pseudonormal, "vertex" | "edge" | "face")."""
        ids = [int(i) for i in self.f[face]]
        a, b, c = self.v[ids]
        n = self.face[face]
        if n.any():
            foot = q - n * float((q - a) @ n)
            area = float(np.cross(b - a, c - a) @ n)
            wa, wb, wc = (float(np.cross(b - foot, c - foot) @ n) / area, float(np.cross(c - foot, a - foot) @ n) / area,
                          float(np.cross(a - foot, b - foot) @ n) / area)
            if min(wa, wb, wc) > ON_FEATURE:
                return foot, n, "face"
        best = None
        for i, j in ((0, 1), (0, 2), (1, 2)):
            x, y = self.v[ids[i]], self.v[ids[j]]
            d = y - x
            t = min(1.0, max(0.0, float((q - x) @ d) / float(d @ d))) if d.any() else 0.0
            p = x + t * d
            dist = float(np.linalg.norm(q - p))
            if best is None or dist < best[0]:
                if t <= ON_FEATURE:
                    best = (dist, p, self.vertex[ids[i]], "vertex")
                elif t >= 1.0 - ON_FEATURE:
                    best = (dist, p, self.vertex[ids[j]], "vertex")
                else:
                    best = (dist, p, self.edge[(min(ids[i], ids[j]), max(ids[i], ids[j]))], "edge")
        return best[1], best[2], best[3]


def pseudonormal_inside(points, vertices, faces, pairs=None, normals: Pseudonormals = None):
    """Truth (i): (inside by the first nearest face: bool (N,), the nearest face set disagrees with itself: bool (N,), feature
    class per point: list of str, reference distance (N,))."""
    q = np.asarray(points, np.float64)[:, :3]
    pn = normals or Pseudonormals(vertices, faces)
    d = ref.pair_distances(q, vertices, faces) if pairs is None else pairs
    least = d.min(axis=1)
    near = d <= (least + ref.TOL["leaf"] * ref.scale_of(q, least))[:, None]
    inside, split, kinds = np.zeros(len(q), bool), np.zeros(len(q), bool), []
    for i in range(len(q)):
        signs = []
        for face in np.flatnonzero(near[i]):
            p, n, kind = pn.of_nearest(q[i], int(face))
            signs.append(float((q[i] - p) @ n) < 0.0)
            if len(signs) == 1:
                kinds.append(kind)
        inside[i], split[i] = signs[0], len(set(signs)) > 1
    return inside, split, kinds, least


def winding_number(points, vertices, faces) -> np.ndarray:
    """Truth (ii): float64 (N,), the generalised winding number before rounding."""
    q = np.asarray(points, np.float64)[:, :3]
    v = np.asarray(vertices, np.float64)[:, :3]
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    out = np.zeros(len(q))
    for first in range(0, len(q), 512):
        a = v[f[:, 0]][None] - q[first:first + 512, None]
        b = v[f[:, 1]][None] - q[first:first + 512, None]
        c = v[f[:, 2]][None] - q[first:first + 512, None]
        la, lb, lc = np.linalg.norm(a, axis=2), np.linalg.norm(b, axis=2), np.linalg.norm(c, axis=2)
        num = (a * np.cross(b, c)).sum(axis=2)
        den = la * lb * lc + (a * b).sum(axis=2) * lc + (b * c).sum(axis=2) * la + (c * a).sum(axis=2) * lb
        out[first:first + 512] = (2.0 * np.arctan2(num, den)).sum(axis=1) / (4.0 * math.pi)
    return out


def compare(points, vertices, faces, inside, closed: bool, reversed_: bool = False, pairs=None, normals: Pseudonormals = None) -> dict:
    """Holds `inside` (bool (N,): the answer's distance is negative) against truth (i) and, for a closed mesh, truth (ii).
    `vertices`, `faces`: the mesh as ANSWERED (a reversed mesh is given reversed, with reversed_ True: truth (i) follows the
    faces as they are, truth (ii) says -1 inside and the oracle calls the outside inside).
    {"violations": [...], "excluded": share left out, "judged": count, "kinds": per point}."""
    q = np.asarray(points, np.float64)[:, :3]
    first, split, kinds, distance = pseudonormal_inside(q, vertices, faces, pairs=pairs, normals=normals)
    judged = distance >= ref.TOL["distance"] * ref.scale_of(q, distance)
    violations = []
    inside = np.asarray(inside, bool)
    if closed and (split & judged).any():
        violations.append(f"(i) the nearest faces of point {np.flatnonzero(split & judged)[0]} disagree about the side: the mesh is not closed")
    for i in np.flatnonzero(judged & (inside != first) & ~split)[:5]:
        violations.append(f"(i) point {i} ({kinds[i]}): inside {bool(inside[i])}, the float64 pseudonormal says {bool(first[i])}")
    if closed:
        w = winding_number(q[judged], vertices, faces)
        whole = np.rint(w)
        if np.abs(w - whole).max(initial=0.0) > 1e-9:
            violations.append(f"(ii) a winding number {np.abs(w - whole).max():.3g} from an integer: the mesh is not closed")
        truly_inside = whole != 0
        assert set(np.unique(whole)) <= ({0.0, -1.0} if reversed_ else {0.0, 1.0}), np.unique(whole)
        want = ~truly_inside if reversed_ else truly_inside  # (a reversed mesh's normals point inward)
        rows = np.flatnonzero(judged)
        for k in np.flatnonzero(inside[judged] != want)[:5]:
            violations.append(f"(ii) point {rows[k]} ({kinds[rows[k]]}): inside {bool(inside[rows[k]])}, winding number {whole[k]:+.0f}")
    excluded = 1.0 - judged.mean() if len(q) else 0.0
    if excluded > EXCLUDED_CAP:
        violations.append(f"{excluded:.4f} of the set lies within the distance tolerance of the surface (cap {EXCLUDED_CAP})")
    return {"violations": violations, "excluded": float(excluded), "judged": int(judged.sum()), "kinds": kinds,
            "split": int((split & judged).sum())}
