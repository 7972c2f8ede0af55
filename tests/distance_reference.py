"""A BVH-free float64 reference for the closest-point queries (include/rt_hip_nearest.h) and the comparator that holds an
answer against it.  numpy float64 on the float32 inputs, over the mesh's faces in FILE order; it shares no line with the
library's routine: per (point, face) pair the distance is the minimum of the three edges as segments and, where the
point's projection onto the face's plane lies inside the face, the distance to that plane -- a face without area has no
such projection and is its edges, by construction.

The comparator needs no "unjudged" class.  Per point it checks
  (a) `hit` equals the reference's wherever the reference's distance is not within tolerance of max_distance,
  (b) `distance` is within tolerance of the reference's minimum,
  (c) the returned leaf -- through the leaf -> file-face map -- is a face whose OWN float64 distance is within tolerance of it,
  (d) `position` is the barycentric combination of that face's vertices,
  (e) the barycentrics are >= -tolerance and sum to 1,
  (f) |q - position| matches `distance`,
  (g) `normal` is the normalised barycentric combination of that face's vertex normals (where that has a length).
The reference's own nearest point is never compared: on shared edges and on the medial axis it is not unique.

Scaling as in DESIGN section 13: |delta| / max(1, distance, max |q_i|) for lengths, per component for barycentrics and normals.
MEASURED: the worst scaled difference between the C oracle (tests/nearest_oracle.c) and this reference over the CPU cases of
tests/test_nearest_cpu.py, per check; TOL = 8 x MEASURED -- the factor only absorbs another sample of points: the GPU is
held to the oracle bit for bit, and to this comparator with the same tolerances.
"""
import numpy as np

# check -> worst scaled difference measured (tests/test_nearest_cpu.py::test_oracle_against_the_reference prints them)
MEASURED = {
    # (b): `ties`, a query AT the apex of a sliver 0.8 long and 1e-5 high.  height^2 / edge^2 = 1.6e-10 lies below what the
    # binary32 uu, uv, vv resolve (2^-24): the routine's `vc` is rounding noise there, edge AB is taken before vertex C is
    # tried, and the answer is off by the sliver's height.  Without that face the worst is 7.9e-8 (interior_hard).
    "distance": 1.01e-5,
    "leaf": 1.8e-8,         # (c)
    "position": 4.1e-7,     # (d)
    "barycentric": 6.0e-8,  # (e): the sum's distance from 1 (no component was negative)
    "consistency": 1.1e-7,  # (f)
    "normal": 9.1e-8,       # (g)
}
TOL = {k: 8.0 * v for k, v in MEASURED.items()}


def _dot(x, y):
    return (x * y).sum(axis=-1)


def _segment_d2(q, a, b):
    """(N, F): squared distance from q (N, 1, 3) to the segments a-b ((1, F, 3) each); a segment without length is a."""
    ab = b - a
    length2 = _dot(ab, ab)
    t = np.where(length2 > 0.0, np.clip(_dot(q - a, ab) / np.where(length2 > 0.0, length2, 1.0), 0.0, 1.0), 0.0)
    e = q - (a + t[..., None] * ab)
    return _dot(e, e)


def pair_distances(points, vertices, faces, chunk: int = 0) -> np.ndarray:
    """float64 (N, F): the distance from every point to every face (faces: (F, 3) vertex ids)."""
    q_all = np.asarray(points, dtype=np.float64)[:, :3]
    v = np.asarray(vertices, dtype=np.float64)[:, :3]
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    a, b, c = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
    n = np.cross(b - a, c - a)
    nn = _dot(n, n)
    out = np.empty((q_all.shape[0], f.shape[0]))
    step = chunk or max(1, int(4e6 // max(1, f.shape[0])))
    with np.errstate(all="ignore"):
        for first in range(0, q_all.shape[0], step):
            q = q_all[first:first + step, None, :]
            d2 = np.minimum(np.minimum(_segment_d2(q, a, b), _segment_d2(q, a, c)), _segment_d2(q, b, c))
            w = q - a
            height = _dot(w, n)
            safe = np.where(nn > 0.0, nn, 1.0)
            foot = w - n * (height / safe)[..., None]  # the projection, relative to a
            wb = _dot(np.cross(foot, c - a), n) / safe
            wc = _dot(np.cross(b - a, foot), n) / safe
            inside = (nn > 0.0) & (wb >= 0.0) & (wc >= 0.0) & (wb + wc <= 1.0)
            d2 = np.where(inside, np.minimum(d2, height * height / safe), d2)
            out[first:first + step] = np.sqrt(d2)
    return out


def scale_of(points, distance) -> np.ndarray:
    q = np.abs(np.asarray(points, dtype=np.float64)[:, :3]).max(axis=1)
    d = np.where(np.isfinite(distance), distance, 0.0)
    return np.maximum(1.0, np.maximum(d, np.where(np.isfinite(q), q, 0.0)))


def compare(points, vertices, vnormals, faces, face_of_leaf, max_distance, answer: dict, tol: dict = None, pairs=None) -> dict:
    """Holds `answer` ({"hit", "distance", "leaf", "barycentric", "position", "normal"}) against the reference.  Returns
    {"violations": [text ...], "measured": {check: worst scaled difference}}.  `pairs`: pair_distances of the same points,
    vertices and faces where the caller has it already."""
    tol = TOL if tol is None else tol
    q = np.asarray(points, dtype=np.float64)[:, :3]
    v = np.asarray(vertices, dtype=np.float64)[:, :3]
    vn = np.asarray(vnormals, dtype=np.float64)[:, :3]
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    n = q.shape[0]
    usable = np.isfinite(q).all(axis=1) & bool(max_distance >= 0.0)
    d_all = pair_distances(np.where(usable[:, None], q, 0.0), v, f) if pairs is None else pairs
    d_min = d_all.min(axis=1)
    scale = scale_of(np.where(usable[:, None], q, 0.0), d_min)
    violations, measured = [], {k: 0.0 for k in MEASURED}
    hit = np.asarray(answer["hit"]).astype(bool)

    def report(check, rows, text):
        for i in np.flatnonzero(rows)[:5]:
            violations.append(f"({check}) point {i}: {text(i)}")

    # (a)
    md = float(max_distance)
    want = usable & (d_min <= md)
    near_radius = usable & np.isfinite(md) & (np.abs(d_min - md) <= tol["distance"] * scale)
    report("a", (hit != want) & ~near_radius, lambda i: f"hit {int(hit[i])}, reference distance {d_min[i]:.9g}, radius {md:.9g}")
    # without one: the empty record
    empty = ~hit
    bad_empty = empty & ~(np.isposinf(answer["distance"]) & (answer["leaf"] == 0xFFFFFFFF) & (answer["barycentric"] == 0).all(axis=1)
                          & (answer["position"] == 0).all(axis=1) & (answer["normal"] == 0).all(axis=1))
    report("a", bad_empty, lambda i: "not found, but the record is not the empty one")
    rows = np.flatnonzero(hit)
    if rows.size == 0:
        return {"violations": violations, "measured": measured}
    leaf = np.asarray(answer["leaf"])[rows].astype(np.int64)
    if (leaf >= len(face_of_leaf)).any():
        violations.append("(c) a leaf index beyond the scene's leaves")
        return {"violations": violations, "measured": measured}
    face = np.asarray(face_of_leaf, dtype=np.int64)[leaf]
    dist = np.asarray(answer["distance"], dtype=np.float64)[rows]
    bary = np.asarray(answer["barycentric"], dtype=np.float64)[rows]
    pos = np.asarray(answer["position"], dtype=np.float64)[rows]
    nrm = np.asarray(answer["normal"], dtype=np.float64)[rows]
    sc = scale[rows]

    def hold(check, diff, shown):
        measured[check] = max(measured[check], float(diff.max()))
        full = np.zeros(n, bool)
        full[rows[diff > tol[check]]] = True
        report({"distance": "b", "leaf": "c", "position": "d", "barycentric": "e", "consistency": "f", "normal": "g"}[check], full, shown)

    by_row = {int(r): k for k, r in enumerate(rows)}
    # (b)
    hold("distance", np.abs(dist - d_min[rows]) / sc, lambda i: f"distance {dist[by_row[i]]:.9g}, reference {d_min[i]:.9g}")
    # (c)
    own = d_all[rows, face]
    hold("leaf", np.abs(own - d_min[rows]) / sc, lambda i: f"face {face[by_row[i]]} lies at {own[by_row[i]]:.9g}, the nearest at {d_min[i]:.9g}")
    # (d)
    tri = v[f[face]]  # (R, 3, 3)
    combo = np.einsum("rk,rkc->rc", bary, tri)
    hold("position", np.abs(pos - combo).max(axis=1) / sc, lambda i: f"position {pos[by_row[i]]} is not the face's point {combo[by_row[i]]}")
    # (e)
    low = np.maximum(0.0, -bary.min(axis=1))
    hold("barycentric", np.maximum(low, np.abs(bary.sum(axis=1) - 1.0)), lambda i: f"barycentrics {bary[by_row[i]]}")
    # (f)
    hold("consistency", np.abs(np.linalg.norm(q[rows] - pos, axis=1) - dist) / sc,
         lambda i: f"|q - position| = {np.linalg.norm(q[i] - pos[by_row[i]]):.9g}, distance {dist[by_row[i]]:.9g}")
    # (g)
    blend = np.einsum("rk,rkc->rc", bary, vn[f[face]])
    length = np.linalg.norm(blend, axis=1)
    sure = length > 1e-6
    unit = blend / np.where(sure, length, 1.0)[:, None]
    hold("normal", np.where(sure, np.abs(nrm - unit).max(axis=1), 0.0), lambda i: f"normal {nrm[by_row[i]]}, of the face's normals {unit[by_row[i]]}")
    return {"violations": violations, "measured": measured}
