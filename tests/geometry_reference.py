"""Geometric ground truth for the ray, multi-hit and ambient-occlusion queries and the posed camera: every ray against
every triangle of the mesh in FILE order, in numpy float64.  No BVH, no float32 arithmetic on the hot path, no C.
TEST INFRASTRUCTURE ONLY.

The CPU oracles (tests/*_oracle.c) walk the same tree in the same float32 arithmetic as the kernels, so they can only
say that kernel and oracle agree.  This module says whether they are RIGHT, wherever the answer does not hang on a
rounding.  It reads scene.vertices, scene.faces and scene.vnormals -- never sorted_faces, nodes or aabbs -- and leaf
indices coming back from the library are mapped through scene.face_of_leaf() before they are compared, so that map
is under test too.

Per (ray, triangle) pair the contract of include/rt_hip_query.h / rt_hip_multihit.h is evaluated in float64 on the float32
inputs (dot products are written as matrix products, nothing else is rearranged):
    n = (B - A) x (C - A),  a = -n . (o - A),  b = n . d,  r = a / b,  ip = o + r d,  w = ip - A
    s = (uv wv - vv wu) / D,  t = (uv wu - uu wv) / D  with  uu = u.u, uv = u.v, vv = v.v, wu = w.u, wv = w.v, D = uv^2 - uu vv
    reported distance r |d|
    t_min: the slab entry of the triangle's own bounding box (min / max of its three float32 vertices) as a ray
    parameter, the direction NOT normalised.  "max_distance only culls BOXES" reduces to this box: every box contains
    its children (so an ancestor's t_min is never larger), and a leaf's box is its triangle's bounds; both are asserted
    in tests/test_geometry_cpu.py.
and the pair is
    clearly accepted  when  |b| >= 1e-6 (1 + M),  a sign(b) >= M_A |n| L  (L = |o - A| + longest edge),
                            s >= M, t >= M, s + t <= 1 - M,  t_min < max_distance (1 - M) - 1e-6;
    clearly rejected  when  |b| < 1e-6 (1 - M),  or  a sign(b) <= -M_A |n| L,  or  s or t outside [-1e-5 - M, 1 + 1e-5 + M],
                            or  s + t > 1 + 1e-5 + M,  or  t_min > max_distance (1 + M) + 1e-6;
    borderline        otherwise (a NaN anywhere lands here).
A ray is JUDGED when none of its pairs is borderline; an ambient-occlusion ray also when one pair is clearly accepted
(any-hit needs one); a point when all its rays are.  Rays with a non-finite component or an all-zero direction are
outside this reference (the odd-input tests own them); exactly-zero components are inside.

Within a ray the accepted pairs are ordered by (distance, file-order face).  The contract's tie rule is about LEAF
indices, which this module does not know: the comparator matches a slot against every reference slot within the distance
tolerance, and checks the leaf order among equal distances on the answer itself.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

NONE = 0xFFFFFFFF
M = 1e-4      # margin on |b|, the barycentrics and max_distance
M_A = 1e-6    # margin on the side of the plane the origin lies on, in units of |n| L
B_MIN = 1e-6  # the contract's |b| threshold
ST_EPS = 1e-5  # the contract's tolerance on the barycentrics
KEEP = 17     # reference slots kept per ray: RT_MULTIHIT_MAX_K and one more (the neighbour of slot 15)
THREADS = 8
PAIRS_PER_CHUNK = 1 << 17

# ---- tolerances ---------------------------------------------------------------------------------------------------------
# Worst difference of each float field between the CPU ORACLES (query / multihit / ao / camera oracle, float32, bit-equal
# to the GPU) and this reference, over all the cases of tests/test_geometry_cpu.py (blob, ties, layered; both trees; unit,
# x 37 and x 0.01 directions; max_distance 1e5, 5, 0.3, 0.02; the posed frames) -- printed by that file's tests.  Each
# tolerance is 8 x the measured value: the GPU's differences are the oracle's, the factor only absorbs another ray sample.
#   distance     |delta| / max(1, distance)
#   barycentric  |delta|, per component
#   position     |delta| per component / max(1, distance)
#   normal       |delta|, per component
#   shade        |delta|
# Measured (rounded up to two digits): distance on blob, max_distance 1e5; barycentric, position and normal there too (the
# x 37 and x 0.01 directions); shade on the interior stand-in's frame.
MEASURED = {"distance": 5.9e-7, "barycentric": 1.9e-5, "position": 4.7e-7, "normal": 6.5e-6, "shade": 1.2e-5}
TOL = {f: 8.0 * v for f, v in MEASURED.items()}


class Mesh:
    """Per-triangle float64 terms of a scene's mesh in file order."""

    def __init__(self, scene):
        self.scene = scene
        V = np.asarray(scene.vertices, np.float32)[:, :3].astype(np.float64)
        F = np.asarray(scene.faces, np.uint32).reshape(-1, 3).astype(np.int64)
        self.faces = F
        self.vnormals = np.asarray(scene.vnormals, np.float32)[:, :3].astype(np.float64)
        A, B, C = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
        self.A = A
        self.u, self.v = B - A, C - A
        self.n = np.cross(self.u, self.v)
        self.nlen = np.linalg.norm(self.n, axis=1)
        self.edge = np.maximum(np.maximum(np.linalg.norm(self.u, axis=1), np.linalg.norm(self.v, axis=1)), np.linalg.norm(C - B, axis=1))
        self.uu, self.uv, self.vv = (self.u * self.u).sum(1), (self.u * self.v).sum(1), (self.v * self.v).sum(1)
        self.D = self.uv * self.uv - self.uu * self.vv
        self.nA, self.uA, self.vA, self.AA = (self.n * A).sum(1), (self.u * A).sum(1), (self.v * A).sum(1), (A * A).sum(1)
        self.lo, self.hi = np.minimum(np.minimum(A, B), C), np.maximum(np.maximum(A, B), C)


_MESHES = {}


def mesh_of(scene) -> Mesh:
    if id(scene) not in _MESHES:
        _MESHES[id(scene)] = Mesh(scene)  # (holds the scene: the id stays taken)
    return _MESHES[id(scene)]


def in_scope(o, d) -> np.ndarray:
    """Rays this reference judges at all: finite, with a direction."""
    return np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & (d != 0).any(axis=1)


def _pairs(m: Mesh, o, d, max_distance):
    """o, d: (R, 3) float64.  (accepted, borderline, r, s, t), each (R, T)."""
    with np.errstate(all="ignore"):
        b = d @ m.n.T
        a = m.nA[None, :] - o @ m.n.T  # -n . (o - A)
        r = a / b
        wu = (o @ m.u.T - m.uA[None, :]) + r * (d @ m.u.T)  # (o - A + r d) . u
        wv = (o @ m.v.T - m.vA[None, :]) + r * (d @ m.v.T)
        s = (m.uv * wv - m.vv * wu) / m.D
        t = (m.uv * wu - m.uu * wv) / m.D
        st = s + t
        absb = np.abs(b)
        front = np.where(b < 0, -a, a)  # a sign(b): r >= 0 where this is >= 0
        oA = np.sqrt(np.maximum((o * o).sum(1)[:, None] - 2.0 * (o @ m.A.T) + m.AA[None, :], 0.0))
        thr = M_A * m.nlen[None, :] * (oA + m.edge[None, :])
        t_min = np.full(b.shape, -np.inf)
        for k in range(3):
            near = np.where(np.signbit(d[:, k])[:, None], m.hi[None, :, k], m.lo[None, :, k])
            t_min = np.maximum(t_min, (near - o[:, k, None]) / d[:, k, None])  # (a NaN, 0 / 0, stays: borderline)
        hi = 1.0 + ST_EPS + M
        accepted = (absb >= B_MIN * (1 + M)) & (front >= thr) & (s >= M) & (t >= M) & (st <= 1 - M) & \
            (t_min < max_distance * (1 - M) - 1e-6)
        rejected = (absb < B_MIN * (1 - M)) | (front <= -thr) | (s < -ST_EPS - M) | (s > hi) | (t < -ST_EPS - M) | (t > hi) | \
            (st > hi) | (t_min > max_distance * (1 + M) + 1e-6)
    return accepted, ~(accepted | rejected), r, s, t


def _chunks(n_rays, n_tris):
    step = max(1, PAIRS_PER_CHUNK // max(1, n_tris))
    return [(i, min(n_rays, i + step)) for i in range(0, n_rays, step)]


def _map(fn, spans):
    with ThreadPoolExecutor(THREADS) as pool:  # (numpy releases the interpreter lock inside its loops)
        return list(pool.map(fn, spans))


def multihit(scene, origins, directions, max_distance) -> dict:
    """Everything each ray crosses.  {"count": (N,), "judged": (N,) bool, "distance" / "face": (N, KEEP), "barycentric" /
    "position" / "normal": (N, KEEP, 3)}: the first KEEP accepted pairs by (distance, file-order face); unused slots
    hold +inf / NONE / 0.  Float fields are float64."""
    m = mesh_of(scene)
    o = np.asarray(origins, np.float32)[:, :3].astype(np.float64)
    d = np.asarray(directions, np.float32)[:, :3].astype(np.float64)
    n = o.shape[0]
    out = {"count": np.zeros(n, np.uint32), "judged": np.zeros(n, bool), "distance": np.full((n, KEEP), np.inf),
           "face": np.full((n, KEEP), NONE, np.uint32), "barycentric": np.zeros((n, KEEP, 3)), "position": np.zeros((n, KEEP, 3)),
           "normal": np.zeros((n, KEEP, 3))}
    scope = in_scope(o, d)
    dlen = np.linalg.norm(d, axis=1)

    def work(span):
        i0, i1 = span
        oc, dc = o[i0:i1], d[i0:i1]
        acc, bord, r, s, t = _pairs(m, oc, dc, max_distance)
        out["judged"][i0:i1] = ~bord.any(axis=1) & scope[i0:i1]
        rows, cols = np.nonzero(acc)
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

    _map(work, _chunks(n, len(m.faces)))
    return out


def closest(scene, origins, directions, max_distance, multi=None) -> dict:
    """The nearest accepted pair of each ray, from multihit (pass its answer to reuse it): {"hit", "judged", "distance",
    "face", "barycentric", "position", "normal"}."""
    multi = multi if multi is not None else multihit(scene, origins, directions, max_distance)
    out = {"hit": multi["count"] > 0, "judged": multi["judged"]}
    for f in ("distance", "face", "barycentric", "position", "normal"):
        out[f] = multi[f][:, 0]
    return out


def kernel_float(v) -> float:
    """A float option as the kernels see it: after the reference's "%g" round trip through its -D macros."""
    return float(np.float32(float("%g" % np.float32(v))))


def tangent_frame(normals32):
    """basis_x, basis_z of include/rt_hip_ao.h from the normals AS GIVEN, computed in float64 and rounded to float32 once."""
    n = normals32.astype(np.float64)
    ax, ay, az = np.abs(n[:, 0]), np.abs(n[:, 1]), np.abs(n[:, 2])
    pick_x = (ax <= ay) & (ax <= az)
    pick_y = ~pick_x & (ay <= ax) & (ay <= az)
    pick_z = ~pick_x & ~pick_y & (az <= ax) & (az <= ay)
    h = n.copy()
    h[pick_x, 0] = 1.0
    h[pick_y, 1] = 1.0
    h[pick_z, 2] = 1.0
    with np.errstate(all="ignore"):
        bx = np.cross(h, n)
        bx /= np.linalg.norm(bx, axis=1, keepdims=True)
        bz = np.cross(bx, n)
        bz /= np.linalg.norm(bz, axis=1, keepdims=True)
    return bx.astype(np.float32), bz.astype(np.float32)


def ao_rays(table, points, normals):
    """The UNIFORM rays of include/rt_hip_ao.h: origins (N, 3) = point + normal * (1.0f / 100000.0f), directions (N, K, 3) =
    (basis_x * xs + normal * ys) + basis_z * zs, every product and sum rounded to float32 on its own."""
    p = np.asarray(points, np.float32)[:, :3]
    n = np.asarray(normals, np.float32)[:, :3]
    tab = np.asarray(table, np.float32)[:, :3]
    eps = np.float32(1.0) / np.float32(100000.0)
    o = p + n * eps
    bx, bz = tangent_frame(n)
    xs, ys, zs = tab[None, :, 0, None], tab[None, :, 1, None], tab[None, :, 2, None]
    d = (bx[:, None, :] * xs + n[:, None, :] * ys) + bz[:, None, :] * zs
    assert o.dtype == np.float32 and d.dtype == np.float32
    return o, d


def ao(scene, options, table, points, normals) -> dict:
    """ambient_occlusion (UNIFORM) at caller-supplied points: {"occluded": uint32 (N,), "ao": float32 (N,) = 1 - occluded /
    len(table), "judged": bool (N,), "rays": len(table)}."""
    assert options.ao_method == 0
    m = mesh_of(scene)
    o32, d32 = ao_rays(table, points, normals)
    npts, k = d32.shape[0], d32.shape[1]
    o = np.repeat(o32.astype(np.float64), k, axis=0)
    d = d32.reshape(-1, 3).astype(np.float64)
    max_distance = kernel_float(options.ao_max_distance)
    hit, judged = np.zeros(npts * k, bool), np.zeros(npts * k, bool)
    scope = in_scope(o, d)

    def work(span):
        i0, i1 = span
        acc, bord, _, _, _ = _pairs(m, o[i0:i1], d[i0:i1], max_distance)
        hit[i0:i1] = acc.any(axis=1)
        judged[i0:i1] = (hit[i0:i1] | ~bord.any(axis=1)) & scope[i0:i1]

    _map(work, _chunks(npts * k, len(m.faces)))
    occluded = hit.reshape(npts, k).sum(axis=1).astype(np.uint32)
    return {"occluded": occluded, "ao": np.float32(1.0) - occluded.astype(np.float32) / np.float32(k),
            "judged": judged.reshape(npts, k).all(axis=1), "rays": k}


def camera_rays(options, camera):
    """(origins, directions), (W H, 3) float32 each, by the formula of include/rt_hip_camera.h in float32 numpy, one rounding
    per operation.  `camera`: (4, 3) eye, right, up, forward, or an object with as_array()."""
    pose = np.asarray(camera.as_array() if hasattr(camera, "as_array") else camera, np.float32).reshape(4, 3)
    n = int(np.sqrt(float(options.n_super_samples)))
    W, H = options.width * n, options.height * n
    f32 = np.float32
    a = f32(kernel_float(options.focal_length)) * f32(max(W, H))
    x, y = np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32)
    cx = (x + f32(0.5)) / a - f32(W) / (f32(2.0) * a)
    cy = -((y + f32(0.5)) / a - f32(H) / (f32(2.0) * a))
    cx, cy = np.broadcast_to(cx[None, :], (H, W)).reshape(-1), np.broadcast_to(cy[:, None], (H, W)).reshape(-1)
    eye, R, U, F = pose
    w = (R[None, :] * cx[:, None] + U[None, :] * cy[:, None]) + F[None, :]
    length = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
    d = w / length[:, None]
    assert d.dtype == np.float32
    return np.broadcast_to(eye[None, :], d.shape).copy(), d


def posed_frame(scene, options, camera) -> dict:
    """The frame of a posed camera without ambient occlusion: {"hit": (H, W) bool, "shade": (H, W) float64 = clamp(-n . d)
    (1 where shading is off, 0 without a hit), "judged": (H, W) bool, "origins" / "directions": the rays, "closest": the
    rays' closest hits, "shading": whether shading is on}."""
    o, d = camera_rays(options, camera)
    n = int(np.sqrt(float(options.n_super_samples)))
    shape = (options.height * n, options.width * n)
    near = closest(scene, o, d, 100000.0)
    shade = np.ones(len(o))
    if options.enable_shading:
        shade = np.clip(-(near["normal"] * d.astype(np.float64)).sum(axis=1), 0.0, 1.0)
    shade = np.where(near["hit"], shade, 0.0)
    return {"hit": near["hit"].reshape(shape), "shade": shade.reshape(shape), "judged": near["judged"].reshape(shape),
            "origins": o, "directions": d, "closest": near, "shading": bool(options.enable_shading)}


def without_shading(frame: dict) -> dict:
    """posed_frame()'s answer for the same options with shading off: 1 at every hit."""
    out = dict(frame)
    out["shade"], out["shading"] = frame["hit"].astype(np.float64), False
    return out


# ---- the comparator -----------------------------------------------------------------------------------------------------
class Report(dict):
    """What a comparison found.  Keys: "rays", "judged_share", "hit_share", mismatch counts ("count", "hit", "leaf", "order",
    "fill", ...) under "mismatches", and the worst difference per float field under "worst"."""

    def failures(self, tol=None, max_unjudged=0.01) -> list:
        tol = TOL if tol is None else tol
        bad = [f"{k}: {v} mismatches" for k, v in self["mismatches"].items() if v]
        bad += [f"{f}: worst difference {v:.3g} > {tol[f]:.3g}" for f, v in self["worst"].items() if not v <= tol[f]]
        if not self["judged_share"] >= 1.0 - max_unjudged:
            bad.append(f"only {self['judged_share']:.4%} judged")
        return bad

    def __str__(self):
        worst = ", ".join(f"{f} {v:.3g}" for f, v in self["worst"].items())
        mism = ", ".join(f"{k} {v}" for k, v in self["mismatches"].items())
        return f"{self['rays']} rays, judged {self['judged_share']:.4%}, with a hit {self['hit_share']:.2%}; mismatches: {mism}; worst: {worst}"


def _worst(a):
    return float(a.max()) if a.size else 0.0


def compare_multihit(scene, ref: dict, got: dict, k: int, tol=None) -> Report:
    """A multi-hit answer in the library's form ({"count", "distance", "leaf", "barycentric", "position", "normal"}, k slots,
    leaves in the tree's order) against multihit()'s, on the judged rays."""
    tol = TOL if tol is None else tol
    j = ref["judged"]
    n_ref = np.minimum(ref["count"], k)
    mism = {"count": int((got["count"] != ref["count"])[j].sum())}
    ok = j & (got["count"] == ref["count"])  # the slots are compared where the counts agree
    used = (np.arange(k)[None, :] < n_ref[:, None]) & ok[:, None]
    free = (np.arange(k)[None, :] >= n_ref[:, None]) & ok[:, None]
    leaf = np.asarray(got["leaf"], np.uint32).reshape(-1, k)
    gd = np.asarray(got["distance"], np.float64).reshape(-1, k)
    # unused slots: +inf / NONE / 0
    fill_bad = free & ~((leaf == NONE) & np.isposinf(gd))
    for f in ("barycentric", "position", "normal"):
        fill_bad |= free & (np.asarray(got[f]).reshape(-1, k, 3) != 0).any(axis=2)
    mism["fill"] = int(fill_bad.sum())
    mism["unused_slot"] = int((used & (leaf == NONE)).sum())
    face = scene.face_of_leaf(leaf.reshape(-1)).reshape(-1, k)
    # the slot's face must be a reference face within the distance tolerance of the reference's slot: that slot itself
    # unless the reference's neighbours tie with it
    rd = ref["distance"]
    with np.errstate(invalid="ignore"):
        near = np.abs(rd[:, None, :] - rd[:, :k, None]) <= tol["distance"] * np.maximum(1.0, rd[:, :k, None])
    match = near & (ref["face"][:, None, :] == face[:, :, None]) & (face[:, :, None] != NONE)
    found = match.any(axis=2)
    mism["leaf"] = int((used & ~found).sum())
    at = np.where(found, match.argmax(axis=2), np.arange(k)[None, :])  # the reference slot a slot stands for
    rows = np.arange(len(rd))[:, None]
    cmp = used & found
    rdist = rd[rows, at]
    scale = np.maximum(1.0, np.where(cmp, rdist, 1.0))
    worst = {}
    with np.errstate(invalid="ignore"):
        worst["distance"] = _worst((np.abs(gd - rdist) / scale)[cmp])
        for f in ("barycentric", "position", "normal"):
            delta = np.abs(np.asarray(got[f], np.float64).reshape(-1, k, 3) - ref[f][rows, at]).max(axis=2)
            worst[f] = _worst((delta / scale if f == "position" else delta)[cmp])
    # the contract's order on the answer itself: distance ascending, leaf ascending among equal distances
    if k > 1:
        both = used[:, :-1] & used[:, 1:]
        asc = (gd[:, :-1] < gd[:, 1:]) | ((gd[:, :-1] == gd[:, 1:]) & (leaf[:, :-1].astype(np.int64) < leaf[:, 1:].astype(np.int64)))
        mism["order"] = int((both & ~asc).sum())
    return Report(rays=len(j), judged_share=float(j.mean()), hit_share=float((ref["count"] > 0).mean()), mismatches=mism, worst=worst)


def compare_closest(scene, ref_multi: dict, got: dict, tol=None) -> Report:
    """A closest-hit answer in the library's form ({"hit", "distance", "leaf", "barycentric", "position", "normal"}) against
    multihit()'s: slot 0, `hit` = count > 0, and +inf / NONE / 0 without a hit."""
    hit = np.asarray(got["hit"]).astype(bool)
    as_multi = {"count": np.where(hit, ref_multi["count"], 0).astype(np.uint32)}  # (the count itself is count_hits' business)
    for f in ("distance", "leaf"):
        as_multi[f] = np.asarray(got[f]).reshape(-1, 1)
    for f in ("barycentric", "position", "normal"):
        as_multi[f] = np.asarray(got[f]).reshape(-1, 1, 3)
    rep = compare_multihit(scene, ref_multi, as_multi, 1, tol)
    rep["mismatches"]["hit"] = int((hit != (ref_multi["count"] > 0))[ref_multi["judged"]].sum())
    del rep["mismatches"]["count"]
    return rep


def compare_flags(ref_multi: dict, got_hit, what="hit") -> Report:
    """An occlusion answer (or any per-ray boolean that must equal count > 0) against multihit()'s."""
    j = ref_multi["judged"]
    bad = int((np.asarray(got_hit).astype(bool) != (ref_multi["count"] > 0))[j].sum())
    return Report(rays=len(j), judged_share=float(j.mean()), hit_share=float((ref_multi["count"] > 0).mean()),
                  mismatches={what: bad}, worst={})


def compare_counts(ref_multi: dict, got_count) -> Report:
    j = ref_multi["judged"]
    bad = int((np.asarray(got_count) != ref_multi["count"])[j].sum())
    return Report(rays=len(j), judged_share=float(j.mean()), hit_share=float((ref_multi["count"] > 0).mean()),
                  mismatches={"count": bad}, worst={})


def compare_ao(ref: dict, got: dict) -> Report:
    """{"ao", "occluded"} of the library's form against ao()'s: the counts exactly on judged points, and ao = 1 - occluded /
    divisor in float32 on every point."""
    j = ref["judged"]
    occ = np.asarray(got["occluded"])
    mism = {"occluded": int((occ != ref["occluded"])[j].sum())}
    own = np.float32(1.0) - occ.astype(np.float32) / np.float32(ref["rays"])
    mism["ao"] = int((np.asarray(got["ao"], np.float32).view(np.uint32) != own.view(np.uint32)).sum())
    return Report(rays=len(j), judged_share=float(j.mean()), hit_share=float((ref["occluded"] > 0).mean()), mismatches=mism, worst={})


def compare_frame(ref: dict, image) -> Report:
    """A float frame rendered WITHOUT ambient occlusion against posed_frame()'s, on judged pixels.  Shading off: the frame
    is the hit mask (1 / 0), compared exactly.  Shading on: the shade within tolerance (a back-facing hit is shaded 0, so
    the mask is not read off such a frame)."""
    img = np.asarray(image, np.float64)
    j = ref["judged"]
    mism, worst = {}, {}
    if ref["shading"]:
        worst["shade"] = _worst(np.abs(img - ref["shade"])[j])
    else:
        mism["hit"] = int((((img != 0) != ref["hit"]) | ((img != 0) & (img != 1)))[j].sum())
    return Report(rays=j.size, judged_share=float(j.mean()), hit_share=float(ref["hit"].mean()), mismatches=mism, worst=worst)
