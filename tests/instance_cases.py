"""Inputs the CPU and GPU tests of the instanced ray queries share (include/rt_hip_instances.h): families of transforms sized
relative to the mesh's root box, odd transforms for the error path, and rays.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import multihit_oracle as mo

MAX_DISTANCES = (1e5, 5.0, 0.3)
FAMILIES = ("identity", "translations", "rotations", "scales", "shear", "mirror", "tie_pair", "overlap_pair", "grid")
COUNTS = (1, 2, 3, 64, 65, 1000)
# the sets that push the terms of the instance box margin (csrc/instances.cc, instance_margin): the inverse's entries (`ill`),
# the reach of the whole set against a copy's own size (`tiny_huge`, `wide`), the translations (`far`), and both (`far_ill`)
HARD_FAMILIES = ("ill", "tiny_huge", "far", "wide", "far_ill")
ILL_SINGULAR_VALUES = ((1.0, 1.0, 1e-2), (1e2, 1.0, 1e-1), (30.0, 1.0, 3e-3), (1.0, 1e-4, 1.0), (-1.0, 1.0, 1e-2))
ORIGIN_CLASSES = ("inside", "shell", "grazing")


def root_box(arrays):
    lo, hi = mo.box_of(arrays)
    return lo.astype(np.float32), hi.astype(np.float32)


def _rotation(rng) -> np.ndarray:
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))[None, :]
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _about(A, centre, shift) -> np.ndarray:
    """[A | t] that applies A about `centre` and then moves by `shift`."""
    W = np.zeros((3, 4))
    W[:, :3] = A
    W[:, 3] = centre - A @ centre + shift
    return W


def family(name: str, arrays, seed: int = 0) -> np.ndarray:
    """float32 (n, 3, 4): the transforms of one family for the mesh of `arrays`."""
    lo, hi = mo.box_of(arrays)
    centre, ext = (lo + hi) / 2, hi - lo
    diag = float(np.linalg.norm(ext))
    rng = np.random.default_rng(1000 + 17 * (FAMILIES + HARD_FAMILIES).index(name) + seed)
    eye, none = np.eye(3), np.zeros(3)

    def direction():
        v = rng.normal(size=3)
        return v / np.linalg.norm(v)

    if name == "identity":
        W = [_about(eye, centre, none)]
    elif name == "translations":  # up to 4 box diagonals
        W = [_about(eye, centre, direction() * diag * u) for u in (0.0, 0.5, 1.0, 2.0, 3.0, 4.0)]
    elif name == "rotations":
        W = [_about(_rotation(rng), centre, direction() * diag * 0.6 * k) for k in range(6)]
    elif name == "scales":  # uniform, in [1/4, 4]
        W = [_about(eye * s, centre, direction() * diag * 0.8 * k) for k, s in enumerate((0.25, 0.5, 1.0, 2.0, 4.0))]
    elif name == "shear":  # U diag(s) V^T with s_max / s_min <= 8: a non-uniform scale with shear
        W = []
        for k, s in enumerate(((1.0, 2.0, 8.0), (0.5, 1.0, 3.0), (2.0, 0.25, 1.0), (1.0, 1.0, 6.0))):
            W.append(_about(_rotation(rng) @ np.diag(s) @ _rotation(rng).T, centre, direction() * diag * 1.2 * k))
    elif name == "mirror":  # a negative determinant
        W = [_about(_rotation(rng) @ np.diag((-1.0, 1.0, 1.0)), centre, none), _about(np.diag((1.0, -1.0, 1.0)), centre, direction() * diag * 0.7)]
    elif name == "tie_pair":  # the same transform twice: every hit ties
        one = _about(_rotation(rng), centre, direction() * diag * 0.25)
        W = [one, one.copy()]
    elif name == "overlap_pair":  # two copies half a box apart
        W = [_about(eye, centre, none), _about(eye, centre, np.array([ext[0] / 2, 0.0, 0.0]))]
    elif name == "grid":  # 5 x 5 x 5, translated and rotated
        W = []
        for i in range(5):
            for j in range(5):
                for k in range(5):
                    W.append(_about(_rotation(rng), centre, (np.array([i, j, k]) - 2.0) * ext.max() * 1.6))
    elif name in ("ill", "far_ill"):  # U diag(s) V^T with s_max / s_min of 1e2, 1e3 and 1e4; the last has a negative determinant
        W = []
        for k, s in enumerate(ILL_SINGULAR_VALUES):
            away = direction() * diag * (1e3 if name == "far_ill" else 0.0)  # (far_ill: |O_j3| large, the other half of q_j)
            W.append(_about(_rotation(rng) @ np.diag(s) @ _rotation(rng).T, centre, direction() * diag * 1.5 * k * max(1.0, max(np.abs(s)) / 4) + away))
    elif name == "tiny_huge":  # uniform scales 1e-3 .. 1e3 in one set: the large copies make G, the small ones sit in its margin
        W = [_about(eye * s, centre, np.eye(3)[k % 3] * diag * u) for k, (s, u) in enumerate(((1e-3, 0.0), (1e-2, 0.05), (1e2, 150.0), (1e3, 1500.0)))]
    elif name == "far":  # rigid copies 1e2, 1e3 and 1e4 box diagonals from the origin: a translation alone, and with a rotation
        W = []
        for u in (1e2, 1e3, 1e4):
            W.append(_about(eye, centre, direction() * diag * u))
            W.append(_about(_rotation(rng), centre, direction() * diag * u))
    elif name == "wide":  # one copy at the mesh's own place, six at +-1e4 diagonals along the axes: rotated at +, as they are at -
        W = [_about(eye, centre, none)]
        for a in range(3):
            W += [_about(_rotation(rng), centre, np.eye(3)[a] * diag * 1e4), _about(eye, centre, -np.eye(3)[a] * diag * 1e4)]
    else:
        raise KeyError(name)
    return np.ascontiguousarray(np.stack(W), np.float32)


def many(arrays, n: int, seed: int = 0) -> np.ndarray:
    """n translated, rotated and scaled copies scattered over a cube that grows with n."""
    lo, hi = mo.box_of(arrays)
    centre, ext = (lo + hi) / 2, hi - lo
    rng = np.random.default_rng(5000 + n + seed)
    side = max(1.0, float(n) ** (1.0 / 3.0)) * ext.max() * 1.5
    W = [_about(_rotation(rng) * rng.uniform(0.5, 1.5), centre, (rng.random(3) - 0.5) * side) for _ in range(n)]
    return np.ascontiguousarray(np.stack(W), np.float32)


def odd_transforms(arrays) -> dict:
    """Transforms rt_set_instances must refuse: each a (1, 3, 4) float32."""
    base = family("identity", arrays)[0].astype(np.float64)
    out = {}
    w = base.copy(); w[1, 2] = np.nan; out["nan"] = w
    w = base.copy(); w[0, 3] = np.inf; out["inf"] = w
    w = base.copy(); w[:, :3] = 0.0; out["singular"] = w
    w = base.copy(); w[2, :3] = w[0, :3] + w[1, :3]; out["rank2"] = w
    w = base.copy(); w[:, :3] = np.eye(3) * 1e-39; out["inverse_overflows"] = w  # (the inverse's entries exceed binary32)
    return {k: np.ascontiguousarray(v[None], np.float32) for k, v in out.items()}


def top_box(nodes):
    return np.asarray(nodes["lo"][0], np.float64), np.asarray(nodes["hi"][0], np.float64)


def rays(nodes, n: int, seed: int):
    """(origins, directions) float32 (n, 3): origins uniform in the top-level root box x 1.25; random directions -- half of
    them isotropic, half towards a point drawn in a random instance's box, so that sparse sets are hit too -- of length 1,
    37 and 0.01 in turn."""
    rng = np.random.default_rng(seed)
    lo, hi = top_box(nodes)
    centre, half = (lo + hi) / 2, (hi - lo) / 2 * 1.25
    o = centre - half + rng.random((n, 3)) * 2 * half
    d = rng.normal(size=(n, 3))
    leaves = nodes[nodes["leaf"] != 0xFFFFFFFF]
    pick = leaves[rng.integers(0, len(leaves), n)]
    target = pick["lo"] + rng.random((n, 3)) * (pick["hi"].astype(np.float64) - pick["lo"])
    aimed = np.arange(n) % 2 == 1
    d[aimed] = (target - o)[aimed]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d *= np.array([1.0, 37.0, 0.01])[np.arange(n) % 3][:, None]
    return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)


def set_reach(arrays, W) -> float:
    """The reach of the whole set as csrc/instances.cc defines it (instance_reach, its maximum): G = 4 x this."""
    lo, hi = mo.box_of(arrays)
    absW = np.abs(np.asarray(W, np.float64))
    return float((absW[:, :, :3] @ np.maximum(np.abs(lo), np.abs(hi)) + absW[:, :, 3]).max())


def restated_margins(arrays, plan, W) -> np.ndarray:
    """(n, 3) float64: instance_margin restated, m_k = 2^-20 (G + sum_j |A_kj| q_j), q_j = (|O_j0| + |O_j1| + |O_j2|) G + |O_j3|."""
    G = 4.0 * set_reach(arrays, W)
    absW, absO = np.abs(np.asarray(W, np.float64)), np.abs(np.asarray(plan["object_from_world"], np.float64))
    q = absO[:, :, :3].sum(axis=2) * G + absO[:, :, 3]
    return 2.0 ** -20 * (G + np.einsum("nkj,nj->nk", absW[:, :, :3], q))


def leaf_boxes(nodes, n: int):
    """(lo, hi) float64 (n, 3): the top-level leaf box of every instance, by instance index."""
    leaves = nodes[nodes["leaf"] != 0xFFFFFFFF]
    lo, hi = np.zeros((n, 3)), np.zeros((n, 3))
    lo[leaves["leaf"]], hi[leaves["leaf"]] = leaves["lo"], leaves["hi"]
    return lo, hi


def margin_plans(rt, arrays, W):
    """(real, open): two plans of the same set from rt.instance_plan.  `real` has the scene's root box: the boxes the library
    makes.  `open` has a root box with one coordinate +inf, so that every leaf box is (-inf, +inf) and every copy is entered.
    rt.instance_plan raises where rt_instance_plan refuses a transform."""
    lo, hi = root_box(arrays)
    endless = hi.copy()
    endless[0] = np.inf
    real, opened = rt.instance_plan(lo, hi, W), rt.instance_plan(lo, endless, W)
    assert real["object_from_world"].tobytes() == opened["object_from_world"].tobytes()
    assert np.isneginf(opened["nodes"]["lo"]).all() and np.isposinf(opened["nodes"]["hi"]).all()
    assert np.isfinite(real["nodes"]["lo"]).all() and np.isfinite(real["nodes"]["hi"]).all()
    for plan in (real, opened):
        plan["world_from_object"] = W
    return real, opened


def clearly_inside(answer, least) -> np.ndarray:
    """The rays of a closest answer that hit at a finite distance with every returned barycentric >= least."""
    return (answer["hit"] != 0) & np.isfinite(answer["distance"]) & (answer["barycentric"] >= np.float32(least)).all(axis=1)


def origin_class(n: int) -> np.ndarray:
    """The index into ORIGIN_CLASSES of each of margin_rays' n rays."""
    return np.arange(n) % 3


def margin_rays(arrays, plan, W, n: int, seed: int, beta=(2e-4, 0.3)):
    """(origins, directions) float32 (n, 3) that attack the top-level leaf boxes of `plan` (the library's own plan of W, finite
    boxes).  Each ray belongs to a target in a random instance: a point of a triangle that owns a vertex attaining the
    object root box's lo or hi on an axis (all six faces in turn), at barycentrics (1 - 2 b, b, b) from that vertex, b
    log-uniform in `beta`, mapped to world space in float64 -- the hits nearest the box's boundary.  Origins, by index % 3
    (ORIGIN_CLASSES): uniform in the top-level root box; on the shell 0.5 G <= |o|_inf <= G, G = 4 x set_reach; just outside
    a face of the target instance's own leaf box, within four margins of it (half of them the face nearest the target).
    Two thirds of the rays are aimed at the target.  Every third triple of rays grazes instead: its direction lies within
    1e-3 rad (log-uniform from 1e-6) of the face of the instance's world box -- the float64 image of the root box -- that
    is nearest the target, its origin moved along that face's axis to make it so; half of these pass through the target, the
    other half through the target's projection on a plane 1e-6 to 4 margins (log-uniform) OUTSIDE that face: a ray that
    misses the exact box, in which the lane can still find a hit through the rounding of its own object ray -- what the
    margin is for -- and, beyond one margin, a ray that misses the library's box too, in which it must find none.  Directions have length 1, 37 and 0.01 in turn, and every tenth direction
    component is exactly 0.  Every origin is finite with |o|_inf <= G: the contract's scope."""
    rng = np.random.default_rng(seed)
    W64 = np.asarray(W, np.float64)
    count = len(W64)
    G = 4.0 * set_reach(arrays, W)
    margins = restated_margins(arrays, plan, W)
    box_lo, box_hi = leaf_boxes(plan["nodes"], count)
    assert np.isfinite(box_lo).all() and np.isfinite(box_hi).all()
    root_lo, root_hi = mo.box_of(arrays)
    corners = np.array([[(root_hi if k >> a & 1 else root_lo)[a] for a in range(3)] for k in range(8)])
    image = np.einsum("nij,kj->nki", W64[:, :, :3], corners) + W64[:, None, :, 3]
    i = np.arange(n)
    cls, grazing = origin_class(n), (i // 9) % 3 == 0
    inst = rng.integers(0, count, n)
    # targets
    faces, verts = arrays.faces.reshape(-1, 3), arrays.vertices[:, :3].astype(np.float64)
    used = np.unique(faces)
    face = rng.permutation(n) % 6
    b = np.exp(rng.uniform(np.log(beta[0]), np.log(beta[1]), n))
    target = np.zeros((n, 3))
    for f in range(6):
        column = verts[used, f % 3]
        extreme = used[column == (column.min() if f < 3 else column.max())]
        rows, cols = np.nonzero(np.isin(faces, extreme))
        at = np.flatnonzero(face == f)
        pick = rng.integers(0, len(rows), len(at))
        tri, col = faces[rows[pick]], cols[pick]
        k = np.arange(len(at))
        p0, p1, p2 = verts[tri[k, col]], verts[tri[k, (col + 1) % 3]], verts[tri[k, (col + 2) % 3]]
        point = p0 + b[at, None] * (p1 - p0) + b[at, None] * (p2 - p0)
        target[at] = np.einsum("nij,nj->ni", W64[inst[at], :, :3], point) + W64[inst[at], :, 3]
    # origins
    top_lo, top_hi = top_box(plan["nodes"])
    o = top_lo + rng.random((n, 3)) * (top_hi - top_lo)
    v = rng.random((n, 3)) * 2 - 1
    shell = v / np.abs(v).max(axis=1, keepdims=True) * G * rng.uniform(0.501, 0.999, (n, 1))
    # ... every other one at the far end of the set as its target sees it: beyond the world's origin along the target's largest
    # coordinate, where the rounding of the object origin's coordinate on that axis is coarsest against the copy's own box
    far_end = np.flatnonzero((i // 3) % 2 == 1)
    was, to = np.abs(shell[far_end]).argmax(axis=1), np.abs(target[far_end]).argmax(axis=1)
    shell[far_end, was], shell[far_end, to] = shell[far_end, to], shell[far_end, was]
    shell[far_end, to] = -np.copysign(shell[far_end, to], target[far_end, to])
    o[cls == 1] = shell[cls == 1]
    lo, hi, m = box_lo[inst], box_hi[inst], margins[inst]
    gap = np.concatenate([target - lo, hi - target], axis=1)  # (to the six faces of the leaf box: lo x, y, z, hi x, y, z)
    side = np.where((i // 3) % 2 == 0, rng.integers(0, 6, n), gap.argmin(axis=1))
    outside = lo - 0.1 * (hi - lo) + rng.random((n, 3)) * 1.2 * (hi - lo)
    c = np.exp(rng.uniform(np.log(1e-3), np.log(4.0), n))
    outside[i, side % 3] = np.where(side < 3, lo[i, side % 3] - c * m[i, side % 3], hi[i, side % 3] + c * m[i, side % 3])
    o[cls == 2] = outside[cls == 2]
    # the grazing rays: the aim, then the origin's coordinate along the face's axis
    image_lo, image_hi = image.min(axis=1)[inst], image.max(axis=1)[inst]
    nearest = np.concatenate([target - image_lo, image_hi - target], axis=1).argmin(axis=1)
    along = nearest % 3
    plane = np.where(nearest < 3, image_lo[i, along], image_hi[i, along])
    beyond = np.where(nearest < 3, -1.0, 1.0) * np.exp(rng.uniform(np.log(1e-6), np.log(4.0), n)) * m[i, along]
    aim = target.copy()
    aim[i, along] = np.where((i // 27) % 2 == 0, plane + beyond, target[i, along])
    aim = np.where(grazing[:, None], aim, target)
    heavy = np.abs(o).argmax(axis=1)
    clash = np.flatnonzero(grazing & (cls == 1) & (along == heavy))  # (the shell's largest coordinate stays: swap it away)
    other = (heavy[clash] + 1) % 3
    o[clash, heavy[clash]], o[clash, other] = o[clash, other], o[clash, heavy[clash]]
    rest = o - aim
    rest[i, along] = 0.0
    angle = np.exp(rng.uniform(np.log(1e-6), np.log(1e-3), n)) * rng.choice([-1.0, 1.0], n)
    moved = o.copy()
    moved[i, along] = aim[i, along] + angle * np.linalg.norm(rest, axis=1)
    moved = np.where((cls == 0)[:, None], np.clip(moved, top_lo, top_hi), moved)
    o[grazing] = moved[grazing]
    o = np.ascontiguousarray(o, np.float32)
    assert np.isfinite(o).all() and np.abs(o.astype(np.float64)).max() <= G
    assert (np.abs(o[cls == 1].astype(np.float64)).max(axis=1) >= 0.5 * G).all()
    d = aim - o.astype(np.float64)
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-300)
    d *= np.array([1.0, 37.0, 0.01])[(i // 3) % 3][:, None]
    d = np.ascontiguousarray(d, np.float32)
    d.reshape(-1)[9::10] = 0.0
    return o, d


def odd_rays(nodes, seed: int = 9):
    """Rays with zero, NaN and infinite components and zero-length directions among ordinary ones."""
    o, d = rays(nodes, 520, seed)
    k = np.arange(len(o))
    o[k % 7 == 1, 0] = np.nan
    d[k % 11 == 2, 1] = np.nan
    o[k % 13 == 3, 2] = np.inf
    d[k % 17 == 4, 0] = -np.inf
    d[k % 19 == 6] = np.inf
    d[k % 23 == 7] *= np.float32(1e30)
    o[k % 29 == 8] = np.float32(3e38)
    d[k % 31 == 9, 1] = np.float32(1e-41)
    d[k % 37 == 10, 2] = np.float32(-0.0)
    d[k % 41 == 11, 0] = np.float32(0.0)
    o[k % 43 == 12] = np.float32(0.0)
    d[k % 5 == 0] = np.float32(0.0)  # (last: no direction whatever the rest holds)
    return o, d


def without_negative_zero(o, d):
    """The rays of the identity relation: finite components, no -0."""
    ok = np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & ~(np.signbit(o) & (o == 0)).any(axis=1) & ~(np.signbit(d) & (d == 0)).any(axis=1)
    return np.ascontiguousarray(o[ok]), np.ascontiguousarray(d[ok])
