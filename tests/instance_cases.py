"""Inputs the CPU and GPU tests of the instanced ray queries share (include/rt_hip_instances.h): families of transforms sized
relative to the mesh's root box, odd transforms for the error path, and rays.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import multihit_oracle as mo

MAX_DISTANCES = (1e5, 5.0, 0.3)
FAMILIES = ("identity", "translations", "rotations", "scales", "shear", "mirror", "tie_pair", "overlap_pair", "grid")
COUNTS = (1, 2, 3, 64, 65, 1000)


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
    rng = np.random.default_rng(1000 + 17 * FAMILIES.index(name) + seed)
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
