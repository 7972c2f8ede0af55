"""Inputs the CPU and GPU tests of the segment queries share (include/rt_hip_segment.h).  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import multihit_oracle as mo
import query_oracle as qo

DEFAULT = (1e-4, 1 - 1e-4)
INTERVALS = (DEFAULT, (0.25, 0.75), (-1.0, np.inf))
SURFACE_INTERVAL = (1e-3, 1 - 1e-3)
# t_lo, t_hi in {NaN, -1, 0, +inf}, every combination (it holds t_lo > t_hi and t_lo == t_hi), and two more reversed ones
ODD_VALUES = (np.nan, -1.0, 0.0, np.inf)
ODD_INTERVALS = tuple((lo, hi) for lo in ODD_VALUES for hi in ODD_VALUES) + ((0.75, 0.25), (1.0, 1e-4), (-np.inf, np.inf), (0.5, -np.inf))


def blocks_nothing(interval) -> bool:
    """The intervals for which the header says "nothing blocks" whatever the segment: a NaN, t_hi <= 0, t_lo = +inf,
    t_lo >= t_hi."""
    lo, hi = float(interval[0]), float(interval[1])
    return bool(np.isnan(lo) or np.isnan(hi) or hi <= 0.0 or lo == np.inf or lo >= hi)


def endpoints(arrays, n, seed, factor=1.25):
    """n points, float32 (n, 3), uniform in the root box scaled by `factor` about its centre."""
    rng = np.random.default_rng(seed)
    lo, hi = mo.box_of(arrays)
    centre, half = (lo + hi) / 2, (hi - lo) / 2 * factor
    return (centre - half + rng.random((n, 3)) * 2 * half).astype(np.float32)


def box_segments(arrays, n, seed):
    """(a, b): n segments with both endpoints in the root box x 1.25."""
    return endpoints(arrays, n, seed), endpoints(arrays, n, seed + 1000)


def surface_segments(arrays, n, seed):
    """(a, b): n segments between points ON the surface -- closest hits of random rays, by the CPU oracle -- paired at random:
    the triangles the endpoints lie on are at r ~ 0 and r ~ 1.  That needs a segment that LEAVES the planes of its own two
    triangles: for one that lies in such a plane (both ends on the blob's flat base) r is 0 / 0, and no arithmetic decides it.
    Pairs whose direction makes less than 0.01 (as a sine) with either plane are not taken -- five in six on the blob, whose
    base catches most rays."""
    o, d = mo.random_rays(arrays, 80 * n, seed=seed)
    res = qo.closest(arrays, o, d, 100000.0)
    hit = np.flatnonzero(res["hit"].astype(bool) & np.isfinite(res["distance"]))
    hit = hit[:len(hit) // 2 * 2]
    p = np.ascontiguousarray(res["position"][hit]).astype(np.float64)
    corners = arrays.vertices[:, :3][arrays.faces.reshape(-1, 3)[res["leaf"][hit]]].astype(np.float64)
    normal = np.cross(corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0])
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    half = len(hit) // 2
    along = p[half:] - p[:half]
    along /= np.linalg.norm(along, axis=1, keepdims=True)
    leaves = (np.abs((along * normal[:half]).sum(axis=1)) > 0.01) & (np.abs((along * normal[half:]).sum(axis=1)) > 0.01)
    keep = np.flatnonzero(leaves)[:n]
    assert len(keep) == n, len(keep)
    p32 = p.astype(np.float32)
    return np.ascontiguousarray(p32[:half][keep]), np.ascontiguousarray(p32[half:][keep])


def odd_segments(arrays, seed=9):
    """(a, b, nothing): segments with odd endpoints -- of no length, with a NaN or an infinite coordinate at either end,
    huge, denormal -- among ordinary ones; nothing[i]: the header says "nothing blocks" for segment i whatever the interval."""
    a, b = box_segments(arrays, 520, seed)
    k = np.arange(len(a))
    a[k % 7 == 1, 0] = np.nan
    b[k % 11 == 2, 1] = np.nan
    a[k % 13 == 3, 2] = np.inf
    b[k % 17 == 4, 0] = -np.inf
    a[k % 19 == 6] = np.inf
    b[k % 19 == 6] = np.inf
    b[k % 23 == 7] *= np.float32(1e30)   # a far end far away: r tiny
    a[k % 29 == 8] = np.float32(3e38)    # (b - a overflows or not, component by component)
    b[k % 31 == 9, 1] = np.float32(1e-41)
    a[k % 37 == 10] = np.float32(-0.0)
    zero = k % 5 == 0                    # (last: of no length whatever the ends hold)
    b[zero] = a[zero]
    nothing = zero | ~np.isfinite(a).all(axis=1) | ~np.isfinite(b).all(axis=1)
    return a, b, nothing


def mask_inputs(arrays, n_points, n_targets, seed):
    return endpoints(arrays, n_points, seed), endpoints(arrays, n_targets, seed + 500)


def pairs_of(points, targets):
    """The P x T segments of a mask call, written out (tests only): row-major, (i, j) at i T + j."""
    p, t = np.asarray(points), np.asarray(targets)
    return np.repeat(p, len(t), axis=0), np.tile(t, (len(p), 1))


def popcount(words) -> np.ndarray:
    w = np.ascontiguousarray(words, np.uint32)
    if w.shape[1] == 0:
        return np.zeros(w.shape[0], np.uint32)
    return np.unpackbits(w.view(np.uint8), axis=-1).reshape(w.shape[0], -1).sum(axis=1).astype(np.uint32)
