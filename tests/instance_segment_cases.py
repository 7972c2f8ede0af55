"""Inputs the CPU and GPU tests of the instanced segment queries share (include/rt_hip_instance_segments.h), built on
instance_cases and segment_cases.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import instance_cases
import instance_oracle
import segment_cases

INTERVALS = segment_cases.INTERVALS
SURFACE_INTERVAL = segment_cases.SURFACE_INTERVAL
ODD_INTERVALS = segment_cases.ODD_INTERVALS
blocks_nothing = segment_cases.blocks_nothing


def plan_for(rt, arrays, transforms) -> dict:
    """The plan the library would make for `transforms` over the mesh of `arrays` (rt_instance_plan: host only)."""
    lo, hi = instance_cases.root_box(arrays)
    plan = rt.instance_plan(lo, hi, transforms)
    plan["world_from_object"] = transforms
    return plan


def box_points(nodes, n: int, seed: int, factor: float = 1.25) -> np.ndarray:
    """n points, float32 (n, 3), uniform in the top-level root box scaled by `factor` about its centre."""
    rng = np.random.default_rng(seed)
    lo, hi = instance_cases.top_box(nodes)
    centre, half = (lo + hi) / 2, (hi - lo) / 2 * factor
    return (centre - half + rng.random((n, 3)) * 2 * half).astype(np.float32)


def box_segments(nodes, n: int, seed: int):
    """(a, b) float32 (n, 3): both ends uniform in the top-level root box x 1.25, every second b pushed through a point
    drawn in a random instance's leaf box -- b = a + 2 (point - a), the point at the segment's middle --, so that sparse
    sets are crossed."""
    a = box_points(nodes, n, seed).astype(np.float64)
    b = box_points(nodes, n, seed + 1000).astype(np.float64)
    rng = np.random.default_rng(seed + 2000)
    leaves = nodes[nodes["leaf"] != 0xFFFFFFFF]
    pick = leaves[rng.integers(0, len(leaves), n)]
    through = pick["lo"] + rng.random((n, 3)) * (pick["hi"].astype(np.float64) - pick["lo"])
    aimed = np.arange(n) % 2 == 1
    b[aimed] = (a + 2.0 * (through - a))[aimed]
    return np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)


def surface_segments(arrays, plan, n: int, seed: int):
    """(a, b) float32 (n, 3): both ends are closest-hit positions of instance_oracle.closest for random rays, paired at
    random: the triangles the ends lie on are at r ~ 0 and r ~ 1.  As in segment_cases.surface_segments, a pair whose
    direction makes less than 0.01 (as a sine) with the plane of either end's triangle -- its world normal -- is not taken:
    there r is 0 / 0 and no arithmetic decides it.  For oracle-against-GPU comparisons, word for word."""
    o, d = instance_cases.rays(plan["nodes"], 40 * n, seed)
    res = instance_oracle.closest(arrays, plan, o, d, 100000.0)
    hit = np.flatnonzero(res["hit"].astype(bool) & np.isfinite(res["distance"]) & np.isfinite(res["normal"]).all(axis=1))
    hit = hit[:len(hit) // 2 * 2]
    p = np.ascontiguousarray(res["position"][hit]).astype(np.float64)
    # the plane of an end's triangle in the world: its corners under world_from_object
    W = np.asarray(plan["world_from_object"], np.float64)[res["instance"][hit]]
    corners = arrays.vertices[:, :3][arrays.faces.reshape(-1, 3)[res["leaf"][hit]]].astype(np.float64)
    corners = np.einsum("nij,nkj->nki", W[:, :, :3], corners) + W[:, None, :, 3]
    normal = np.cross(corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0])
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    half = len(hit) // 2
    along = p[half:] - p[:half]
    with np.errstate(all="ignore"):
        along /= np.linalg.norm(along, axis=1, keepdims=True)
        leaves = (np.abs((along * normal[:half]).sum(axis=1)) > 0.01) & (np.abs((along * normal[half:]).sum(axis=1)) > 0.01)
    keep = np.flatnonzero(leaves)[:n]
    assert len(keep) == n, len(keep)
    p32 = p.astype(np.float32)
    return np.ascontiguousarray(p32[:half][keep]), np.ascontiguousarray(p32[half:][keep])


odd_segments = segment_cases.odd_segments  # (a, b, _): in and around the SCENE's root box, where the first copies of a family lie


def nothing_blocks(a, b, nodes, interval) -> np.ndarray:
    """(N,) bool: the segments for which the header DERIVES "nothing blocks" under this interval, for every accepted
    transform: every segment under an interval that blocks nothing; a segment of no length; a NaN coordinate at either end;
    an infinite coordinate of a; an infinite coordinate of b alone where t_lo >= 0, or where the top-level root's two
    differences lo.c - a.c and hi.c - a.c are finite in binary32 for an infinite column c."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if blocks_nothing(interval):
        return np.ones(len(a), bool)
    with np.errstate(all="ignore"):
        no_length = np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1) & (b - a == 0).all(axis=1)
        nan = np.isnan(a).any(axis=1) | np.isnan(b).any(axis=1)
        inf_a = np.isinf(a).any(axis=1)
        inf_b = np.isinf(b) & ~inf_a[:, None] & ~nan[:, None]  # (N, 3): the infinite columns of b alone
        lo, hi = nodes["lo"][0].astype(np.float32), nodes["hi"][0].astype(np.float32)
        finite_differences = np.isfinite(lo[None, :] - a) & np.isfinite(hi[None, :] - a)
    rejected_at_root = (inf_b & finite_differences).any(axis=1)
    r_is_zero_or_nan = inf_b.any(axis=1) & (float(interval[0]) >= 0.0)
    return no_length | nan | inf_a | rejected_at_root | r_is_zero_or_nan
