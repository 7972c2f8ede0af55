"""What the tests of device-side instance sets share (tests/test_instance_build_cpu.py, tests/test_instance_build_gpu.py;
include/rt_hip_instance_build.h): an independent numpy restatement of the tree that header defines -- the leaf boxes taken
from the host planner's tree (rt.instance_plan: the same six floats per instance), keys by the formula, np.lexsort for the
order, the shape TOP-DOWN by the highest differing bit, skips, pre-order and the inner boxes from the recursion (the library
searches per node, bottom-up links, a count and arrival counters: lbvh.h, kernels/instance_build.hip.h) -- and the sets the
tests build.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import instance_cases as cases

NONE = 0xFFFFFFFF
COUNTS = (1, 2, 3, 64, 65, 257, 1000)


def leaf_boxes_of(nodes, n: int):
    """(lo, hi) float32 (n, 3) by instance index, the bits as they lie in a tree's leaf records."""
    leaves = nodes[nodes["leaf"] != NONE]
    assert sorted(leaves["leaf"].tolist()) == list(range(n))
    lo, hi = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    lo[leaves["leaf"]], hi[leaves["leaf"]] = leaves["lo"], leaves["hi"]
    return lo, hi


def keys_of(lo: np.ndarray, hi: np.ndarray) -> np.ndarray:
    """The 30-bit key of every leaf box over the per-axis minimum and maximum of all of them."""
    root_lo, root_hi = lo.min(axis=0), hi.max(axis=0)
    with np.errstate(all="ignore"):
        centre = (lo + hi) * np.float32(0.5)
    assert centre.dtype == np.float32
    key = np.zeros(len(lo), np.uint32)
    for axis, shift in ((0, 2), (1, 1), (2, 0)):
        with np.errstate(all="ignore"):
            extent = np.float32(root_hi[axis] - root_lo[axis])
        cell = np.zeros(len(lo), np.uint32)
        if extent > 0 and np.isfinite(extent):
            with np.errstate(all="ignore"):
                x = (centre[:, axis] - root_lo[axis]) * (np.float32(1024.0) / extent)
            assert x.dtype == np.float32
            cell = np.where(np.isnan(x), np.float32(0), np.clip(x, np.float32(0), np.float32(1023))).astype(np.uint32)  # (truncates)
        for b in range(10):
            key |= ((cell >> np.uint32(b)) & np.uint32(1)) << np.uint32(3 * b + shift)
    return key


def restate(lo: np.ndarray, hi: np.ndarray, node_dtype) -> dict:
    """{"nodes": the records in pre-order, "keys": sorted, "order": the instance of every rank} from the leaf boxes by instance."""
    n = len(lo)
    keys = keys_of(lo, hi)
    order = np.lexsort((np.arange(n), keys)).astype(np.uint32)
    sorted_keys = keys[order]
    words = (sorted_keys.astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    nodes = np.zeros(2 * n - 1, node_dtype)
    counter = [0]

    def emit(l: int, r: int) -> int:  # pre-order: a node, its first child's subtree, its second child's
        at = counter[0]
        counter[0] += 1
        if l == r:
            k = int(order[l])
            nodes["lo"][at], nodes["hi"][at], nodes["skip"][at], nodes["leaf"][at] = lo[k], hi[k], 1, k
            return at
        bit = (int(words[l]) ^ int(words[r])).bit_length() - 1  # the highest bit in which the words of l and r differ
        boundary = ((int(words[l]) >> bit) | 1) << bit          # the first word that has it set
        split = l + int(np.searchsorted(words[l:r + 1], np.uint64(boundary))) - 1
        assert l <= split < r
        a, b = emit(l, split), emit(split + 1, r)
        first, second = nodes[a], nodes[b]
        # by comparison, the first child's value where two compare equal
        nodes["lo"][at] = np.where(second["lo"] < first["lo"], second["lo"], first["lo"])
        nodes["hi"][at] = np.where(first["hi"] < second["hi"], second["hi"], first["hi"])
        nodes["skip"][at], nodes["leaf"][at] = 2 * (r - l + 1) - 1, NONE
        return at

    import sys

    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 4 * n + 1000))  # (equal keys: a chain as deep as the set)
    try:
        emit(0, n - 1)
    finally:
        sys.setrecursionlimit(limit)
    assert counter[0] == 2 * n - 1
    return {"nodes": nodes, "keys": sorted_keys, "order": order}


def restated_plan(rt, root_lo, root_hi, W) -> dict:
    """The plan include/rt_hip_instance_build.h defines, restated: the inverses and leaf boxes of rt.instance_plan (the host
    planner's), the tree by restate()."""
    host = rt.instance_plan(root_lo, root_hi, W)
    lo, hi = leaf_boxes_of(host["nodes"], len(W))
    out = restate(lo, hi, rt.INSTANCE_NODE)
    out["object_from_world"] = host["object_from_world"]
    return out


def identical(arrays, n: int) -> np.ndarray:
    """n copies of one transform: every key equal."""
    return np.ascontiguousarray(np.repeat(cases.family("rotations", arrays)[1:2], n, axis=0))


def sets(arrays) -> dict:
    """name -> float32 (n, 3, 4): every family of instance_cases, the hard ones among them, and cases.many at COUNTS."""
    out = {name: cases.family(name, arrays) for name in cases.FAMILIES + cases.HARD_FAMILIES}
    for n in COUNTS:
        out[f"many{n}"] = cases.many(arrays, n, seed=n)
    out["identical70"] = identical(arrays, 70)
    return out


def bad_transforms(arrays) -> dict:
    """The refusals of the header: NaN, inf, singular, an inverse that overflows -- each a (3, 4) float32."""
    odd = cases.odd_transforms(arrays)
    return {k: odd[k][0] for k in ("nan", "inf", "singular", "inverse_overflows")}
