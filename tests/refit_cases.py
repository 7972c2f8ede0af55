"""What the vertex-update tests share (tests/test_refit_cpu.py, tests/test_refit_gpu.py): the deformations, an independent
numpy restatement of the refit rule (include/rt_hip_update.h), and the checks of a refit schedule."""
import numpy as np

from conftest import mesh_file

DEFORMATIONS = ("identity", "far", "twist", "collapse", "back")
MOVING = ("far", "twist", "collapse")  # deformations 2-4
LOCAL = 0x80000000


def fresh_scene(rt, mesh: str, bvh: str):
    """A Scene of the test's own (Scene.refit changes it: the session's cached scenes must stay as loaded)."""
    return rt.Scene.load_off(mesh_file(mesh)).build_bvh(0 if bvh == "longest" else 1)


def twist(v: np.ndarray) -> np.ndarray:
    """A twist about y by 1.5 rad per unit of height, and a radial bulge of the (x, z) distance that grows with it; float32
    operations throughout.  Not affine: boxes change shape, and siblings change their order by distance."""
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    angle = np.float32(1.5) * y
    c, s = np.cos(angle).astype(np.float32), np.sin(angle).astype(np.float32)
    bulge = np.float32(1.0) + np.float32(0.75) * np.sqrt(x * x + z * z)
    out = v.copy()
    out[:, 0] = (x * c - z * s) * bulge
    out[:, 2] = (x * s + z * c) * bulge
    return out


def steps(name: str, v: np.ndarray) -> list:
    """The vertex arrays, (V, 4) float32, that deformation `name` of the original `v` applies one after the other."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    if name == "identity":
        return [v.copy()]
    if name == "far":  # far enough that a box left stale misses every ray aimed at the new place, and the other way round
        out = v.copy()
        out[:, :3] += np.array([7.0, -5.0, 3.0], np.float32)
        return [out]
    if name == "twist":
        return [twist(v)]
    if name == "collapse":  # every triangle into the plane z = 0.25: edge-on boxes, u.z = v.z = 0 in every record
        out = v.copy()
        out[:, 2] = np.float32(0.25)
        return [out]
    if name == "back":
        return [twist(v), v.copy()]
    raise KeyError(name)


def deformed(name: str, v: np.ndarray) -> np.ndarray:
    return steps(name, v)[-1]


def children_of(skips: np.ndarray, i: int) -> list:
    out, c = [], i + 1
    while c < i + int(skips[i]):
        out.append(c)
        c += int(skips[c])
    return out


def leaf_indices(skips: np.ndarray, leaf_words=None) -> np.ndarray:
    """The leaf index of every node (0xFFFFFFFF for inner nodes): the leaves in front of it, or the records' own words."""
    if leaf_words is not None:
        return np.asarray(leaf_words, np.uint32)
    is_leaf = skips == 1
    return np.where(is_leaf, np.cumsum(is_leaf) - 1, 0xFFFFFFFF).astype(np.uint32)


def _min(acc, nxt):  # std::min(acc, next): (next < acc) ? next : acc
    return np.where(nxt < acc, nxt, acc)


def _max(acc, nxt):  # std::max(acc, next): (acc < next) ? next : acc
    return np.where(acc < nxt, nxt, acc)


def leaf_boxes(sorted_faces: np.ndarray, vertices: np.ndarray):
    """(lo, hi), (T, 3) each: min(a, min(b, c)), max(a, max(b, c)) per axis of every leaf's three vertices."""
    tri = np.ascontiguousarray(vertices, np.float32)[:, :3][np.asarray(sorted_faces, np.int64).reshape(-1, 3)]
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    return _min(a, _min(b, c)), _max(a, _max(b, c))


def inner_boxes(skips: np.ndarray, lo: np.ndarray, hi: np.ndarray):
    """The refit rule for the inner nodes, in place, in descending index order: the union of the children's boxes from the
    first child on, in index order.  lo, hi: (N, 3), the leaves' rows filled."""
    for i in range(len(skips) - 1, -1, -1):
        if skips[i] == 1:
            continue
        kids = children_of(skips, i)
        l, h = lo[kids[0]].copy(), hi[kids[0]].copy()
        for c in kids[1:]:
            l, h = _min(l, lo[c]), _max(h, hi[c])
        lo[i], hi[i] = l, h
    return lo, hi


def restated_aabbs(skips: np.ndarray, sorted_faces: np.ndarray, vertices: np.ndarray) -> np.ndarray:
    """The aabbs array, (2 N, 4) float32, that the refit rule gives for a scene's own node array."""
    skips = np.asarray(skips, np.uint32)
    n = len(skips)
    lo, hi = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    leaf = leaf_indices(skips)
    at = skips == 1
    llo, lhi = leaf_boxes(sorted_faces, vertices)
    lo[at], hi[at] = llo[leaf[at]], lhi[leaf[at]]
    inner_boxes(skips, lo, hi)
    out = np.zeros((2 * n, 4), np.float32)
    out[0::2, :3], out[1::2, :3] = lo, hi
    return out


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def pass_bound(nodes: int, group_nodes: int) -> int:
    """ceil(log_max(S, 2) N) + 1, in exact integer arithmetic."""
    base, k, power = max(int(group_nodes), 2), 0, 1
    while power < nodes:
        power *= base
        k += 1
    return k + 1


def inner_height(skips: np.ndarray) -> int:
    """The longest chain of inner nodes from the root down (0 where the root is a leaf)."""
    height = np.zeros(len(skips), np.int64)
    for i in range(len(skips) - 1, -1, -1):
        if skips[i] != 1:
            height[i] = 1 + max(height[c] for c in children_of(skips, i))
    return int(height[0]) if len(skips) else 0


def check_schedule(s: dict, group_nodes: int, log_bound: bool = True) -> None:
    """Every inner node once; no group larger than S; every child of a node a leaf, earlier in the same group at a lower
    round, or in a group of an earlier pass; groups in pass order, entries by round.  The pass count: a chain of h inner
    nodes needs ceil(h / S) passes whatever the cut (a pass holds at most S of them, in one group) and never more than h (a
    pass per level does with groups of one); with `log_bound` also at most ceil(log_max(S, 2) N) + 1."""
    skips, entries, children, groups = s["skips"], s["entries"], s["children"], s["groups"]
    n = len(skips)
    inner = np.flatnonzero(skips != 1)
    assert s["group_nodes"] == group_nodes
    assert sorted(entries[:, 0].tolist()) == inner.tolist()
    assert int(groups[:, 1].sum()) == len(entries) and (groups[:, 1] <= group_nodes).all() and (groups[:, 1] >= 1).all()
    assert (np.diff(groups[:, 3].astype(np.int64)) >= 0).all()
    if len(groups):
        assert groups[0, 3] == 1 and groups[-1, 3] == s["passes"] and set(groups[:, 3].tolist()) == set(range(1, s["passes"] + 1))
    else:
        assert s["passes"] == 0 and len(inner) == 0
    pass_of, group_of, slot_of, round_of = {}, {}, {}, {}
    at = 0
    for g, (first, count, rounds, pas) in enumerate(groups.tolist()):
        assert first == at
        at += count
        rs = entries[first:first + count, 3]
        assert (np.diff(rs.astype(np.int64)) >= 0).all() and rs[0] == 0 and rs[-1] == rounds - 1
        for e in range(first, first + count):
            node = int(entries[e, 0])
            pass_of[node], group_of[node], slot_of[node], round_of[node] = pas, g, e - first, int(entries[e, 3])
    for node, first_child, count, rnd in entries.tolist():
        kids = children_of(skips, node)
        refs = children[first_child:first_child + count].tolist()
        assert len(refs) == len(kids) >= 2
        for c, ref in zip(kids, refs):  # in index order
            if skips[c] == 1:
                assert ref == c
            elif ref & LOCAL:
                assert group_of[c] == group_of[node] and slot_of[c] == ref & ~LOCAL
                assert round_of[c] < rnd and slot_of[c] < slot_of[node]
            else:
                assert ref == c and pass_of[c] < pass_of[node]
    height = inner_height(skips)
    assert -(-height // group_nodes) <= s["passes"] <= height, (s["passes"], height, group_nodes)
    if log_bound:
        assert s["passes"] <= pass_bound(n, group_nodes), (s["passes"], pass_bound(n, group_nodes), n, group_nodes)


def node_rule_holds(nodes: np.ndarray, tris: np.ndarray) -> None:
    """Downloaded records: every leaf's box carries the bits of its leaf record's box, every inner box the bits of the
    refit rule applied to its children's boxes as downloaded."""
    skips = nodes["skip"]
    at = skips == 1
    assert np.array_equal(bits(nodes["lo"][at]), bits(tris["lo"][nodes["leaf"][at]]))
    assert np.array_equal(bits(nodes["hi"][at]), bits(tris["hi"][nodes["leaf"][at]]))
    assert (nodes["leaf"][~at] == 0xFFFFFFFF).all()
    lo, hi = nodes["lo"].copy(), nodes["hi"].copy()
    inner_boxes(skips, lo, hi)
    assert np.array_equal(bits(lo), bits(nodes["lo"])) and np.array_equal(bits(hi), bits(nodes["hi"]))
