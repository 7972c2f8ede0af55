"""What the device-side-build tests share (tests/test_build_cpu.py, tests/test_build_gpu.py): the meshes, and an independent
numpy restatement of the tree include/rt_hip_build.h defines -- keys by the formula, np.lexsort for the order, the shape
TOP-DOWN by the highest differing bit, skips and pre-order from the recursion (the library searches per node, bottom-up
links and a count: lbvh.h)."""
import functools

import numpy as np

import layers_oracle as lo
import multihit_oracle as mo
import orc
import query_oracle as qo
import refit_cases as rc
from conftest import mesh_file

FILE_MESHES = ("single", "ties", "blob", "bunny")
MADE_MESHES = ("stack", "flat", "pair", "strip")
MESHES = FILE_MESHES + MADE_MESHES
SMALL_MESHES = tuple(m for m in MESHES if m != "bunny")


def _pad4(v) -> np.ndarray:
    v = np.asarray(v, np.float32)
    out = np.zeros((len(v), 4), np.float32)
    out[:, :v.shape[1]] = v
    return out


def made_mesh(name: str):
    if name == "stack":  # 70 copies of one triangle: every key equal, the order by face id crosses a wave boundary
        return _pad4([[0.1, 0.2, 0.3], [0.9, 0.1, 0.4], [0.3, 0.8, 0.2]]), np.tile(np.array([[0, 1, 2]], np.uint32), (70, 1))
    if name == "pair":
        return _pad4([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5]]), np.array([[0, 1, 2], [1, 3, 2]], np.uint32)
    if name == "flat":  # a 9 x 7 grid of vertices in z = 0: no extent on one axis
        xs, ys = np.meshgrid(np.arange(9, dtype=np.float32) * np.float32(0.37), np.arange(7, dtype=np.float32) * np.float32(0.53))
        v = _pad4(np.stack([xs.ravel(), ys.ravel(), np.zeros(63, np.float32)], axis=1))
        f = []
        for y in range(6):
            for x in range(8):
                a = y * 9 + x
                f += [[a, a + 1, a + 9], [a + 1, a + 10, a + 9]]
        return v, np.array(f, np.uint32)
    if name == "strip":  # 257 triangles: one past a workgroup of 256 lanes
        k = np.arange(259)
        v = _pad4(np.stack([k * 0.25, (k % 2) * 1.0 + 0.01 * k, np.sin(k * 0.3)], axis=1).astype(np.float32))
        return v, np.stack([k[:-2], k[1:-1], k[2:]], axis=1).astype(np.uint32)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _mesh(name: str):
    if name in MADE_MESHES:
        v, f = made_mesh(name)
    else:
        import opencl_raytracer_amd as rt

        scene = rt.Scene.load_off(mesh_file(name))
        v, f = scene.vertices.copy(), scene.faces.reshape(-1, 3).copy()
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


def mesh(name: str):
    """(vertices (V, 4) float32, faces (F, 3) uint32), read-only and shared."""
    return _mesh(name)


def keys_of(vertices: np.ndarray, faces: np.ndarray) -> np.ndarray:
    """The 30-bit key of every face, in file order."""
    lo, hi = rc.leaf_boxes(np.asarray(faces).reshape(-1), vertices)
    root_lo, root_hi = lo.min(axis=0), hi.max(axis=0)
    centre = (lo + hi) * np.float32(0.5)
    assert centre.dtype == np.float32
    key = np.zeros(len(lo), np.uint32)
    for axis, shift in ((0, 2), (1, 1), (2, 0)):
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


@functools.lru_cache(maxsize=None)
def _restated(name: str):
    v, f = mesh(name)
    return restate(v, f)


def restated(name: str) -> dict:
    """restate() of a named mesh, computed once."""
    return _restated(name)


def restate(vertices: np.ndarray, faces: np.ndarray) -> dict:
    """{"keys": sorted, "triangles": the face of every leaf, "nodes": skips in pre-order, "leaf": the records' leaf words,
    "leaf_node": the node of every leaf}."""
    keys = keys_of(vertices, faces)
    order = np.lexsort((np.arange(len(keys)), keys)).astype(np.uint32)
    sorted_keys = keys[order]
    n = len(order)
    words = (sorted_keys.astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    nodes, leaf, leaf_node = np.zeros(2 * n - 1, np.uint32), np.full(2 * n - 1, 0xFFFFFFFF, np.uint32), np.zeros(n, np.uint32)
    at, stack = 0, [(0, n - 1)]
    while stack:  # pre-order: a node, its first child's subtree, its second child's
        l, r = stack.pop()
        if l == r:
            nodes[at], leaf[at], leaf_node[l] = 1, l, at
        else:
            nodes[at] = 2 * (r - l + 1) - 1
            bit = (int(words[l]) ^ int(words[r])).bit_length() - 1  # the highest bit in which the keys of l and r differ
            boundary = ((int(words[l]) >> bit) | 1) << bit          # the first word that has it set
            split = l + int(np.searchsorted(words[l:r + 1], np.uint64(boundary))) - 1
            assert l <= split < r
            stack.append((split + 1, r))
            stack.append((l, split))
        at += 1
    assert at == 2 * n - 1
    return {"keys": sorted_keys, "triangles": order, "nodes": nodes, "leaf": leaf, "leaf_node": leaf_node}


def lbvh_scene(rt, name: str):
    v, f = mesh(name)
    return rt.Scene.from_arrays(v, f).build_lbvh()


def longest_scene(rt, name: str):
    v, f = mesh(name)
    return rt.Scene.from_arrays(v, f).build_bvh(0)


def two_poses(rt, arrays):
    lo_, hi_ = mo.box_of(arrays)
    centre, size = (lo_ + hi_) / 2, float(np.max(hi_ - lo_))
    return [rt.Camera.look_at(tuple(centre + np.array(e) * size), tuple(centre)) for e in ((0.3, 0.4, 1.6), (-1.5, 0.2, -0.7))]


def rays_for(rt, arrays, w=48, h=36):
    """The rays of the cross-builder checks: the camera rays of two poses around the mesh, and 4 096 random rays in and
    around its box with odd ones among them (zero components, huge and tiny directions, origins far away and at infinity)."""
    params = orc.params_from_options(rt.Options.defaults(width=w, height=h, n_super_samples=1, ao_num_samples=3, ao_max_distance=0.2))
    origins, directions = [], []
    for pose in two_poses(rt, arrays):
        d = lo.render(params, arrays, pose)["direction"].reshape(-1, 3)
        origins.append(np.tile(np.asarray(pose.eye, np.float32), (len(d), 1)))
        directions.append(d)
    ro, rd = mo.random_rays(arrays, 4096, 17)
    ro, rd = ro[:, :3].copy(), rd[:, :3].copy()
    k = np.arange(len(ro))
    rd[k % 7 == 0, 1] = 0.0
    rd[k % 11 == 0, 2] = -0.0
    rd[k % 13 == 0] *= np.float32(1e20)
    rd[k % 17 == 0] *= np.float32(1e-20)
    ro[k % 29 == 0, 0] += np.float32(50.0)
    # (no coordinate that is not a number: such a ray's hits all lie at distance inf or NaN, none is nearer than another, and
    # which one an oracle reports is its walk order's -- the tie rule speaks of distances that compare)
    ro[k % 47 == 0, 0] = np.inf
    origins.append(ro)
    directions.append(rd)
    return qo.as4(np.concatenate(origins)), qo.as4(np.concatenate(directions))


def tie_rays(arrays, o4, d4) -> np.ndarray:
    """Rays whose two nearest accepted distances, by the multi-hit oracle, are equal floats."""
    two = mo.multihit(arrays, o4, d4, 100000.0, 2)
    return (two["count"] >= 2) & (two["distance"][:, 0] == two["distance"][:, 1])
