"""The cases the instanced closest-point tests share (tests/test_instance_nearest_cpu.py, tests/test_instance_nearest_gpu.py):
a mesh with a tree and what the oracle and the reference each need of it, the plan of a set, and world-space point sets.
Transforms come from tests/instance_cases.py, meshes, radii and odd points from tests/nearest_cases.py.  Deterministic."""
import numpy as np

import instance_cases as ic
import instance_nearest_oracle as ino
import instance_nearest_reference as inref
import nearest_cases as cases


class Mesh:
    """A scene with its tree: leaf order for the oracle, file order for the reference."""

    def __init__(self, scene):
        self.scene = scene
        self.vertices, self.vnormals = scene.vertices.copy(), scene.vnormals.copy()
        self.faces = scene.faces.reshape(-1, 3).copy()
        self.leaf_faces = scene.sorted_faces.copy()
        self.face_of_leaf = scene.face_of_leaf().copy()
        self.leaves = len(self.face_of_leaf)

    def root_box(self):
        return ic.root_box(self.scene)  # (the root node's box, as the device holds it)

    def family(self, name):
        return ic.family(name, self.scene)

    def plan(self, rt, W) -> dict:
        lo, hi = self.root_box()
        plan = rt.instance_plan(lo, hi, W)
        plan["world_from_object"] = np.ascontiguousarray(W, np.float32)
        return plan

    def oracle(self, plan, points, radius=np.inf) -> dict:
        return ino.closest_points(self.leaf_faces, self.vertices, self.vnormals, plan["world_from_object"], plan["object_from_world"],
                                  points, radius)

    def compare(self, plan, points, radius, answer, pairs=None) -> dict:
        return inref.compare(points, self.vertices, self.vnormals, self.faces, self.face_of_leaf, plan["world_from_object"], radius,
                             answer, pairs=pairs)

    def pairs(self, plan, points):
        return inref.pair_distances(points, self.vertices, self.faces, plan["world_from_object"])


def handcrafted_mesh(rt, method: int = 0) -> Mesh:
    v, f = cases.handcrafted()
    return Mesh(rt.Scene.from_arrays(v, f).build_bvh(method))


def in_top_box(plan, count: int, seed: int, factor: float = 1.25) -> np.ndarray:
    """`count` points uniform in the top-level root box scaled by `factor` about its centre."""
    lo, hi = ic.top_box(plan["nodes"])
    rng = np.random.default_rng(seed)
    return ((lo + hi) / 2 + (rng.random((count, 3)) * 2 - 1) * (hi - lo) / 2 * factor).astype(np.float32)


def on_world_surface(mesh: Mesh, plan, count: int, seed: int) -> np.ndarray:
    """Vertices, edge midpoints and centroids of the copies' float64 triangles, rounded to float32."""
    mv, _, mf = inref.merged_mesh(mesh.vertices, mesh.vnormals, mesh.faces, plan["world_from_object"])
    return cases.on_surface(mv, mf, count, seed)


def far_from_set(plan, count: int, seed: int, sizes: float = 1e3) -> np.ndarray:
    """`count` points `sizes` top-level box sizes from its centre, in random directions."""
    lo, hi = ic.top_box(plan["nodes"])
    return cases.far_away(np.stack([lo, hi]), count, seed, sizes)


def odd_points(plan) -> np.ndarray:
    lo, hi = ic.top_box(plan["nodes"])
    return cases.odd_points(np.stack([lo, hi]))


def mixed_points(mesh: Mesh, plan, n_box: int, n_surface: int, n_far: int, seed: int) -> np.ndarray:
    return np.concatenate([in_top_box(plan, n_box, seed), on_world_surface(mesh, plan, n_surface, seed + 1),
                           far_from_set(plan, n_far, seed + 2), far_from_set(plan, n_far, seed + 3, sizes=2.0)])


def write_scene_file(path: str, mesh: Mesh, W) -> None:
    """What tests/instance_nearest_margin_check.cc reads: the tree, the leaf-ordered faces, the vertices, the transforms."""
    nodes, aabbs = mesh.scene.nodes, mesh.scene.aabbs
    W = np.ascontiguousarray(W, np.float32).reshape(-1, 12)
    with open(path, "wb") as out:
        np.array([len(nodes), mesh.leaves, len(mesh.vertices), len(W)], np.uint32).tofile(out)
        np.ascontiguousarray(nodes, np.uint32).tofile(out)
        np.ascontiguousarray(aabbs, np.float32).tofile(out)
        np.ascontiguousarray(mesh.leaf_faces, np.uint32).tofile(out)
        np.ascontiguousarray(mesh.vertices, np.float32).tofile(out)
        W.tofile(out)
