"""The cases the signed distance tests share (tests/test_signed_cpu.py, tests/test_signed_gpu.py): the two closed meshes the
repository otherwise lacks, their reversed copies, and the per-feature point set.  Deterministic; float32 on the way out."""
import numpy as np

import signed_reference as sref


def torus(R: float = 1.0, r: float = 0.4, around: int = 24, across: int = 12):
    """(vertices (around * across, 3), faces (2 * around * across, 3)): closed, outward oriented; 576 faces by default."""
    i, j = np.meshgrid(np.arange(around), np.arange(across), indexing="ij")
    theta, phi = 2.0 * np.pi * i / around, 2.0 * np.pi * j / across
    v = np.stack([(R + r * np.cos(phi)) * np.cos(theta), (R + r * np.cos(phi)) * np.sin(theta), r * np.sin(phi)], axis=-1).reshape(-1, 3)
    at = lambda a, b: (a % around) * across + (b % across)
    faces = []
    for a in range(around):
        for b in range(across):
            faces.append([at(a, b), at(a + 1, b), at(a + 1, b + 1)])
            faces.append([at(a, b), at(a + 1, b + 1), at(a, b + 1)])
    return v.astype(np.float32), np.array(faces, np.uint32)


def star(points: int = 7, outer: float = 1.0, inner: float = 0.4, above: float = 0.6, below: float = -0.46):
    """A star-shaped outline in the plane z = 0 joined to an apex above and one below: 2 * points + 2 vertices, 4 * points
    faces; closed, outward oriented.  Reflex edges run from the inner vertices to both apexes, convex ones from the outer."""
    n = 2 * points
    k = np.arange(n)
    radius = np.where(k % 2 == 0, outer, inner)
    ring = np.stack([radius * np.cos(np.pi * k / points), radius * np.sin(np.pi * k / points), np.zeros(n)], axis=-1)
    v = np.concatenate([ring, [[0.0, 0.0, above], [0.0, 0.0, below]]])
    faces = []
    for a in range(n):
        b = (a + 1) % n
        faces.append([a, b, n])      # counter-clockwise seen from above
        faces.append([b, a, n + 1])  # ... and from below
    return v.astype(np.float32), np.array(faces, np.uint32)


def reversed_faces(faces) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(faces).reshape(-1, 3)[:, ::-1])


def signed_volume(vertices, faces) -> float:
    v = np.asarray(vertices, np.float64)[:, :3]
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return float((v[f[:, 0]] * np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


def edge_uses(faces) -> dict:
    uses = {}
    for a, b, c in np.asarray(faces, np.int64).reshape(-1, 3):
        for x, y in ((a, b), (a, c), (b, c)):
            key = (min(int(x), int(y)), max(int(x), int(y)))
            uses[key] = uses.get(key, 0) + 1
    return uses


def sheared(vertices) -> np.ndarray:
    """A sheared, stretched copy: every normal and angle changes, the topology stays."""
    v = np.asarray(vertices, np.float32)[:, :3].copy()
    out = v.copy()
    out[:, 0] = v[:, 0] + np.float32(0.35) * v[:, 2]
    out[:, 1] = np.float32(1.25) * v[:, 1] - np.float32(0.2) * v[:, 0]
    return out


def per_feature(vertices, faces, offset: float = 1e-2):
    """(points (2 (V + E + F), 3) float32, kinds): every vertex, edge midpoint and face centroid, displaced by +offset and by
    -offset along the float64 pseudonormal of the feature.  Half of them lie inside a closed outward mesh."""
    pn = sref.Pseudonormals(vertices, faces)
    at, normal, kinds = [], [], []
    for x in range(len(pn.v)):
        if x in pn.vertex:
            at.append(pn.v[x]), normal.append(pn.vertex[x]), kinds.append("vertex")
    for x, y in pn.edges():
        at.append((pn.v[x] + pn.v[y]) / 2.0), normal.append(pn.edge[(x, y)]), kinds.append("edge")
    for k, ids in enumerate(pn.f):
        at.append(pn.v[ids].mean(axis=0)), normal.append(pn.face[k]), kinds.append("face")
    at, normal = np.array(at), np.array(normal)
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    return np.concatenate([at + offset * normal, at - offset * normal]).astype(np.float32), kinds + kinds
