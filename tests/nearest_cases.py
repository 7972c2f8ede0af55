"""The cases the closest-point tests share (tests/test_nearest_cpu.py, tests/test_nearest_gpu.py): meshes, point sets, radii
and odd inputs.  Deterministic; everything is float32 by the time it leaves this file."""
import numpy as np

RADII = (np.inf, 0.3, 0.02, 0.0)
ODD_RADII = (-1.0, -0.0, np.nan, -np.inf)  # (-0.0 is a radius of 0: the contract compares `>= 0`)


def handcrafted():
    """(vertices (V, 3), faces (F, 3)): a point triangle, a needle, and two coincident triangles -- the same three vertices
    listed twice, once more with the vertices' own copies --, so that leaves tie exactly and the lowest must win."""
    v = np.array([
        [0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0],              # 0-2: the coincident pair's triangle
        [0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0],              # 3-5: its copy
        [2.0, 2.0, 2.0],                                                 # 6: the point triangle
        [-1.0, -1.0, 0.5], [3.0, -1.0, 0.5], [1.0, -1.0 + 1e-6, 0.5],   # 7-9: the needle (a sliver 4 long, 1e-6 high)
        [0.5, 0.5, -1.0], [0.5, 0.5, -1.0], [0.5, 1.5, -1.0],           # 10-12: a segment (two vertices coincide)
    ], dtype=np.float32)
    f = np.array([[0, 1, 2], [3, 4, 5], [0, 1, 2], [6, 6, 6], [7, 8, 9], [10, 11, 12], [12, 10, 11]], dtype=np.uint32)
    return v, f


def box_of(vertices):
    v = np.asarray(vertices, dtype=np.float64)[:, :3]
    return v.min(axis=0), v.max(axis=0)


def in_box(vertices, count: int, seed: int, factor: float = 1.5) -> np.ndarray:
    """`count` points uniform in the mesh's box scaled by `factor` about its centre (a box without extent gets one of 1)."""
    lo, hi = box_of(vertices)
    centre, half = (lo + hi) / 2.0, np.maximum((hi - lo) / 2.0, 0.5 * ((hi - lo) <= 0.0))
    rng = np.random.default_rng(seed)
    return (centre + (rng.random((count, 3)) * 2.0 - 1.0) * half * factor).astype(np.float32)


def on_surface(vertices, faces, count: int, seed: int) -> np.ndarray:
    """Thirds of `count`: vertices, edge midpoints, centroids (rounded to float32: on the surface up to that)."""
    v = np.asarray(vertices, dtype=np.float64)[:, :3]
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    third = count // 3
    picks = rng.integers(0, f.shape[0], size=count)
    corner = rng.integers(0, 3, size=count)
    tri = v[f[picks]]
    at_vertex = tri[np.arange(count), corner]
    midpoint = (tri[np.arange(count), corner] + tri[np.arange(count), (corner + 1) % 3]) / 2.0
    centroid = tri.mean(axis=1)
    out = np.where((np.arange(count) < third)[:, None], at_vertex, np.where((np.arange(count) < 2 * third)[:, None], midpoint, centroid))
    return out.astype(np.float32)


def far_away(vertices, count: int, seed: int, sizes: float = 1e3) -> np.ndarray:
    """`count` points `sizes` box sizes from the mesh's centre, in random directions."""
    lo, hi = box_of(vertices)
    size = float(np.linalg.norm(hi - lo)) or 1.0
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(count, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return ((lo + hi) / 2.0 + d * size * sizes).astype(np.float32)


def shell(vertices, count: int, seed: int, sizes: float = 2.0) -> np.ndarray:
    return far_away(vertices, count, seed, sizes)


def odd_points(vertices) -> np.ndarray:
    """Points the contract finds nothing for -- a NaN or infinite coordinate -- between ordinary ones."""
    p = in_box(vertices, 12, 7)
    p[1, 0] = np.nan
    p[3, 1] = np.inf
    p[5, 2] = -np.inf
    p[7] = np.nan
    p[9, 0], p[9, 1] = np.inf, np.nan
    return p


def region_shares(barycentric) -> tuple:
    """Shares of the answers nearest to a vertex, an edge's interior, a face's interior -- by the zeros among the
    barycentrics (edge BC's first one is 1 - (1 - k) - k: zero up to a rounding)."""
    zeros = (np.abs(np.asarray(barycentric)) < 1e-6).sum(axis=1)
    n = float(len(zeros))
    return (zeros == 2).sum() / n, (zeros == 1).sum() / n, (zeros == 0).sum() / n
