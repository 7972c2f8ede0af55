"""ctypes view of tests/multihit_oracle.c (the CPU oracle of the multi-hit queries), compiled on first use with the
oracle's flags into a private temporary directory; and the inputs the CPU and GPU tests of the multi-hit queries share:
the layered scene and the ray sets."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import orc
from query_oracle import as4, same_words  # noqa: F401  (same_words: for the tests)

HERE = os.path.dirname(os.path.abspath(__file__))
NONE = 0xFFFFFFFF
MAX_K = 16
SLOT_FIELDS = ("distance", "leaf", "barycentric", "position", "normal")
FIELDS = ("count",) + SLOT_FIELDS
_LIB = None


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        out = os.path.join(tempfile.mkdtemp(prefix="ocrt_multihit_oracle_"), "libmultihit_oracle.so")
        subprocess.run(["gcc", "-std=gnu11", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-fPIC", "-shared",
                        "-o", out, os.path.join(HERE, "multihit_oracle.c"), "-lm"], check=True)
        L = C.CDLL(out)
        S, p = C.POINTER(orc.OrcScene), C.c_void_p
        L.mo_multihit.argtypes = [S, p, p, C.c_uint32, C.c_float, C.c_uint32, p, p, p, p, p, p]
        L.mo_multihit.restype = None
        _LIB = L
    return _LIB


def multihit(arrays, origins, directions, max_distance: float, k: int) -> dict:
    """{"count": (N,), "distance" / "leaf": (N, k), "barycentric" / "position" / "normal": (N, k, 3)}."""
    o4, d4 = as4(origins), as4(directions)
    n = o4.shape[0]
    out = {"count": np.zeros(n, np.uint32), "distance": np.zeros((n, k), np.float32), "leaf": np.zeros((n, k), np.uint32),
           "barycentric": np.zeros((n, k, 3), np.float32), "position": np.zeros((n, k, 3), np.float32),
           "normal": np.zeros((n, k, 3), np.float32)}
    sc = arrays.c_struct()
    lib().mo_multihit(C.byref(sc), o4.ctypes.data, d4.ctypes.data, n, float(max_distance), k,
                      *[out[f].ctypes.data for f in FIELDS])
    return out


def first_slots(full: dict, k: int) -> dict:
    """The answer for k slots from the answer for more: the count, and the first k slots of every ray."""
    return {f: (v if f == "count" else np.ascontiguousarray(v[:, :k])) for f, v in full.items()}


# ---- the layered scene ----------------------------------------------------------------------------------------------
LAYERS = 24
DOUBLED = (1, 5, 9, 13, 17, 21)  # the planes that carry a second, coplanar quad


def layered_mesh():
    """24 planes z = c_j, each an axis-aligned unit quad of two triangles over [-0.5, 0.5]^2; on six of them a second quad
    of the same size with vertices of its own, shifted by half a width in x.  Every coordinate is a small dyadic number,
    so both quads of a plane have the same edge vectors and the same normal (0, 0, nz) bit for bit: a ray through the
    overlap meets two triangles at exactly equal distances."""
    verts, faces = [], []

    def quad(x0, z):
        b = len(verts)
        verts.extend([(x0, -0.5, z), (x0 + 1.0, -0.5, z), (x0 + 1.0, 0.5, z), (x0, 0.5, z)])
        faces.extend([(b, b + 1, b + 2), (b, b + 2, b + 3)])

    for j in range(LAYERS):
        z = (j - 11.5) / 16.0
        quad(-0.5, z)
        if j in DOUBLED:
            quad(0.0, z)
    return np.array(verts, np.float32), np.array(faces, np.uint32)


def layered_scene(rt, bvh: str):
    """(product Scene with BVH, SceneArrays for the oracle)."""
    v, f = layered_mesh()
    scene = rt.Scene.from_arrays(v, f).build_bvh(0 if bvh == "longest" else 1)
    return scene, orc.SceneArrays.from_scene(scene)


def axis_rays(n, seed):
    """Rays along -z and +z through the stack, from both sides, over a rectangle a little larger than the two quads."""
    rng = np.random.default_rng(seed)
    o = np.zeros((n, 3), np.float32)
    o[:, 0] = (-0.6 + 1.7 * rng.random(n)).astype(np.float32)
    o[:, 1] = (-0.6 + 1.2 * rng.random(n)).astype(np.float32)
    down = np.arange(n) % 2 == 0
    o[:, 2] = np.where(down, 2.0, -2.0).astype(np.float32)
    d = np.zeros((n, 3), np.float32)
    d[:, 2] = np.where(down, -1.0, 1.0).astype(np.float32)
    return o, d


def box_of(arrays):
    lo, hi = arrays.aabbs[0, :3], arrays.aabbs[1, :3]
    return lo.astype(np.float64), hi.astype(np.float64)


def random_rays(arrays, n, seed, grow=0.25):
    rng = np.random.default_rng(seed)
    lo, hi = box_of(arrays)
    ext = hi - lo
    o = (lo - grow * ext + rng.random((n, 3)) * (1 + 2 * grow) * ext).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    return o, d.astype(np.float32)


def layered_rays(arrays, n_axis=12000, n_oblique=8000, seed=5):
    ao, ad = axis_rays(n_axis, seed)
    ro, rd = random_rays(arrays, n_oblique, seed + 1)
    return np.concatenate([ao, ro]), np.concatenate([ad, rd]), n_axis


def in_contract_order(res: dict) -> np.ndarray:
    """Per ray: the slots are ascending by (distance, leaf) over the used ones, and the used ones come first."""
    d, leaf = res["distance"], res["leaf"].astype(np.int64)
    if d.shape[1] < 2:
        return np.ones(d.shape[0], bool)
    used = res["leaf"] != NONE
    both = used[:, :-1] & used[:, 1:]
    ascending = (d[:, :-1] < d[:, 1:]) | ((d[:, :-1] == d[:, 1:]) & (leaf[:, :-1] < leaf[:, 1:]))
    no_gap = used[:, :-1] | ~used[:, 1:]
    return (np.where(both, ascending, True) & no_gap).all(axis=1)


def fill_values_hold(res: dict) -> np.ndarray:
    """Per ray: exactly min(k, count) slots are used, and the others hold +inf / NONE / 0."""
    k = res["leaf"].shape[1]
    used = res["leaf"] != NONE
    want = np.arange(k)[None, :] < np.minimum(res["count"], k)[:, None]
    free = ~want
    ok = (used == want).all(axis=1)
    ok &= np.where(free, np.isposinf(res["distance"]), True).all(axis=1)
    for f in ("barycentric", "position", "normal"):
        ok &= np.where(free[:, :, None], res[f].view(np.uint32) == 0, True).all(axis=(1, 2))
    return ok
