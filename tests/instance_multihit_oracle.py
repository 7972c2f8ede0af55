"""ctypes view of tests/instance_multihit_oracle.c (the CPU oracle of the instanced multi-hit queries,
include/rt_hip_instance_multihit.h), compiled on first use with the oracle's flags into a private temporary directory; and
what the CPU and GPU tests of those queries share: the layered stack as an instanced scene, and the checks on an answer's
own order and fill values."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import multihit_oracle as mo
import orc
from query_oracle import as4, same_words  # noqa: F401  (same_words: for the tests)

HERE = os.path.dirname(os.path.abspath(__file__))
NONE = 0xFFFFFFFF
MAX_K = 16
SLOT_FIELDS = mo.SLOT_FIELDS + ("instance",)
FIELDS = ("count",) + SLOT_FIELDS
_LIB = None


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        out = os.path.join(tempfile.mkdtemp(prefix="ocrt_instance_multihit_oracle_"), "libinstance_multihit_oracle.so")
        subprocess.run(["gcc", "-std=gnu11", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-fPIC", "-shared",
                        "-o", out, os.path.join(HERE, "instance_multihit_oracle.c"), "-lm"], check=True)
        L = C.CDLL(out)
        S, p, u, f = C.POINTER(orc.OrcScene), C.c_void_p, C.c_uint32, C.c_float
        L.im_multihit.argtypes = [S, p, u, p, p, p, u, f, u, p, p, p, p, p, p, p]
        L.im_multihit.restype = None
        _LIB = L
    return _LIB


def multihit(arrays, plan, origins, directions, max_distance: float, k: int) -> dict:
    """{"count": (N,), "distance" / "leaf" / "instance": (N, k), "barycentric" / "position" / "normal": (N, k, 3)} on the plan
    -- host.instances() or rt.instance_plan() -- it is handed."""
    nodes = np.ascontiguousarray(plan["nodes"])
    inverse = np.ascontiguousarray(plan["object_from_world"], np.float32)
    assert nodes.dtype.itemsize == 32 and len(nodes) == 2 * len(inverse) - 1
    o4, d4 = as4(origins), as4(directions)
    n = o4.shape[0]
    out = {"count": np.zeros(n, np.uint32), "distance": np.zeros((n, k), np.float32), "leaf": np.zeros((n, k), np.uint32),
           "barycentric": np.zeros((n, k, 3), np.float32), "position": np.zeros((n, k, 3), np.float32),
           "normal": np.zeros((n, k, 3), np.float32), "instance": np.zeros((n, k), np.uint32)}
    sc = arrays.c_struct()
    lib().im_multihit(C.byref(sc), nodes.ctypes.data, len(nodes), inverse.ctypes.data, o4.ctypes.data, d4.ctypes.data, n,
                      float(max_distance), k, *[out[f].ctypes.data for f in FIELDS])
    return out


def first_slots(full: dict, k: int) -> dict:
    """The answer for k slots from the answer for more: the count, and the first k slots of every ray."""
    return {f: (v if f == "count" else np.ascontiguousarray(v[:, :k])) for f, v in full.items()}


def assert_same(got: dict, want: dict, what="") -> None:
    for f in got:
        ok = same_words(got[f], want[f])
        assert ok.all(), (what, f, int((~ok).sum()), np.argwhere(~ok)[:5].tolist())


def in_contract_order(res: dict) -> np.ndarray:
    """Per ray: the used slots come first and ascend by (distance, instance, leaf)."""
    d, inst, leaf = res["distance"], res["instance"].astype(np.int64), res["leaf"].astype(np.int64)
    if d.shape[1] < 2:
        return np.ones(d.shape[0], bool)
    used = res["leaf"] != NONE
    both = used[:, :-1] & used[:, 1:]
    lower = (inst[:, :-1] < inst[:, 1:]) | ((inst[:, :-1] == inst[:, 1:]) & (leaf[:, :-1] < leaf[:, 1:]))
    ascending = (d[:, :-1] < d[:, 1:]) | ((d[:, :-1] == d[:, 1:]) & lower)
    no_gap = used[:, :-1] | ~used[:, 1:]
    return (np.where(both, ascending, True) & no_gap).all(axis=1)


def fill_values_hold(res: dict) -> np.ndarray:
    """Per ray: exactly min(k, count) slots are used, and the others hold +inf / NONE / NONE / 0."""
    ok = mo.fill_values_hold(res)
    return ok & ((res["instance"] == NONE) == (res["leaf"] == NONE)).all(axis=1)


# ---- the layered stack under an instance set ------------------------------------------------------------------------
def layered_rays(plan, arrays, W, n_axis=3000, n_oblique=1500, seed=5):
    """multihit_oracle.layered_rays's two sets in WORLD space: its axis rays carried along by the first transform (they run
    down the first copy's stack, and through whatever other copy overlaps it), and random rays over the top-level root box.
    Returns (origins, directions, n_axis)."""
    import instance_cases as ic

    ao, ad = mo.axis_rays(n_axis, seed)
    w = np.asarray(W[0], np.float64)
    wo = ao.astype(np.float64) @ w[:, :3].T + w[:, 3]
    wd = ad.astype(np.float64) @ w[:, :3].T
    ro, rd = ic.rays(plan["nodes"], n_oblique, seed + 1)
    return (np.ascontiguousarray(np.concatenate([wo.astype(np.float32), ro])),
            np.ascontiguousarray(np.concatenate([wd.astype(np.float32), rd])), n_axis)
