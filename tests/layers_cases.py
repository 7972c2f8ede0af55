"""The cases the CPU and GPU tests of the frame layers (include/rt_hip_layers.h) share, and their oracle answers.

A case is (mesh, tree, width, height, supersamples, pose name or None, shading, AO rings).  The sizes are the ones at
which layers_kernel can go wrong: 37 x 23 is 5 x 3 tiles, partial on both edges, 15 tiles -- no multiple of the four
waves of a workgroup -- and has a centre row whose cy is -0; 16 x 16 and 8 x 8 are whole tiles; 1 x 1 and 5 x 3 are less
than one; 11 x 6 at 9 supersamples is 33 x 18 sub-pixels; 8 x 8 at 4 is 16 x 16.  The poses are those of
tests/test_camera_gpu.py: poses_for (made for the bunny, a model of unit size around the origin, like the others)."""
import numpy as np

import layers_oracle as lo
import orc

# width, height, supersamples (a square number: the grid is its root)
SIZES = [(37, 23, 1), (16, 16, 1), (8, 8, 1), (1, 1, 1), (5, 3, 1), (11, 6, 9), (8, 8, 4)]
POSES = [None, "orbit_135", "roll", "skewed", "inside_root_box", "far_1e7", "infinite"]
OPTIONS = [(1, 2), (0, 5), (1, 5), (0, 2)]  # shading, AO rings (UNIFORM)
TREES = ["longest", "sah"]
SEES_NOTHING = ("far_1e7", "infinite")  # beyond the primary rays' max_distance / no finite eye: no sub-pixel is hit


def _cases():
    out = []
    k = 0
    for mesh, poses in (("blob", POSES), ("ties", [None, "orbit_135", "roll", "far_1e7"]), ("single", [None, "skewed", "infinite"])):
        for size in SIZES:
            for pose in poses:
                shading, ao = OPTIONS[k % 4]
                out.append((mesh, TREES[(k // 4 + k) % 2], *size, pose, shading, ao))
                k += 1
    for pose in POSES:  # the bunny at 64 x 48, every pose on both trees
        for tree in TREES:
            shading, ao = OPTIONS[k % 4]
            out.append(("bunny", tree, 64, 48, 1, pose, shading, ao))
            k += 1
    return out


CASES = _cases()
# the cases of `ties` (coincident faces) that must show sub-pixels whose two nearest triangles lie at equal distances
TIES_CASES = [c for c in CASES if c[0] == "ties" and c[5] not in SEES_NOTHING and c[2] * c[3] * c[4] >= 500]


def case_id(case) -> str:
    mesh, tree, w, h, ss, pose, shading, ao = case
    return f"{mesh}_{tree}_{w}x{h}_s{ss}_{pose or 'unposed'}_sh{shading}_a{ao}"


def options_of(rt, case, **overrides):
    mesh, tree, w, h, ss, pose, shading, ao = case
    kw = dict(width=w, height=h, n_super_samples=ss, enable_shading=shading, ao_num_samples=ao, enable_ao=int(ao != 0),
              ao_max_distance=1.0 if mesh == "ties" else 0.2, bvh_method=0 if tree == "longest" else 1)
    kw.update(overrides)
    return rt.Options.defaults(**kw)


def camera_of(rt, scene_for, case):
    """The case's Camera, or None for a host without a pose."""
    from test_camera_gpu import poses_for

    if case[5] is None:
        return None
    return poses_for(rt, scene_for("bunny", "longest")[1])[case[5]]


_WANT = {}


def oracle_layers(rt, scene_for, case, **overrides) -> dict:
    """The CPU oracle's layers of a case (tests/layers_oracle.c), computed once and shared: treat them as read-only."""
    key = (case, tuple(sorted(overrides.items())))
    if key not in _WANT:
        _, arrays = scene_for(case[0], case[1])
        want = lo.render(orc.params_from_options(options_of(rt, case, **overrides)), arrays, camera_of(rt, scene_for, case))
        for a in want.values():
            a.setflags(write=False)
        _WANT[key] = want
    return _WANT[key]


def eye_of(rt, scene_for, case) -> np.ndarray:
    cam = camera_of(rt, scene_for, case)
    return np.array([0.0, 0.0, 2.0], np.float32) if cam is None else cam.as_array()[0].astype(np.float32)


def rays_of(rt, scene_for, case, direction) -> tuple:
    """(origins, directions), (N, 3) each: the eye and a `direction` layer as rays for the queries."""
    d = np.ascontiguousarray(direction, np.float32).reshape(-1, 3)
    return np.ascontiguousarray(np.broadcast_to(eye_of(rt, scene_for, case), d.shape)), d


def must_see_both(case) -> bool:
    """Whether the case must hold hit and missed sub-pixels alike (every one that is not a single sub-pixel or an eye that
    sees nothing)."""
    return case[5] not in SEES_NOTHING and (case[2], case[3]) != (1, 1)
