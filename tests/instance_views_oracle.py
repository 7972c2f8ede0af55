"""The expected values of instanced ambient occlusion and instanced views (include/rt_hip_instance_views.h) BY COMPOSITION of
the oracles the project has: the ambient-occlusion rays of tests/directional_oracle.c (or the rays host.ao_rays() wrote out),
the instanced walk of tests/instance_oracle.c on a plan read back from a host (or made by rt.instance_plan), the camera rays
of tests/layers_oracle.c, and numpy float32 for what the header states operation by operation.  No C oracle of its own.
TEST INFRASTRUCTURE ONLY."""
import numpy as np

import directional_oracle as do
import instance_cases as cases
import instance_oracle as io
import layers_oracle as lo
import orc
from camera_oracle import pose_array
from query_oracle import same_words  # noqa: F401

RECORD = ("hit", "distance", "leaf", "barycentric", "position", "normal", "instance")
LAYERS = RECORD + ("direction", "shade", "ao", "value")
F1 = np.float32(1.0)


def ao_divisor(params, rays: int) -> int:
    """The n of `1 - hits / n` (rt_ao_rays_per_point's divisor)."""
    return rays if params.ao_method == 0 else params.ao_num_samples + 1


def ao_rays(params, arrays, points, normals, seeds=None):
    """(origins (N, 3), directions (N, R, 3)) the oracle's ambient_occlusion casts: they do not depend on the scene."""
    d = do.directional(params, arrays, points, normals, seeds)
    return d["origins"], d["directions"]


def ao(params, arrays, plan, points, normals, seeds=None, rays=None) -> dict:
    """{"occluded": uint32 (N,), "ao": float32 (N,)}: every ray of every point through instance_oracle.occluded with
    ao_max_distance, summed per point.  `rays`: (origins, directions) to use instead of the oracle's -- the RANDOM method's
    sampler depends on the device's libm, so its rays come from host.ao_rays()."""
    n = len(points)
    if n == 0:
        return {"occluded": np.zeros(0, np.uint32), "ao": np.zeros(0, np.float32)}
    origins, directions = ao_rays(params, arrays, points, normals, seeds) if rays is None else rays
    origins, directions = np.asarray(origins, np.float32)[:, :3], np.asarray(directions, np.float32)[..., :3]
    per = directions.shape[1]
    o = np.ascontiguousarray(np.repeat(origins, per, axis=0))
    d = np.ascontiguousarray(directions.reshape(n * per, 3))
    flags = io.occluded(arrays, plan, o, d, params.ao_max_distance)
    occluded = flags.reshape(n, per).sum(axis=1, dtype=np.uint32)
    with np.errstate(all="ignore"):
        factor = F1 - occluded.astype(np.float32) / np.float32(ao_divisor(params, per))
    return {"occluded": occluded, "ao": factor.astype(np.float32)}


def shade(normal, direction, hit, shading: bool) -> np.ndarray:
    """min(max(-dot(normal, direction), 0), 1) in dot3's order with fmaxf / fminf (a NaN operand loses); 1 without shading;
    0 without a hit."""
    n, d = np.asarray(normal, np.float32), np.asarray(direction, np.float32)
    with np.errstate(all="ignore"):
        dot = ((n[..., 0] * d[..., 0]).astype(np.float32) + (n[..., 1] * d[..., 1]).astype(np.float32)).astype(np.float32)
        dot = (dot + (n[..., 2] * d[..., 2]).astype(np.float32)).astype(np.float32)
        lit = np.fmin(np.fmax(-dot, np.float32(0.0)), F1).astype(np.float32)
    if not shading:
        lit = np.ones_like(lit)
    return np.where(np.asarray(hit).astype(bool), lit, np.float32(0.0)).astype(np.float32)


def camera_rays(params, arrays, pose):
    """(origins, directions) float32 (N, 3) of one view's sub-pixels in index order: the eye, and the `direction` layer of
    the layers oracle (always the posed form)."""
    direction = lo.render(params, arrays, pose)["direction"].reshape(-1, 3)
    eye = pose_array(pose)[0]
    return np.ascontiguousarray(np.tile(eye, (len(direction), 1)), np.float32), np.ascontiguousarray(direction, np.float32)


def view(params, arrays, plan, pose, with_ao: bool = True, rays_of=None) -> dict:
    """Every layer of one instanced view, {name: (H, W) or (H, W, 3)} ("ao" only with_ao).  `rays_of(points, normals, seeds)`:
    where the ambient-occlusion rays come from instead of the oracle (RANDOM)."""
    h, w = params.height, params.width
    o, d = camera_rays(params, arrays, pose)
    out = io.closest(arrays, plan, o, d, 1e5)
    hit = out["hit"].astype(bool)
    out["direction"] = d
    out["shade"] = shade(out["normal"], d, hit, bool(params.shading_enable))
    if with_ao:
        seeds = np.flatnonzero(hit).astype(np.uint32)
        points, normals = np.ascontiguousarray(out["position"][hit]), np.ascontiguousarray(out["normal"][hit])
        rays = rays_of(points, normals, seeds) if rays_of is not None and len(seeds) else None
        factor = np.ones(h * w, np.float32)
        factor[hit] = ao(params, arrays, plan, points, normals, seeds, rays)["ao"]
        out["ao"] = factor
        with np.errstate(all="ignore"):
            out["value"] = (out["shade"] * factor).astype(np.float32)
    else:
        out["value"] = out["shade"].copy()
    return {k: v.reshape((h, w) + v.shape[1:]) for k, v in out.items()}


def cameras(rt, plan) -> list:
    """Three poses for a set: from outside the top-level root box towards its centre, from inside it towards the first
    instance's box, and one whose eye is not finite (it sees nothing)."""
    nodes = plan["nodes"]
    lo_, hi_ = np.asarray(nodes["lo"][0], np.float64), np.asarray(nodes["hi"][0], np.float64)
    centre, ext = (lo_ + hi_) / 2, float(np.linalg.norm(hi_ - lo_))
    first = nodes[nodes["leaf"] == 0][0]
    target = (np.asarray(first["lo"], np.float64) + np.asarray(first["hi"], np.float64)) / 2
    outside = rt.Camera.look_at((centre + np.array([0.21, 0.17, 0.45]) * ext).tolist(), centre.tolist())
    eye = centre + np.array([0.031, -0.022, 0.017]) * ext
    assert ((eye > lo_) & (eye < hi_)).all()
    inside = rt.Camera.look_at(eye.tolist(), target.tolist(), (0.1, 1.0, 0.05))
    nowhere = rt.Camera.from_vectors((np.inf, 0.0, np.nan), outside.as_array()[1], outside.as_array()[2], outside.as_array()[3])
    return [outside, inside, nowhere]


IDENTITY_SIZE = (48, 40)
RECORD_CAP, AO_CAP = 0.01, 0.05  # what the -0 filter may leave out: of the sub-pixels; of the hit sub-pixels


def oblique_pose(rt, arrays):
    """The pose of the identity relation's tests: from outside the root box, along no axis and no diagonal."""
    lo_, hi_ = cases.root_box(arrays)
    centre, ext = (lo_ + hi_) / 2, float(np.linalg.norm(hi_ - lo_))
    eye = centre + np.array([0.43, 0.31, 0.68], np.float32) * ext
    return rt.Camera.look_at(eye.tolist(), (centre + np.array([0.013, -0.021, 0.008], np.float32) * ext).tolist(), (0.12, 1.0, 0.07))


def identity_options(rt):
    return rt.Options.defaults(width=IDENTITY_SIZE[0], height=IDENTITY_SIZE[1], n_super_samples=1, ao_num_samples=3)


def identity_case(rt, scene_for, mesh):
    """(params, arrays, plan, pose, plain layers) of one identity instance at IDENTITY_SIZE."""
    _, arrays = scene_for(mesh, "longest")
    opt = identity_options(rt)
    params = orc.params_from_options(opt)
    W = cases.family("identity", arrays)
    plan = rt.instance_plan(*cases.root_box(arrays), W)
    pose = oblique_pose(rt, arrays)
    return params, arrays, plan, pose, lo.render(params, arrays, pose)


def identity_masks(params, arrays, pose, plain):
    """(record mask, ao mask) over the sub-pixels in index order: where the relation speaks of the record layers, and
    where it speaks of `ao` and `value` too."""
    o, d = camera_rays(params, arrays, pose)
    record = identity_filter(o, d)
    hit = plain["hit"].reshape(-1).astype(bool)
    points, normals = plain["position"].reshape(-1, 3)[hit], plain["normal"].reshape(-1, 3)[hit]
    ao_o, ao_d = ao_rays(params, arrays, points, normals, np.flatnonzero(hit).astype(np.uint32))
    clean = identity_filter(ao_o[:, None, :], ao_d).all(axis=1)
    ao = np.zeros(len(hit), bool)
    ao[hit] = clean
    return record, record & ao, hit


def negative_zero(a) -> np.ndarray:
    a = np.asarray(a)
    return np.signbit(a) & (a == 0)


def identity_filter(o, d):
    """The rays of the identity relation: six finite components, no -0 (instance_cases.without_negative_zero's rule), as a mask."""
    return np.isfinite(o).all(axis=-1) & np.isfinite(d).all(axis=-1) & ~negative_zero(o).any(axis=-1) & ~negative_zero(d).any(axis=-1)


def assert_layers(got: dict, want: dict, names, what="") -> None:
    for f in names:
        assert got[f].shape == want[f].shape and got[f].dtype == want[f].dtype, (what, f, got[f].shape, want[f].shape, got[f].dtype)
        ok = same_words(got[f], want[f])
        assert ok.all(), (what, f, int((~ok).sum()), np.argwhere(~ok)[:5].tolist())
