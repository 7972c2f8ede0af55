"""Geometric ground truth for directional occlusion, the frame layers and multi-view rendering, on top of
tests/geometry_reference.py: every ray against every triangle in file order, in numpy float64, no tree.  TEST
INFRASTRUCTURE ONLY.

tests/directional_oracle.c and tests/layers_oracle.c walk the kernels' tree in the kernels' arithmetic: they say that kernel
and oracle agree.  This module says whether a mask BIT sits at the right ray, whether `bent` was summed over the right rays,
and whether a layer's value belongs to the sub-pixel it is stored at -- wherever that does not hang on a rounding.  UNIFORM
ambient occlusion only: the RANDOM method's rays depend on the device's libm.

directional(): the rays are geometry_reference.ao_rays' (float32 origins and directions, the tangent frame rounded ONCE from
float64), every ray classified by geometry_reference._pairs.  A ray is judged when one of its pairs is clearly accepted or
none is borderline (the any-hit rule of geometry_reference.ao, kept per ray); a point when all its rays are.  The kernels
round the frame per operation, so their directions are not this module's words: a few per cent of the components differ by
an ulp.  Directions and `bent` therefore get tolerances; mask bits and counts stay exact on judged rays, where the margin
geometry_reference.M absorbs that ulp.

layers(): the sub-pixels' rays are geometry_reference.camera_rays' (the library's WORDS), the record is the closest hit of
geometry_reference.multihit, the shade clamp(-n . d).  The ambient-occlusion factor is composed in compare_layers, as
tests/test_geometry_gpu.py composes a frame: the reference's count at the ANSWER's own hit point and normal.
"""
import numpy as np

import geometry_reference as gr

PRIMARY_MAX_DISTANCE = 100000.0  # the frame's own rays (include/rt_hip_layers.h)
UNPOSED = np.array([[0, 0, 2], [1, 0, 0], [0, 1, 0], [0, 0, -1]], np.float32)  # a host without a pose, as eye / right / up / forward

# ---- tolerances ---------------------------------------------------------------------------------------------------------
# Worst difference between the CPU ORACLE (tests/directional_oracle.c, float32, bit-equal to the GPU) and this reference
# over all the directional cases of tests/test_shading_reference_cpu.py (blob / 16, both trees, the four settings, and the
# device-built blob) -- printed by that file's tests, rounded up to two digits here.  As in geometry_reference each tolerance
# is 8 x the measured value: the GPU's differences are the oracle's, the factor only absorbs another sample.
#   ao_direction  |delta| per component of a ray's direction (the frame rounded once here, per operation there)
#   bent          |delta| per component / R: the sum grows with the rays per point
# Measured: ao_direction on blob / 16, 3 rings; bent on blob / 16, 5 rings (R = 71).
MEASURED = {"ao_direction": 1.8e-7, "bent": 1.6e-7}
TOL = {**gr.TOL, **{f: 8.0 * v for f, v in MEASURED.items()}}
TOL["value"] = gr.TOL["shade"]  # shade x ao with ao <= 1 an exact word on both sides: the shade's difference, no more


class Report(gr.Report):
    """geometry_reference.Report against this module's tolerances."""

    def failures(self, tol=None, max_unjudged=0.01) -> list:
        return super().failures(TOL if tol is None else tol, max_unjudged)


class Surface:
    """What the reference and the comparators read of a scene -- vertices, faces, vnormals, face_of_leaf -- for a mesh no
    Scene stands for as it is: vertices a host was updated to, a tree a host built."""

    def __init__(self, vertices, faces, vnormals, face_of_leaf):
        self.vertices = np.array(vertices, np.float32)
        self.faces = np.array(faces, np.uint32).reshape(-1, 3)
        self.vnormals = np.array(vnormals, np.float32)
        self.face_of_leaf = face_of_leaf
        self.num_faces = len(self.faces)


def _words(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def popcount(mask) -> np.ndarray:
    return np.unpackbits(np.ascontiguousarray(mask, np.uint32).view(np.uint8), axis=1).sum(axis=1, dtype=np.uint32)


def unpack(mask, bits: int) -> np.ndarray:
    """bool (N, bits): bit k & 31 of word k >> 5, for every k below `bits` (which may exceed the rays per point)."""
    mask = np.ascontiguousarray(mask, np.uint32)
    k = np.arange(bits)
    return ((mask[:, k >> 5] >> (k & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)


def pack(flags) -> np.ndarray:
    """uint32 (N, ceil(R / 32)) of bool (N, R): unpack's inverse."""
    n, r = flags.shape
    words = (r + 31) // 32
    padded = np.zeros((n, words * 32), np.uint64)
    padded[:, :r] = flags
    weights = np.uint64(1) << np.arange(32, dtype=np.uint64)
    return (padded.reshape(n, words, 32) * weights).sum(axis=2).astype(np.uint32)


# ---- directional occlusion ----------------------------------------------------------------------------------------------
def directional(scene, options, table, points, normals) -> dict:
    """{"hit", "judged": bool (N, R), "bent": float64 (N, 3) -- the sum of the reference's own directions over the rays with
    hit False --, "rays": R, "occluded": uint32 (N,), "point_judged": bool (N,), "origins": float32 (N, 3), "directions":
    float32 (N, R, 3)}."""
    assert options.ao_method == 0
    m = gr.mesh_of(scene)
    o32, d32 = gr.ao_rays(table, points, normals)
    npts, k = d32.shape[0], d32.shape[1]
    o = np.repeat(o32.astype(np.float64), k, axis=0)
    d = d32.reshape(-1, 3).astype(np.float64)
    max_distance = gr.kernel_float(options.ao_max_distance)
    hit, judged = np.zeros(npts * k, bool), np.zeros(npts * k, bool)
    scope = gr.in_scope(o, d)

    def work(span):
        i0, i1 = span
        acc, bord, _, _, _ = gr._pairs(m, o[i0:i1], d[i0:i1], max_distance)
        hit[i0:i1] = acc.any(axis=1)
        judged[i0:i1] = (hit[i0:i1] | ~bord.any(axis=1)) & scope[i0:i1]

    gr._map(work, gr._chunks(npts * k, len(m.faces)))
    hit, judged = hit.reshape(npts, k), judged.reshape(npts, k)
    bent = (d32.astype(np.float64) * ~hit[:, :, None]).sum(axis=1)
    return {"hit": hit, "judged": judged, "bent": bent, "rays": k, "occluded": hit.sum(axis=1).astype(np.uint32),
            "point_judged": judged.all(axis=1), "origins": o32, "directions": d32}


def first_points(ref: dict, n: int) -> dict:
    """directional()'s answer for the first n points alone."""
    return {f: (v[:n] if isinstance(v, np.ndarray) else v) for f, v in ref.items()}


def compare_directional(ref: dict, got: dict) -> Report:
    """{"mask", "occluded", "ao", "bent"} of the library's form, or any of them, against directional()'s.
    mismatches: "mask" -- bit k of a row differs from hit[:, k], on judged RAYS; "mask_tail" -- rows with a bit from R
    upwards set; "occluded" -- differs from the row's popcount (every point) or from the reference's count (judged points);
    "ao" -- not the word 1 - occluded / R in float32 (every point).  worst: "bent", |delta| per component / R on judged
    points.  Also "judged_rays_share", and "judged_share" of the points."""
    R, pj = ref["rays"], ref["point_judged"]
    mism, worst = {}, {}
    count = None
    if "mask" in got:
        mask = np.asarray(got["mask"], np.uint32)
        words = (R + 31) // 32
        assert mask.shape == (len(pj), words), (mask.shape, words)
        flags = unpack(mask, 32 * words)
        mism["mask"] = int(((flags[:, :R] != ref["hit"]) & ref["judged"]).sum())
        mism["mask_tail"] = int(flags[:, R:].any(axis=1).sum())
        count = popcount(mask)
    if "occluded" in got:
        occ = np.asarray(got["occluded"], np.uint32)
        mism["occluded"] = int(((occ != ref["occluded"]) & pj).sum()) + (0 if count is None else int((occ != count).sum()))
        count = occ
    if "ao" in got:
        # (the answer's own count, on every point; an `ao` that came alone: the reference's count, on judged points)
        of, where = (ref["occluded"], pj) if count is None else (count, np.ones(len(pj), bool))
        own = np.float32(1.0) - of.astype(np.float32) / np.float32(R)
        mism["ao"] = int(((_words(got["ao"]) != _words(own)) & where).sum())
    if "bent" in got:
        with np.errstate(invalid="ignore"):
            delta = np.abs(np.asarray(got["bent"], np.float64).reshape(-1, 3) - ref["bent"]).max(axis=1) / R
        worst["bent"] = float(np.nan_to_num(delta[pj], nan=np.inf).max()) if pj.any() else 0.0
    return Report(rays=ref["hit"].size, judged_share=float(pj.mean()), hit_share=float((ref["occluded"] > 0).mean()),
                  judged_rays_share=float(ref["judged"].mean()), mismatches=mism, worst=worst)


def compare_rays(ref_o, ref_d, got: dict) -> Report:
    """{"origins": (N, 3 or 4), "directions": (N, R, 3 or 4)} -- Host.ao_rays, or the oracle's -- against
    geometry_reference.ao_rays': the origins as words (a fourth component must be 0), the directions within tolerance."""
    o, d = np.asarray(got["origins"], np.float32), np.asarray(got["directions"], np.float32)
    assert o.shape[0] == ref_o.shape[0] and d.shape[:2] == ref_d.shape[:2], (o.shape, d.shape, ref_d.shape)
    mism = {"origin": int((_words(o[:, :3]) != _words(ref_o)).any(axis=1).sum()),
            "w": int((o[:, 3:] != 0).sum() + (d[:, :, 3:] != 0).sum())}
    delta = np.abs(d[:, :, :3].astype(np.float64) - ref_d.astype(np.float64))
    worst = {"ao_direction": float(np.nan_to_num(delta, nan=np.inf).max()) if delta.size else 0.0}
    return Report(rays=d.shape[0] * d.shape[1], judged_share=1.0, hit_share=0.0, mismatches=mism, worst=worst,
                  differing_share=float((_words(d[:, :, :3]) != _words(ref_d)).mean()) if delta.size else 0.0)


# ---- frame layers -------------------------------------------------------------------------------------------------------
def layers(scene, options, table, camera) -> dict:
    """The layers of one frame but `ao`, per sub-pixel of total_width x total_height, flat in row order: {"direction":
    float32 (N, 3), "origins", "multi": geometry_reference.multihit's answer, "hit", "judged": bool (N,), "shade": float64
    (N,) = clamp(-n . d), 1 with shading off, 0 without a hit, "shape": (H, W), "grid": the root of the supersample count,
    "options", "table": for compare_layers' ambient-occlusion step}.  camera None: a host without a pose.  (Its direction
    is normalize((cx, cy, -1)); through the pose's formula a cx or cy of -0 would come out as +0.  The frames here have even
    sizes: no such sub-pixel.)"""
    o, d = gr.camera_rays(options, UNPOSED if camera is None else camera)
    n = int(np.sqrt(float(options.n_super_samples)))
    multi = gr.multihit(scene, o, d, PRIMARY_MAX_DISTANCE)
    hit = multi["count"] > 0
    shade = np.ones(len(o))
    if options.enable_shading:
        shade = np.clip(-(multi["normal"][:, 0] * d.astype(np.float64)).sum(axis=1), 0.0, 1.0)
    shade = np.where(hit, shade, 0.0)
    return {"direction": d, "origins": o, "multi": multi, "hit": hit, "judged": multi["judged"], "shade": shade,
            "shape": (options.height * n, options.width * n), "grid": n, "options": options, "table": table}


def flat(got: dict) -> dict:
    """A layers answer of the library's form, (H, W[, 3]) per layer, per sub-pixel in row order."""
    return {f: (np.asarray(v).reshape(-1, 3) if np.asarray(v).ndim == 3 else np.asarray(v).reshape(-1)) for f, v in got.items()}


def ao_of_layers(scene, ref: dict, got: dict) -> dict:
    """geometry_reference.ao at the ANSWER's own position and normal of its hit sub-pixels, and "at": their indices."""
    g = flat(got)
    at = np.flatnonzero(g["hit"].astype(bool))
    out = dict(gr.ao(scene, ref["options"], ref["table"], np.ascontiguousarray(g["position"][at]), np.ascontiguousarray(g["normal"][at])))
    out["at"] = at
    return out


def compare_layers(scene, ref: dict, got: dict, ao_ref=None) -> Report:
    """Every layer of the library's form ((H, W) or (H, W, 3) arrays, `ao` absent on a host without ambient occlusion)
    against layers()'s.
    mismatches: "direction" (words), geometry_reference.compare_closest's ("hit", "leaf", "fill", "unused_slot": the record
    through face_of_leaf, the no-hit values included), "ao" -- not the word float32(1 - occluded / R) with the reference's
    count at the answer's own hit point, where pixel and point are judged --, "ao_miss" -- not 1.0 without a hit --,
    "value" -- not the word float32(shade) * float32(ao) of the answer's own layers, on every sub-pixel.
    worst: compare_closest's, "shade", and "value" against the reference's shade x the reference's factor, on judged
    sub-pixels.  Also "ao_judged_share", "ao_occluded_share", and -- for the 8-bit image -- "ref_value" and "sure"."""
    g = flat(got)
    n = len(ref["hit"])
    for f in g.values():
        assert f.shape[0] == n, (f.shape, n)
    j = ref["judged"]
    rep = gr.compare_closest(scene, ref["multi"], g)
    mism, worst = dict(rep["mismatches"]), dict(rep["worst"])
    mism["direction"] = int((_words(g["direction"]) != _words(ref["direction"])).any(axis=1).sum())
    hit = g["hit"].astype(bool)
    shade = g["shade"].astype(np.float32)
    worst["shade"] = gr._worst(np.abs(shade.astype(np.float64) - ref["shade"])[j])
    ref_value, sure = ref["shade"].copy(), j.copy()
    extra = {}
    if "ao" in g:
        ao_ref = ao_ref if ao_ref is not None else ao_of_layers(scene, ref, got)
        at = ao_ref["at"]
        assert np.array_equal(at, np.flatnonzero(hit)), "ao_ref was made for another answer"
        ao = g["ao"].astype(np.float32)
        sure[at] &= ao_ref["judged"]
        mism["ao"] = int(((_words(ao[at]) != _words(ao_ref["ao"])) & sure[at]).sum())
        mism["ao_miss"] = int((ao[~hit] != 1.0).sum())
        own = shade * ao
        ref_value[at] *= ao_ref["ao"].astype(np.float64)
        extra = {"ao_judged_share": float(ao_ref["judged"].mean()) if len(at) else 1.0,
                 "ao_occluded_share": float((ao_ref["occluded"] > 0).mean()) if len(at) else 0.0, "ao_points": len(at)}
    else:
        own = shade
    mism["value"] = int((_words(g["value"]) != _words(own)).sum())
    worst["value"] = gr._worst(np.abs(g["value"].astype(np.float64) - ref_value)[sure])
    return Report(rays=n, judged_share=float(j.mean()), hit_share=float(ref["hit"].mean()), mismatches=mism, worst=worst,
                  ref_value=ref_value.reshape(ref["shape"]), sure=sure.reshape(ref["shape"]), **extra)


def compare_image(ref_value, sure, image, grid: int) -> Report:
    """The 8-bit image of a view against floor(mean(reference value) x 255) per output pixel, on the pixels all of whose
    grid x grid sub-pixels are judged: at most ONE level apart -- what a difference far below 1 / 255 can move a truncating
    store by."""
    image = np.asarray(image)
    h, w = image.shape
    blocks = lambda a: a.reshape(h, grid, w, grid).transpose(0, 2, 1, 3).reshape(h, w, grid * grid)
    want = np.floor(blocks(ref_value).mean(axis=2) * 255.0)
    ok = blocks(sure).all(axis=2)
    bad = (np.abs(image.astype(np.float64) - want) > 1.0) & ok
    return Report(rays=h * w, judged_share=float(ok.mean()), hit_share=float((want > 0).mean()), mismatches={"image": int(bad.sum())}, worst={})
