"""CPU: the oracles of the ray, multi-hit and ambient-occlusion queries and of the posed camera against the BVH-free float64
reference of tests/geometry_reference.py -- and the inputs, caps and floors that tests/test_geometry_gpu.py shares.

The oracles walk the tree in float32 as the kernels do; the reference tests every ray against every triangle in float64
and declines to judge a ray whose answer hangs on a rounding.  What is asserted: on judged rays the counts, hit flags and
faces are equal and the float fields lie within geometry_reference.TOL; at most 1 % of the rays or pixels (2 % of the AO
points) go unjudged; the floors below keep every case from passing vacuously; doctored answers are reported.
Every test prints its judged share and its worst difference per field (pytest -s): geometry_reference.MEASURED is the
largest of them."""
import numpy as np
import pytest

import ao_oracle as aoo
import camera_oracle as co
import geometry_reference as gr
import multihit_oracle as mo
import orc
import query_oracle as qo
from test_camera_gpu import nave_pose, poses_for

BVHS = ("longest", "sah")
GENERIC_MESHES = ("blob", "ties", "layered")
MAX_DISTANCES = (1e5, 5.0, 0.3, 0.02)
N_RANDOM, N_AXIS = 6000, 1200
KS = (2, 5, 9, 15, 16)
AO_SETTINGS = ((3, 0.2), (2, 0.05), (5, 1.0))  # (ao_num_samples, ao_max_distance), UNIFORM
N_AO_POINTS = 2000
FRAME_W, FRAME_H = 48, 32
FRAME_CASES = (("blob", "orbit_135"), ("blob", "roll"), ("blob", "skewed"), ("blob", "above"), ("interior", "nave"))

MAX_UNJUDGED = 0.01      # of the rays of a (mesh, max_distance), and of the pixels of the posed frames together
MAX_UNJUDGED_AO = 0.02   # of the AO points of a case
MIN_HIT_SHARE = 0.05     # of a mesh's generic rays, at the largest max_distance
MIN_OCCLUDED_SHARE = 0.20  # of the AO points of the case: the three settings together (the short reach of (2, 0.05) alone
MIN_OCCLUDED_SHARE_EACH = 0.05  # occludes fewer, as max_distance 0.02 alone hits fewer than MIN_HIT_SHARE); and of each

_SCENES, _RAYS, _REF = {}, {}, {}


def scene_of(rt, scene_for, mesh, bvh):
    """(product Scene with BVH, SceneArrays): the golden meshes, the layered stack, the blob at 1 / 16 of its size."""
    key = (mesh, bvh)
    if key not in _SCENES:
        if mesh == "layered":
            _SCENES[key] = mo.layered_scene(rt, bvh)
        elif mesh == "blob16":  # a power of two: exact.  Unit-sized, so that the reference's fixed 1e-5 AO offset is many ulps
            base, _ = scene_for("blob", bvh)
            sc = rt.Scene.from_arrays(base.vertices[:, :3] / np.float32(16.0), base.faces.reshape(-1, 3)).build_bvh(0 if bvh == "longest" else 1)
            _SCENES[key] = (sc, orc.SceneArrays.from_scene(sc))
        else:
            _SCENES[key] = scene_for(mesh, bvh)
    return _SCENES[key]


def generic_rays(mesh, arrays):
    """6000 rays from inside the root box, a third of the directions x 37, a third x 0.01 (directions are not normalised);
    for the layered stack also rays along +-z: exact zero components, lists longer than RT_MULTIHIT_MAX_K."""
    if mesh not in _RAYS:
        o, d = mo.random_rays(arrays, N_RANDOM, seed=101 + GENERIC_MESHES.index(mesh), grow=0.0)
        d[0::3] *= np.float32(37.0)
        d[1::3] *= np.float32(0.01)
        if mesh == "layered":
            ao_, ad = mo.axis_rays(N_AXIS, seed=7)
            o, d = np.concatenate([ao_, o]), np.concatenate([ad, d])
        for a in (o, d):
            a.setflags(write=False)
        _RAYS[mesh] = (o, d)
    return _RAYS[mesh]


def frozen(res):
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res


def generic_reference(mesh, scene, o, d, max_distance):
    """The reference's multi-hit answer, once per (mesh, max_distance): it knows no tree."""
    key = (mesh, float(max_distance))
    if key not in _REF:
        _REF[key] = frozen(gr.multihit(scene, o, d, max_distance))
    return _REF[key]


def ao_points(closest_fn, arrays):
    """2000 points with normals: the closest hits of random rays around the mesh, through `closest_fn(o, d)`."""
    o, d = mo.random_rays(arrays, 12000, seed=23)
    res = closest_fn(o, d)
    hit = np.flatnonzero(np.asarray(res["hit"]).astype(bool) & np.isfinite(res["distance"]))[:N_AO_POINTS]
    assert len(hit) == N_AO_POINTS
    return np.ascontiguousarray(res["position"][hit]), np.ascontiguousarray(res["normal"][hit])


def ao_options(rt, samples, reach):
    return rt.Options.defaults(width=64, height=48, n_super_samples=1, ao_num_samples=samples, ao_max_distance=reach)


def ao_reference(scene, opt, table, points, normals):
    key = ("ao", opt.ao_num_samples, float(opt.ao_max_distance))
    if key not in _REF:
        _REF[key] = frozen(gr.ao(scene, opt, table, points, normals))
    return _REF[key]


def frame_options(rt, shading, ao=0):
    return rt.Options.defaults(width=FRAME_W, height=FRAME_H, n_super_samples=1, ao_num_samples=ao, enable_shading=int(shading))


def frame_pose(rt, mesh, pose, arrays):
    return nave_pose(rt, arrays) if pose == "nave" else poses_for(rt, arrays)[pose]


def frame_reference(rt, mesh, pose, scene, shading, cam):
    key = ("frame", mesh, pose)
    if key not in _REF:  # (the rays and their hits do not depend on the shading switch)
        _REF[key] = gr.posed_frame(scene, frame_options(rt, 1), cam)
    return _REF[key] if shading else gr.without_shading(_REF[key])


def passes(report, what, max_unjudged=MAX_UNJUDGED):
    print(f"GEOMETRY {what}: {report}")
    bad = report.failures(max_unjudged=max_unjudged)
    assert not bad, (what, bad)


# ---- what the reduction of "max_distance only culls boxes" to the triangle's own box rests on ------------------------------
@pytest.mark.parametrize("bvh", BVHS)
@pytest.mark.parametrize("mesh", GENERIC_MESHES + ("blob16", "interior"))
def test_leaf_boxes_are_triangle_bounds_and_parents_contain_children(rt, scene_for, mesh, bvh):
    scene, _ = scene_of(rt, scene_for, mesh, bvh)
    nodes = np.asarray(scene.nodes)
    boxes = np.asarray(scene.aabbs).reshape(-1, 2, 4)[:, :, :3]
    lo, hi = boxes[:, 0], boxes[:, 1]
    at = np.arange(len(nodes))
    inner = at[nodes > 1]
    left = inner + 1
    right = left + nodes[left]
    assert (right < inner + nodes[inner]).all() and (right + nodes[right] == inner + nodes[inner]).all()
    for child in (left, right):
        assert (lo[child] >= lo[inner]).all() and (hi[child] <= hi[inner]).all()
    leaves = at[nodes == 1]  # pre-order: the L-th of them is leaf L
    assert len(leaves) == scene.num_faces
    tri = np.asarray(scene.vertices)[:, :3][np.asarray(scene.faces).reshape(-1, 3)[scene.face_of_leaf()]]  # (leaf, corner, xyz)
    assert np.array_equal(lo[leaves], tri.min(axis=1))  # (as values: a bound of -0 may stand as +0, which no comparison sees)
    assert np.array_equal(hi[leaves], tri.max(axis=1))
    # face_of_leaf names the file's face the tree's leaf holds, and every face once
    assert np.array_equal(np.asarray(scene.sorted_faces).reshape(-1, 3), np.asarray(scene.faces).reshape(-1, 3)[scene.face_of_leaf()])
    assert np.array_equal(np.sort(scene.face_of_leaf()), np.arange(scene.num_faces))


# ---- case 1: generic rays ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_distance", MAX_DISTANCES)
@pytest.mark.parametrize("bvh", BVHS)
@pytest.mark.parametrize("mesh", GENERIC_MESHES)
def test_oracles_against_the_reference(rt, scene_for, mesh, bvh, max_distance):
    scene, arrays = scene_of(rt, scene_for, mesh, bvh)
    o, d = generic_rays(mesh, arrays)
    ref = generic_reference(mesh, scene, o, d, max_distance)
    what = f"{mesh}/{bvh} max_distance {max_distance:g}"
    full = mo.multihit(arrays, o, d, max_distance, mo.MAX_K)
    passes(gr.compare_multihit(scene, ref, full, mo.MAX_K), what + " multihit k=16")
    passes(gr.compare_multihit(scene, ref, mo.first_slots(full, 5), 5), what + " multihit k=5")
    passes(gr.compare_closest(scene, ref, qo.closest(arrays, o, d, max_distance)), what + " closest")
    passes(gr.compare_flags(ref, qo.occluded(arrays, o, d, max_distance), "occluded"), what + " occluded")
    if max_distance == MAX_DISTANCES[0]:
        assert (ref["count"] > 0).mean() >= MIN_HIT_SHARE
        if mesh == "layered":
            assert (ref["count"][:N_AXIS] > mo.MAX_K).sum() >= N_AXIS // 4


# ---- case 2: ambient occlusion at caller-supplied points ------------------------------------------------------------------
@pytest.mark.parametrize("bvh", BVHS)
@pytest.mark.parametrize("samples,reach", AO_SETTINGS)
def test_ao_oracle_against_the_reference(rt, oracle, scene_for, samples, reach, bvh):
    scene, arrays = scene_of(rt, scene_for, "blob16", bvh)
    _, first = scene_of(rt, scene_for, "blob16", BVHS[0])
    points, normals = ao_points(lambda o, d: qo.closest(first, o, d, 100000.0), first)
    opt = ao_options(rt, samples, reach)
    p = orc.params_from_options(opt)
    ref = ao_reference(scene, opt, oracle.ao_table(p), points, normals)
    got = aoo.ambient_occlusion(p, arrays, points, normals)
    assert got["rays"] == ref["rays"]
    passes(gr.compare_ao(ref, got), f"blob/16 {bvh} ao {samples} rings reach {reach:g}", MAX_UNJUDGED_AO)
    assert (ref["occluded"] > 0).mean() >= MIN_OCCLUDED_SHARE_EACH
    if (samples, reach) == AO_SETTINGS[-1]:  # (the last setting: the others' references are in the cache by now, or made here)
        refs = [ao_reference(scene, ao_options(rt, s, r), oracle.ao_table(orc.params_from_options(ao_options(rt, s, r))), points, normals)
                for s, r in AO_SETTINGS]
        assert np.mean([(r["occluded"] > 0).mean() for r in refs]) >= MIN_OCCLUDED_SHARE


# ---- case 3: posed frames -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shading", [0, 1], ids=["mask", "shade"])
@pytest.mark.parametrize("mesh,pose", FRAME_CASES)
def test_camera_oracle_against_the_reference(rt, scene_for, mesh, pose, shading):
    scene, arrays = scene_of(rt, scene_for, mesh, "longest")
    opt = frame_options(rt, shading)
    cam = frame_pose(rt, mesh, pose, arrays)
    ref = frame_reference(rt, mesh, pose, scene, shading, cam)
    image, counters = co.render(orc.params_from_options(opt), arrays, cam)
    passes(gr.compare_frame(ref, image), f"{mesh} {pose} {'shade' if shading else 'mask'}", max_unjudged=1.0)  # (the cap: below)
    assert ref["hit"].mean() >= MIN_HIT_SHARE
    if pose == "skewed":  # the doctored pose: up negated
        flipped = gr.posed_frame(scene, opt, cam.as_array() * np.array([[1], [1], [-1], [1]], np.float32))
        assert gr.compare_frame(flipped, image).failures()


def frames_unjudged_share(rt, scene_for):
    """The share of unjudged pixels over the frames of FRAME_CASES together."""
    judged = []
    for mesh, pose in FRAME_CASES:
        scene, arrays = scene_of(rt, scene_for, mesh, "longest")
        judged.append(frame_reference(rt, mesh, pose, scene, 1, frame_pose(rt, mesh, pose, arrays))["judged"])
        print(f"GEOMETRY {mesh} {pose}: {judged[-1].mean():.4%} of the pixels judged")
    return 1.0 - float(np.mean(judged))


def test_posed_frames_leave_few_pixels_unjudged(rt, scene_for):
    """The cap on unjudged pixels holds for the posed frames of the case together, not for each: from `above`, 33 of the
    1536 pixels (2.15 %) go unjudged.  The eye stands over the origin, a focal length times max(W, H) scales both image
    axes, and so the pixels with x - 23.5 = y - 15.5 look along the plane x = z -- which holds the shared diagonal of the
    ground quad's two triangles.  Those rays meet both triangles at s = 0 or t = 0 exactly: inside the contract's own
    tolerance of 1e-5, and nothing a float64 reference can call for either side.  The other four frames leave out at most
    one pixel each (0.07 %)."""
    assert frames_unjudged_share(rt, scene_for) <= MAX_UNJUDGED


# ---- doctored answers: the comparator reports each ---------------------------------------------------------------------------
def test_doctored_answers_are_reported(rt, scene_for):
    mesh, bvh, md, k = "blob", "longest", 0.3, mo.MAX_K
    scene, arrays = scene_of(rt, scene_for, mesh, bvh)
    o, d = generic_rays(mesh, arrays)
    ref = generic_reference(mesh, scene, o, d, md)
    good = mo.multihit(arrays, o, d, md, k)
    assert not gr.compare_multihit(scene, ref, good, k).failures()

    # 1. the tempting reading of max_distance: hits whose DISTANCE exceeds it removed
    cut = {f: v.copy() for f, v in good.items()}
    keep = good["distance"] <= md
    assert (good["count"] <= k).all()
    cut["count"] = keep.sum(axis=1).astype(np.uint32)
    order = np.argsort(~keep, axis=1, kind="stable")  # kept slots first, in their order
    for f in mo.SLOT_FIELDS:
        fill = {"distance": np.inf, "leaf": mo.NONE}.get(f, 0)
        kept = keep if cut[f].ndim == 2 else keep[:, :, None]
        idx = order if cut[f].ndim == 2 else order[:, :, None]
        cut[f] = np.take_along_axis(np.where(kept, good[f], np.asarray(fill, good[f].dtype)), idx, axis=1)
    assert (cut["count"] != good["count"]).sum() >= 10  # the scene does hold triangles beyond max_distance in nearer boxes
    assert mo.fill_values_hold(cut).all() and mo.in_contract_order(cut).all()  # well-formed, and wrong
    rep = gr.compare_multihit(scene, ref, cut, k)
    print("GEOMETRY doctored, distance cut:", rep)
    assert rep["mismatches"]["count"] >= 10 and rep.failures()

    # 2. slots 0 and 1 swapped on rays with two or more hits (all the triangles along the ray: more of those)
    md = MAX_DISTANCES[0]
    ref = generic_reference(mesh, scene, o, d, md)
    good = mo.multihit(arrays, o, d, md, k)
    assert not gr.compare_multihit(scene, ref, good, k).failures()
    swapped = {f: v.copy() for f, v in good.items()}
    two = good["count"] >= 2
    assert two.sum() >= 100
    for f in mo.SLOT_FIELDS:
        swapped[f][two, 0], swapped[f][two, 1] = good[f][two, 1], good[f][two, 0]
    rep = gr.compare_multihit(scene, ref, swapped, k)
    print("GEOMETRY doctored, slots swapped:", rep)
    assert rep["mismatches"]["leaf"] >= 100 and rep["mismatches"]["order"] >= 100 and rep.failures()

    # 3. the leaf of slot 0 replaced by its neighbour in sorted_faces
    shifted = {f: v.copy() for f, v in good.items()}
    some = good["count"] >= 1
    shifted["leaf"][some, 0] = (good["leaf"][some, 0] + 1) % scene.num_faces
    rep = gr.compare_multihit(scene, ref, shifted, k)
    print("GEOMETRY doctored, neighbouring leaf:", rep)
    assert rep["mismatches"]["leaf"] >= 100 and rep.failures()
    near = qo.closest(arrays, o, d, md)
    assert not gr.compare_closest(scene, ref, near).failures()
    near["leaf"] = np.where(near["hit"].astype(bool), (near["leaf"] + 1) % scene.num_faces, near["leaf"]).astype(np.uint32)
    assert gr.compare_closest(scene, ref, near).failures()
