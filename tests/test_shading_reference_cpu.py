"""CPU: the oracles of directional occlusion (tests/directional_oracle.c) and of the frame layers (tests/layers_oracle.c), and
the query oracles over a refit and an LBVH tree, against the BVH-free float64 reference of tests/shading_reference.py -- and
the inputs, caps and floors that tests/test_shading_reference_gpu.py shares.

What is asserted: on judged rays every mask bit is the reference's, on judged points the count, `ao` is the count's word and
`bent` lies within shading_reference.TOL; on judged sub-pixels every layer is the reference's (words for `direction`, `ao`
and the product `value`, tolerances for the float fields of the record and for `shade`), and the 8-bit image lies within one
level; the floors below keep every case from passing vacuously; doctored answers are reported.  Every test prints its judged
shares, mismatch counts and worst differences (pytest -s): shading_reference.MEASURED holds the largest `bent` and
`ao_direction` printed here."""
import hashlib

import numpy as np
import pytest

import build_cases as bc
import directional_oracle as dro
import geometry_reference as gr
import layers_oracle as lo
import multihit_oracle as mo
import orc
import query_oracle as qo
import refit_cases as rc
import shading_reference as sr
import test_geometry_cpu as cases

# (ao_num_samples, ao_max_distance, ao_alpha_max): cases.AO_SETTINGS -- R = 28: two points share a packet of 64 and a point
# straddles packets; R = 14; R = 71: three mask words, a point longer than a packet -- and 2 rings between 4 and 44 degrees:
# R = 32, a row that ends with its word (found by a search over the table lengths of 1 .. 12 rings and whole degrees)
SETTINGS = tuple((s, r, 90) for s, r in cases.AO_SETTINGS) + ((2, 0.1, 44),)
RAYS = {(3, 0.2, 90): 28, (2, 0.05, 90): 14, (5, 1.0, 90): 71, (2, 0.1, 44): 32}
MAX_UNJUDGED_RAYS = 0.001      # of the rays of a directional case
MIN_MIXED_FIRST_WORD = 0.05    # of the judged points: a set AND a clear bit in the first word -- a bit in the wrong place shows
MIN_HIGH_WORD_POINTS = 50      # judged points with a set bit in word 1 or 2, at R = 71
LAYER_POSES = ("orbit_135", "roll", "skewed", "above", None)  # None: a host without a pose
VIEW_NAMES = ("orbit_135 / 16", "away", "close")
MAX_DISTANCES = (1e5, 0.3)  # of the checks on an updated and on a built scene
K = 5

_REF, _AO = {}, {}


def setting_id(setting) -> str:
    return f"a{setting[0]}_d{setting[1]:g}_max{setting[2]}"


def directional_options(rt, setting):
    samples, reach, alpha_max = setting
    return rt.Options.defaults(width=64, height=48, n_super_samples=1, ao_num_samples=samples, ao_max_distance=reach, ao_alpha_max=alpha_max)


def directional_reference(oracle, key, scene, opt, points, normals):
    """The reference's answer once per key: it knows no tree.  (The oracle's closest hits and the kernels' are the same
    words, so the points of a key are the same in both files: asserted.)"""
    if key not in _REF:
        _REF[key] = (cases.frozen(sr.directional(scene, opt, oracle.ao_table(orc.params_from_options(opt)), points, normals)), points, normals)
    ref, p, n = _REF[key]
    assert np.array_equal(p, points) and np.array_equal(n, normals), "the reference of this key was made for other points"
    return ref


def directional_passes(rep, what):
    print(f"SHADING {what}: {rep}; rays judged {rep['judged_rays_share']:.4%}")
    bad = rep.failures(max_unjudged=cases.MAX_UNJUDGED_AO)
    assert not bad, (what, bad)
    assert rep["judged_rays_share"] >= 1.0 - MAX_UNJUDGED_RAYS, what


def directional_floors(ref, what):
    """The conditions on the reference alone."""
    pj, hit = ref["point_judged"], ref["hit"]
    first = hit[:, :32]
    mixed = (first.any(axis=1) & ~first.all(axis=1))[pj].mean()
    print(f"SHADING {what}: {pj.mean():.4%} of the points judged, {(ref['occluded'] > 0).mean():.2%} with a blocked ray, "
          f"{mixed:.2%} of the judged ones with a set and a clear bit in the first word")
    assert pj.mean() >= 1.0 - cases.MAX_UNJUDGED_AO and ref["judged"].mean() >= 1.0 - MAX_UNJUDGED_RAYS
    assert (ref["occluded"] > 0).mean() >= cases.MIN_OCCLUDED_SHARE_EACH
    assert mixed >= MIN_MIXED_FIRST_WORD
    if ref["rays"] == 71:
        high = int((hit[:, 32:].any(axis=1) & pj).sum())
        print(f"SHADING {what}: {high} judged points with a set bit in word 1 or 2")
        assert high >= MIN_HIGH_WORD_POINTS


def blob16_points(rt, scene_for):
    """The points of tests/test_geometry_cpu.py's AO case."""
    _, first = cases.scene_of(rt, scene_for, "blob16", cases.BVHS[0])
    return cases.ao_points(lambda o, d: qo.closest(first, o, d, 100000.0), first)


# ---- 1. directional occlusion ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bvh", cases.BVHS)
@pytest.mark.parametrize("setting", SETTINGS, ids=setting_id)
def test_directional_oracle_against_the_reference(rt, oracle, scene_for, setting, bvh):
    scene, arrays = cases.scene_of(rt, scene_for, "blob16", bvh)
    points, normals = blob16_points(rt, scene_for)
    opt = directional_options(rt, setting)
    ref = directional_reference(oracle, ("directional", setting), scene, opt, points, normals)
    got = dro.directional(orc.params_from_options(opt), arrays, points, normals)
    assert got["rays"] == ref["rays"] == RAYS[setting]
    what = f"blob/16 {bvh} {setting_id(setting)} R = {ref['rays']}"
    directional_passes(sr.compare_directional(ref, got), what)
    rays = sr.compare_rays(ref["origins"], ref["directions"], got)
    print(f"SHADING {what} rays: {rays}; {rays['differing_share']:.2%} of the direction components differ as words")
    assert not rays.failures(), (what, rays.failures())
    directional_floors(ref, what)
    few = sr.compare_directional(sr.first_points(ref, 3), dro.directional(orc.params_from_options(opt), arrays, points[:3], normals[:3]))
    assert not few.failures(max_unjudged=1.0), few.failures(max_unjudged=1.0)


# ---- 2. frame layers --------------------------------------------------------------------------------------------------
def layer_options(rt, ao: int, supersamples: int = 1):
    opt = cases.frame_options(rt, 1, ao=ao)
    opt.n_super_samples = supersamples
    opt.enable_ao = int(ao != 0)
    return opt


def layer_names(opt) -> tuple:
    return tuple(n for n in lo.NAMES if n != "ao" or opt.enable_ao)


def layer_reference(oracle, key, scene, opt, cam):
    if key not in _REF:
        _REF[key] = sr.layers(scene, opt, oracle.ao_table(orc.params_from_options(opt)) if opt.enable_ao else None, cam)
    return _REF[key]


def layers_pass(what, scene, ref, got):
    """compare_layers, with the reference's ambient-occlusion counts at the answer's hit points made once per answer (the
    oracle's and the kernels' are the same words).  The cap on unjudged sub-pixels is the caller's: over its frames together."""
    ao_ref = None
    if "ao" in got:
        g = sr.flat(got)
        hit = g["hit"].astype(bool)
        digest = hashlib.sha1(g["position"][hit].tobytes() + g["normal"][hit].tobytes() + np.flatnonzero(hit).tobytes()).hexdigest()
        key = (id(ref), digest)
        if key not in _AO:
            _AO[key] = sr.ao_of_layers(scene, ref, got)
        ao_ref = _AO[key]
    rep = sr.compare_layers(scene, ref, got, ao_ref)
    print(f"SHADING {what}: {rep}" + (f"; {rep['ao_points']} AO points, {rep['ao_judged_share']:.4%} judged, {rep['ao_occluded_share']:.2%} occluded"
                                     if "ao" in got else ""))
    bad = rep.failures(max_unjudged=1.0)
    assert not bad, (what, bad)
    return rep


def ao_floors(rep, what):
    assert rep["ao_judged_share"] >= 1.0 - cases.MAX_UNJUDGED_AO, what
    assert rep["ao_occluded_share"] >= cases.MIN_OCCLUDED_SHARE_EACH, what


def plain_pose(rt, scene_for, pose):
    _, arrays = cases.scene_of(rt, scene_for, "blob", "longest")
    return None if pose is None else cases.frame_pose(rt, "blob", pose, arrays)


def plain_reference(rt, oracle, scene_for, pose):
    scene, _ = cases.scene_of(rt, scene_for, "blob", "longest")
    return layer_reference(oracle, ("layers", "blob", pose), scene, layer_options(rt, 0), plain_pose(rt, scene_for, pose))


@pytest.mark.parametrize("pose", LAYER_POSES, ids=lambda p: p or "unposed")
def test_layers_oracle_without_ao(rt, oracle, scene_for, pose):
    scene, arrays = cases.scene_of(rt, scene_for, "blob", "longest")
    opt = layer_options(rt, 0)
    ref = plain_reference(rt, oracle, scene_for, pose)
    all_layers = lo.render(orc.params_from_options(opt), arrays, plain_pose(rt, scene_for, pose))
    layers_pass(f"blob {pose or 'unposed'} layers", scene, ref, {n: all_layers[n] for n in layer_names(opt)})
    assert ref["hit"].mean() >= cases.MIN_HIT_SHARE


def plain_unjudged_share(rt, oracle, scene_for) -> float:
    judged = [plain_reference(rt, oracle, scene_for, pose)["judged"] for pose in LAYER_POSES]
    for pose, j in zip(LAYER_POSES, judged):
        print(f"SHADING blob {pose or 'unposed'}: {j.mean():.4%} of the sub-pixels judged")
    return 1.0 - float(np.mean(judged))


def test_plain_layers_leave_few_sub_pixels_unjudged(rt, oracle, scene_for):
    """Over the five frames together, as tests/test_geometry_cpu.py caps its posed frames and for its reason: `above` alone
    leaves 2.15 % out -- its pixels with x - 23.5 = y - 15.5 look along the plane that holds the shared diagonal of the
    ground quad's two triangles, and meet both at s = 0 or t = 0 exactly."""
    assert plain_unjudged_share(rt, oracle, scene_for) <= cases.MAX_UNJUDGED


def orbit16(rt):
    a = np.radians(135)
    return rt.Camera.look_at((2 * np.sin(a) / 16, 0.3 / 16, 2 * np.cos(a) / 16), (0, 0, 0))  # orbit_135, at the scale of blob / 16


AO_LAYER_SUPERSAMPLES = (1, 4)


def ao_layer_reference(rt, oracle, scene_for, supersamples):
    scene, _ = cases.scene_of(rt, scene_for, "blob16", "longest")
    return layer_reference(oracle, ("layers", "blob16", "orbit", supersamples), scene, layer_options(rt, 3, supersamples), orbit16(rt))


def ao_layers_check(rt, oracle, scene_for, render):
    """Both supersample counts through `render(opt, camera)`, the caps over the two frames together."""
    scene, _ = cases.scene_of(rt, scene_for, "blob16", "longest")
    judged = []
    for ss in AO_LAYER_SUPERSAMPLES:
        ref = ao_layer_reference(rt, oracle, scene_for, ss)
        rep = layers_pass(f"blob/16 orbit_135 3 rings s{ss} layers", scene, ref, render(layer_options(rt, 3, ss), orbit16(rt)))
        ao_floors(rep, ss)
        assert ref["hit"].mean() >= cases.MIN_HIT_SHARE
        judged.append(ref["judged"].mean() * ss)
    assert 1.0 - sum(judged) / sum(AO_LAYER_SUPERSAMPLES) <= cases.MAX_UNJUDGED


def test_layers_oracle_with_ao(rt, oracle, scene_for):
    _, arrays = cases.scene_of(rt, scene_for, "blob16", "longest")
    ao_layers_check(rt, oracle, scene_for, lambda opt, cam: lo.render(orc.params_from_options(opt), arrays, cam))


# ---- 3. views ---------------------------------------------------------------------------------------------------------
def view_options(rt):
    return layer_options(rt, 3, 4)  # 96 x 64 sub-pixels a view: six blocks of the hit list's scan


def view_poses(rt) -> list:
    """orbit_135 at the scale of blob / 16; the same eye looking AWAY from the mesh -- no hit: a block of the compacted list
    with nothing in it --; an eye close above the slab, off its axes -- every sub-pixel hits."""
    orbit = orbit16(rt)
    eye = orbit.as_array()[0].astype(np.float64)
    return [orbit, rt.Camera.look_at(tuple(eye), tuple(2.0 * eye)), rt.Camera.look_at((0.03, 0.12, 0.02), (0, 0, 0), up=(0, 0, -1))]


def views_check(rt, oracle, scene_for, views: dict, images):
    """views[name]: (V, H, W[, 3]) in the order of view_poses; images: (V, h, w) uint8.  Every view against its own
    reference, the caps over the three views together."""
    scene, _ = cases.scene_of(rt, scene_for, "blob16", "longest")
    opt = view_options(rt)
    judged = []
    for v, cam in enumerate(view_poses(rt)):
        ref = layer_reference(oracle, ("view", v), scene, opt, cam)
        what = f"blob/16 view {v} ({VIEW_NAMES[v]})"
        rep = layers_pass(what, scene, ref, {n: a[v] for n, a in views.items()})
        image = sr.compare_image(rep["ref_value"], rep["sure"], images[v], ref["grid"])
        print(f"SHADING {what} image: {image}")
        assert not image.failures(max_unjudged=1.0), (what, image.failures(max_unjudged=1.0))
        if VIEW_NAMES[v] == "away":
            assert not ref["hit"].any() and not views["hit"][v].any() and rep["ao_points"] == 0 and not images[v].any()
        else:
            ao_floors(rep, what)
            assert ref["hit"].mean() >= cases.MIN_HIT_SHARE and image["judged_share"] >= 0.9
        if VIEW_NAMES[v] == "close":
            assert views["hit"][v].all()
        judged.append(ref["judged"].mean())
    assert 1.0 - float(np.mean(judged)) <= cases.MAX_UNJUDGED


def oracle_views(rt, scene_for):
    """The layers oracle, view by view (it has no list of hit sub-pixels at all), and RayTracer::resize of its `value`."""
    if "oracle_views" not in _REF:
        _, arrays = cases.scene_of(rt, scene_for, "blob16", "longest")
        opt = view_options(rt)
        each = [lo.render(orc.params_from_options(opt), arrays, cam) for cam in view_poses(rt)]
        _REF["oracle_views"] = ({n: np.stack([e[n] for e in each]) for n in lo.NAMES}, np.stack([rt.resize_cpu(opt, e["value"]) for e in each]))
    return _REF["oracle_views"]


def test_views_oracle_against_the_reference(rt, oracle, scene_for):
    views, images = oracle_views(rt, scene_for)
    views_check(rt, oracle, scene_for, views, images)


# ---- 4. a scene whose tree was re-boxed, a scene whose tree was built anew ---------------------------------------------
def ray_checks(what, surface, o, d, ref_of, closest, occluded, count, multihit):
    """Closest hit, occlusion, counts and the first K hits through the four callables, against the reference's answers
    ref_of(max_distance) for `surface`."""
    for md in MAX_DISTANCES:
        ref = ref_of(md)
        tag = f"{what} max_distance {md:g}"
        cases.passes(gr.compare_closest(surface, ref, closest(o, d, md)), tag + " closest")
        cases.passes(gr.compare_flags(ref, occluded(o, d, md), "occluded"), tag + " occluded")
        cases.passes(gr.compare_counts(ref, count(o, d, md)), tag + " count")
        cases.passes(gr.compare_multihit(surface, ref, multihit(o, d, md), K), tag + f" multihit k={K}")
    assert (ref_of(MAX_DISTANCES[0])["count"] > 0).mean() >= cases.MIN_HIT_SHARE
    assert (ref_of(MAX_DISTANCES[0])["count"] >= 2).sum() >= 100  # (slot 1 holds something too: tests/test_geometry_cpu.py's count)


def oracle_ray_checks(what, surface, arrays, o, d, ref_of):
    ray_checks(what, surface, o, d, ref_of, lambda o, d, md: qo.closest(arrays, o, d, md), lambda o, d, md: qo.occluded(arrays, o, d, md),
               lambda o, d, md: mo.multihit(arrays, o, d, md, 1)["count"], lambda o, d, md: mo.multihit(arrays, o, d, md, K))


def blob_rays(rt, scene_for):
    return cases.generic_rays("blob", cases.scene_of(rt, scene_for, "blob", "longest")[1])


def surface_reference(key, surface, o, d):
    def ref_of(md):
        if (key, md) not in _REF:
            _REF[key, md] = cases.frozen(gr.multihit(surface, o, d, md))
        return _REF[key, md]

    return ref_of


def twisted_blob(rt, host=None):
    """(the scene after Scene.refit to the twisted vertices, the vertices): the tree's shape is the undeformed blob's.  A
    `host` uploads the scene as the file has it and is updated to the twisted vertices, as tests/test_refit_gpu.py does it."""
    scene = rc.fresh_scene(rt, "blob", "longest")
    if host is not None:
        host.upload_scene(scene)
    step = rc.steps("twist", scene.vertices)[-1]
    scene.refit(step)
    if host is not None:
        host.update_vertices(step, scene.vnormals)
    return scene, step


def updated_surface(scene, step, undeformed):
    """What the reference reads after an update: made of the vertices and normals HANDED to the host, never of a mesh cached
    before the vertices moved."""
    if "updated" not in _REF:
        _REF["updated"] = sr.Surface(step, scene.faces, scene.vnormals, None)
    surface = _REF["updated"]
    surface.face_of_leaf = scene.face_of_leaf  # (this run's tree; the file-order arrays are every run's)
    assert np.array_equal(surface.vertices, np.asarray(step, np.float32))
    moved = np.abs(gr.mesh_of(surface).A - gr.Mesh(undeformed).A).max(axis=1)
    assert (moved > 1e-3).mean() > 0.5, "the reference's mesh is not the deformed one"
    return surface


def test_refit_scene_oracles_against_the_reference(rt, scene_for):
    scene, step = twisted_blob(rt)
    surface = updated_surface(scene, step, cases.scene_of(rt, scene_for, "blob", "longest")[0])
    o, d = blob_rays(rt, scene_for)
    oracle_ray_checks("blob twisted, refit", surface, orc.SceneArrays.from_scene(scene), o, d, surface_reference("updated", surface, o, d))


BUILT_SETTING = SETTINGS[0]


def built_mesh(rt, scale16: bool):
    """(vertices, faces, the LBVH scene of them): the blob, or the blob at 1 / 16 of its size (a power of two: exact)."""
    key = ("built mesh", scale16)
    if key not in _REF:
        v, f = bc.mesh("blob")
        if scale16:
            v = v.copy()
            v[:, :3] /= np.float32(16.0)
        _REF[key] = (v, f, rt.Scene.from_arrays(v, f).build_lbvh())
    return _REF[key]


def built_surface(rt, scale16: bool, face_of_leaf):
    v, f, scene = built_mesh(rt, scale16)
    key = ("built", scale16)
    if key not in _REF:
        _REF[key] = sr.Surface(v, f, scene.vnormals, None)
    _REF[key].face_of_leaf = face_of_leaf
    return _REF[key]


def built_directional(rt, oracle, closest, directional, what):
    """One directional call on a scene built from the blob at 1 / 16 of its size, the points its own closest hits.  (On the
    blob as the file has it the reference judges 13 % of these points: the origins' fixed offset of 1e-5 along the normal is
    a few ulps of such coordinates, too little for geometry_reference.M_A to tell the side of the plane a ray starts on.
    tests/test_geometry_cpu.py's `blob16` is there for that reason.)"""
    _, _, scene = built_mesh(rt, True)
    points, normals = cases.ao_points(closest, orc.SceneArrays.from_scene(scene))  # (the arrays: for the box the rays start in)
    opt = directional_options(rt, BUILT_SETTING)
    ref = directional_reference(oracle, ("directional", "built"), built_surface(rt, True, None), opt, points, normals)
    directional_passes(sr.compare_directional(ref, directional(points, normals)), what)
    directional_floors(ref, what)


def test_lbvh_scene_oracles_against_the_reference(rt, oracle, scene_for):
    _, _, scene = built_mesh(rt, False)
    arrays = orc.SceneArrays.from_scene(scene)
    surface = built_surface(rt, False, scene.face_of_leaf)
    o, d = blob_rays(rt, scene_for)
    oracle_ray_checks("blob, LBVH", surface, arrays, o, d, surface_reference("built", surface, o, d))
    arrays16 = orc.SceneArrays.from_scene(built_mesh(rt, True)[2])
    p = orc.params_from_options(directional_options(rt, BUILT_SETTING))
    built_directional(rt, oracle, lambda o, d: qo.closest(arrays16, o, d, 100000.0),
                      lambda points, normals: dro.directional(p, arrays16, points, normals), f"blob/16, LBVH {setting_id(BUILT_SETTING)}")


# ---- 5. doctored answers: every comparator reports each ----------------------------------------------------------------------
def select(ref: dict, rows) -> dict:
    return {f: (v[rows] if isinstance(v, np.ndarray) else v) for f, v in ref.items()}


def test_doctored_directional_answers_are_reported(rt, oracle, scene_for):
    setting = SETTINGS[0]
    scene, arrays = cases.scene_of(rt, scene_for, "blob16", "longest")
    points, normals = blob16_points(rt, scene_for)
    opt = directional_options(rt, setting)
    ref = directional_reference(oracle, ("directional", setting), scene, opt, points, normals)
    good = dro.directional(orc.params_from_options(opt), arrays, points, normals)
    R = ref["rays"]
    assert not sr.compare_directional(ref, good).failures(max_unjudged=cases.MAX_UNJUDGED_AO)
    answer = lambda **change: {**{f: good[f] for f in ("mask", "occluded", "ao", "bent")}, **change}
    made_of = lambda mask: dict(mask=mask, occluded=sr.popcount(mask), ao=(np.float32(1.0) - sr.popcount(mask).astype(np.float32) / np.float32(R)))
    pj = ref["point_judged"]

    # 1. one set bit cleared in 50 judged points
    some = np.flatnonzero(pj & (ref["occluded"] > 0))[:50]
    assert len(some) == 50
    mask = good["mask"].copy()
    mask[some, 0] &= mask[some, 0] - np.uint32(1)  # (R = 28: one word; its lowest set bit)
    rep = sr.compare_directional(ref, answer(mask=mask))
    print("SHADING doctored, a bit cleared:", rep)
    assert rep["mismatches"]["mask"] >= 50 and rep["mismatches"]["occluded"] >= 50 and rep.failures()

    # 2. every bit one place up: on the points where no bit falls off the end the popcount stands, the places do not
    flags = sr.unpack(good["mask"], R)
    shifted = np.zeros_like(flags)
    shifted[:, 1:] = flags[:, :-1]
    kept = ~flags[:, -1]
    doctored = answer(**made_of(sr.pack(shifted)))
    rep = sr.compare_directional(select(ref, kept), select(doctored, kept))
    print("SHADING doctored, bits shifted:", rep)
    assert rep["mismatches"]["mask"] >= 100 and rep["mismatches"]["occluded"] == 0 and rep["mismatches"]["ao"] == 0 and rep.failures()
    assert sr.compare_directional(ref, doctored)["mismatches"]["mask_tail"] == 0

    # 3. a sorted call's rows left in slot order
    order = np.lexsort((points[:, 2], points[:, 1], points[:, 0]))
    rep = sr.compare_directional(ref, {f: v[order] for f, v in answer().items()})
    print("SHADING doctored, rows in slot order:", rep)
    assert rep["mismatches"]["mask"] >= 1000 and rep["mismatches"]["occluded"] >= 100 and "bent" in " ".join(rep.failures())

    # 4., 5. the sum over the blocked rays, and over all rays
    for name, rays in (("the blocked rays", flags), ("all rays", np.ones_like(flags))):
        rep = sr.compare_directional(ref, answer(bent=dro.ordered_sum(good["directions"], rays)))
        print(f"SHADING doctored, bent over {name}:", rep)
        assert not any(rep["mismatches"].values()) and rep["worst"]["bent"] > 100 * sr.TOL["bent"] and rep.failures()

    # a bit above R, and a direction table one entry out of step
    high = good["mask"].copy()
    high[7, 0] |= np.uint32(1) << np.uint32(R)
    assert sr.compare_directional(ref, answer(mask=high))["mismatches"]["mask_tail"] == 1
    assert not sr.compare_rays(ref["origins"], ref["directions"], good).failures()
    assert sr.compare_rays(ref["origins"], ref["directions"], {"origins": good["origins"], "directions": np.roll(good["directions"], 1, axis=1)}).failures()
    assert sr.compare_rays(ref["origins"], ref["directions"], {"origins": points, "directions": good["directions"]})["mismatches"]["origin"] >= 1000


def test_doctored_layers_are_reported(rt, oracle, scene_for):
    scene, arrays = cases.scene_of(rt, scene_for, "blob16", "longest")
    opt, cam = layer_options(rt, 3, 1), orbit16(rt)
    ref = ao_layer_reference(rt, oracle, scene_for, 1)
    good = lo.render(orc.params_from_options(opt), arrays, cam)
    ao_ref = sr.ao_of_layers(scene, ref, good)
    assert not sr.compare_layers(scene, ref, good, ao_ref).failures(max_unjudged=1.0)
    hit = good["hit"].astype(bool)

    # the factor one place on among the hit sub-pixels -- a wrong rank in the compacted list --, the product made of it
    rolled = {f: v.copy() for f, v in good.items()}
    rolled["ao"][hit] = np.roll(good["ao"][hit], 1)
    rolled["value"] = rolled["shade"] * rolled["ao"]
    rep = sr.compare_layers(scene, ref, rolled, ao_ref)
    print("SHADING doctored, ao one place on:", rep)
    assert rep["mismatches"]["ao"] >= 100 and rep["mismatches"]["value"] == 0 and rep.failures()

    # the head-light term without its clamp (the frame holds back-facing hits)
    n, d = good["normal"], good["direction"]
    raw = np.where(hit, -((n[..., 0] * d[..., 0] + n[..., 1] * d[..., 1]) + n[..., 2] * d[..., 2]), np.float32(0)).astype(np.float32)
    assert (raw < -0.01).sum() >= 100
    unclamped = dict(good, shade=raw, value=raw * good["ao"])
    rep = sr.compare_layers(scene, ref, unclamped, ao_ref)
    print("SHADING doctored, shade without the clamp:", rep)
    assert rep["worst"]["shade"] > 0.01 and rep["mismatches"]["value"] == 0 and "shade" in " ".join(rep.failures())

    # the rays of the pose with `up` negated
    flipped = gr.camera_rays(opt, cam.as_array() * np.array([[1], [1], [-1], [1]], np.float32))[1].reshape(good["direction"].shape)
    rep = sr.compare_layers(scene, ref, dict(good, direction=flipped), ao_ref)
    print("SHADING doctored, up negated:", rep)
    assert rep["mismatches"]["direction"] >= 1000 and rep.failures()

    # a product that is not its own layers'
    assert sr.compare_layers(scene, ref, dict(good, value=good["shade"]), ao_ref)["mismatches"]["value"] >= 100


def test_doctored_views_are_reported(rt, oracle, scene_for):
    scene, _ = cases.scene_of(rt, scene_for, "blob16", "longest")
    views, images = oracle_views(rt, scene_for)
    opt, cams = view_options(rt), view_poses(rt)
    refs = [layer_reference(oracle, ("view", v), scene, opt, cams[v]) for v in (0, 1)]
    # views 0 and 1 swapped
    for v in (0, 1):
        rep = sr.compare_layers(scene, refs[v], {n: a[1 - v] for n, a in views.items()})
        print(f"SHADING doctored, view {1 - v} in the place of view {v}:", rep)
        assert rep["mismatches"]["hit"] >= 1000 and rep["mismatches"]["direction"] >= 1000 and rep.failures()
    # the image two levels up
    rep = layers_pass("view 0", scene, refs[0], {n: a[0] for n, a in views.items()})
    assert not sr.compare_image(rep["ref_value"], rep["sure"], images[0], 2).failures(max_unjudged=1.0)
    up = np.where(images[0] <= 253, images[0] + 2, images[0]).astype(np.uint8)
    image = sr.compare_image(rep["ref_value"], rep["sure"], up, 2)
    print("SHADING doctored, image two levels up:", image)
    assert image["mismatches"]["image"] >= 1000 and image.failures(max_unjudged=1.0)
