"""GPU: instanced ambient occlusion and instanced views (include/rt_hip_instance_views.h) against their expected values BY
COMPOSITION (tests/instance_views_oracle.py: the ambient-occlusion rays of the directional oracle, the instanced walk of the
instance oracle on the tree read back from the host, the camera rays of the layers oracle, numpy float32 for the rest), every
output word for word; against render_views under one identity instance; against the float64 reference; and what the calls
leave alone."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ao_direction_cases as adc
import build_cases as bc
import instance_cases as cases
import instance_oracle as io
import instance_reference as ir
import instance_views_oracle as ivo
import orc
import refit_cases as rc
from conftest import bits

pytestmark = pytest.mark.gpu

SORT_MIN = 16384  # RT_QUERY_SORT_MIN, in rays
SIZES = (1, 63, 64, 65, 257, 2000)
NONE = 0xFFFFFFFF
EMPTY = np.zeros((0, 3, 4), np.float32)
VIEW_SIZE = dict(width=24, height=20)  # three tiles across, a partial bottom tile


def ao_host(rt, scene, rung="d14", **over):
    r = adc.SMALL[rung]
    opt = rt.Options.defaults(width=32, height=24, n_super_samples=1, ao_num_samples=r.rings, ao_alpha_min=r.amin, ao_alpha_max=r.amax,
                              ao_max_distance=over.pop("ao_max_distance", 0.5), **over)
    host = rt.Host(opt, 0)
    host.upload_scene(scene)
    if not over.get("ao_method"):
        assert host.ao_rays_per_point == (r.dirs, r.dirs)
    return host


def surface_points(host, plan, n, seed):
    """(points, normals) float32 (n, 3) on the posed surfaces: hit points of trace_instances_closest with their normals."""
    o, d = cases.rays(plan["nodes"], 6 * n + 600, seed)
    got = host.trace_instances_closest(o, d, outputs=("hit", "distance", "position", "normal"))
    at = got["hit"].astype(bool) & (got["distance"] < np.inf)
    assert at.any()
    take = np.resize(np.flatnonzero(at), n)
    return np.ascontiguousarray(got["position"][take]), np.ascontiguousarray(got["normal"][take])


def odd_points(points, normals):
    """Every float is legal: NaN and infinite points, zero, huge, tiny and NaN normals, points far outside the set."""
    p, q = points.copy(), normals.copy()
    k = np.arange(len(p))
    p[k % 7 == 1, 0] = np.nan
    p[k % 11 == 2, 2] = np.inf
    q[k % 13 == 3] = 0.0
    q[k % 17 == 4] *= np.float32(1e30)
    q[k % 19 == 5, 1] = np.nan
    p[k % 23 == 6] *= np.float32(1e6)
    p[k % 29 == 7] = np.float32(3e38)
    q[k % 31 == 8] *= np.float32(1e-30)
    q[k % 37 == 9, 2] = np.float32(-0.0)
    q[k % 41 == 10] = -q[k % 41 == 10]
    return p, q


def check_ao(host, arrays, plan, points, normals, seeds=None, sort=True, rays=None, what=""):
    got = host.instances_ambient_occlusion(points, normals, seeds, sort=sort)
    assert tuple(got) == ("ao", "occluded") and got["ao"].dtype == np.float32 and got["occluded"].dtype == np.uint32
    want = ivo.ao(orc.params_from_options(host.options), arrays, plan, points, normals, seeds, rays)
    for f in ("occluded", "ao"):
        ok = ivo.same_words(got[f], want[f])
        print(f"INSTANCE AO {what} sort {sort}: {f} differs at {int((~ok).sum())} of {len(ok)}")
        assert ok.all(), (what, sort, f, int((~ok).sum()), np.argwhere(~ok)[:5].tolist())
    return got


def sets_of(arrays):
    yield "one", cases.many(arrays, 1, seed=3)
    yield "two", cases.many(arrays, 2, seed=3)
    yield "many65", cases.many(arrays, 65, seed=3)
    for family in ("rotations", "shear", "mirror", "tie_pair"):
        yield family, cases.family(family, arrays)


# ---- 1. instanced ambient occlusion against the composition -----------------------------------------------------------
@pytest.mark.parametrize("mesh,bvh", [("single", "longest"), ("single", "sah"), ("ties", "longest"), ("ties", "sah"), ("blob", "longest"),
                                      ("blob", "sah")])
def test_ao_matches_the_composition(rt, scene_for, mesh, bvh):
    scene, arrays = scene_for(mesh, bvh)
    host = ao_host(rt, scene)  # 14 rays a point: a point's run of lanes straddles packets
    occluded = 0
    try:
        for k, (name, W) in enumerate(sets_of(arrays)):
            host.set_instances(W)
            plan = host.instances()
            points, normals = surface_points(host, plan, max(SIZES), seed=31 + k)
            for n in SIZES:
                got = check_ao(host, arrays, plan, points[:n], normals[:n], sort=bool((n + k) % 2), what=(mesh, bvh, name, n))
                assert got["ao"].shape == (n,)
            occluded += int(got["occluded"].sum())
            p, q = odd_points(points[:520], normals[:520])
            check_ao(host, arrays, plan, p, q, sort=bool(k % 2), what=(mesh, bvh, name, "odd points"))
        assert occluded > 0 and host.last_query_ms > 0.0
        empty = host.instances_ambient_occlusion(points[:0], normals[:0])
        assert empty["ao"].shape == (0,) and empty["occluded"].shape == (0,)
    finally:
        host.close()


@pytest.mark.parametrize("rung", ["d4", "d14", "d71", "d79_alpha"])
def test_ao_direction_counts_sort_threshold_and_subsets(rt, scene_for, rung):
    """A count that divides 64, one below 64 that does not, two above it; a point count on each side of RT_QUERY_SORT_MIN rays;
    output subsets."""
    scene, arrays = scene_for("blob", "sah")
    host = ao_host(rt, scene, rung)
    per = adc.SMALL[rung].dirs
    below = (SORT_MIN - 1) // per  # the last point count whose rays stay below the threshold
    try:
        host.set_instances(cases.family("rotations", arrays))
        plan = host.instances()
        points, normals = surface_points(host, plan, min(below + 1, 1500), seed=43)
        for n in sorted({min(below, len(points)), min(below + 1, len(points)), 65}):
            p, q = points[:n], normals[:n]
            want = check_ao(host, arrays, plan, p, q, what=(rung, n))
            for f in ("ao", "occluded"):
                assert ivo.same_words(host.instances_ambient_occlusion(p, q, sort=False)[f], want[f]).all(), (rung, n, f)
            assert want["occluded"].any() and (want["occluded"] <= per).all()
        for subset in (("ao",), ("occluded",)):
            part = host.instances_ambient_occlusion(p, q, outputs=subset)
            assert tuple(part) == subset and ivo.same_words(part[subset[0]], want[subset[0]]).all()
        assert host.instances_ambient_occlusion(p, q, outputs=()) == {}
        if per * 1500 >= SORT_MIN:  # (both sides of the threshold were met with this many rays a point)
            assert below + 1 <= len(points)
    finally:
        host.close()


def test_ao_across_the_sort_threshold_with_few_rays_a_point(rt, scene_for):
    """14 rays a point: 1170 points make 16380 rays, 1171 make 16394 -- one call on each side of RT_QUERY_SORT_MIN."""
    scene, arrays = scene_for("blob", "longest")
    host = ao_host(rt, scene)
    try:
        host.set_instances(cases.many(arrays, 65, seed=5))
        plan = host.instances()
        points, normals = surface_points(host, plan, 1171, seed=47)
        assert 1170 * 14 < SORT_MIN <= 1171 * 14
        for n in (1170, 1171):
            check_ao(host, arrays, plan, points[:n], normals[:n], what=("threshold", n))
            check_ao(host, arrays, plan, points[:n], normals[:n], sort=False, what=("threshold", n))
    finally:
        host.close()


def test_ao_random_method_with_explicit_seeds(rt, scene_for):
    """RANDOM: the sampler depends on the device's libm, so the rays come from host.ao_rays() and are composed the same way."""
    scene, arrays = scene_for("blob", "sah")
    host = ao_host(rt, scene, "d14", ao_method=1)
    try:
        host.set_instances(cases.family("rotations", arrays))
        plan = host.instances()
        points, normals = surface_points(host, plan, 700, seed=53)
        seeds = (np.arange(700, dtype=np.uint32) * np.uint32(2654435761)) ^ np.uint32(0x9E3779B9)
        rays = host.ao_rays(points, normals, seeds)
        got = check_ao(host, arrays, plan, points, normals, seeds, rays=(rays["origins"], rays["directions"]), what="random, seeds")
        assert got["occluded"].any()
        rays = host.ao_rays(points, normals)
        check_ao(host, arrays, plan, points, normals, None, sort=False, rays=(rays["origins"], rays["directions"]), what="random, own index")
        other = host.instances_ambient_occlusion(points, normals, seeds[::-1].copy())
        assert not np.array_equal(other["occluded"], got["occluded"])  # (the seeds are read)
    finally:
        host.close()


# ---- 2. instanced views against the composition -------------------------------------------------------------------------
def view_options(rt, ss, **over):
    return rt.Options.defaults(**VIEW_SIZE, n_super_samples=ss, ao_num_samples=over.pop("ao_num_samples", 3),
                               ao_max_distance=over.pop("ao_max_distance", 0.5), **over)


def five_cameras(rt, plan):
    cams = ivo.cameras(rt, plan)
    nodes = plan["nodes"]
    lo_, hi_ = cases.top_box(nodes)
    centre, ext = (lo_ + hi_) / 2, float(np.linalg.norm(hi_ - lo_))
    more = [rt.Camera.look_at((centre + np.array(v) * ext).tolist(), centre.tolist()) for v in ([-0.5, 0.2, 0.1], [0.1, -0.45, -0.3])]
    return [cams[0], more[0], cams[2], cams[1], more[1]]


def check_views(rt, host, arrays, plan, cams, names=None, what=""):
    """Every layer, the instance ids and the image of every view == the composition's."""
    opt = host.options
    params = orc.params_from_options(opt)
    with_ao = bool(opt.enable_ao) and opt.ao_num_samples > 0
    names = tuple(n for n in rt.INSTANCE_VIEW_OUTPUTS if with_ao or n != "ao") if names is None else names
    got = host.render_instance_views(cams, names)
    assert tuple(got) == names
    h, w = opt.total_height, opt.total_width
    for v, cam in enumerate(cams):
        want = ivo.view(params, arrays, plan, cam, with_ao)
        want["image"] = rt.resize_cpu(opt, want["value"])
        for f in names:
            block = got[f][v]
            assert block.shape == want[f].shape and block.dtype == want[f].dtype, (what, f, v, block.shape, block.dtype)
            ok = ivo.same_words(block, want[f])
            if not ok.all():
                print(f"INSTANCE VIEWS {what} view {v}: {f} differs at {int((~ok).sum())} of {ok.size}")
            assert ok.all(), (what, f, v, int((~ok).sum()), np.argwhere(~ok)[:5].tolist())
    assert got[names[0]].shape[:3] == (len(cams), h, w) or names[0] == "image"
    return got


@pytest.mark.parametrize("ss", [1, 2])
@pytest.mark.parametrize("family", ["rotations", "grid"])
def test_views_match_the_composition(rt, scene_for, family, ss):
    scene, arrays = scene_for("blob", "sah" if ss == 1 else "longest")
    host = rt.Host(view_options(rt, ss), 0)
    try:
        host.upload_scene(scene)
        host.set_instances(cases.family(family, arrays))
        plan = host.instances()
        cams = ivo.cameras(rt, plan)
        got = check_views(rt, host, arrays, plan, cams, what=(family, ss))
        hit = got["hit"].astype(bool)
        assert hit.any() and not hit.all() and not hit[2].any() and hit[0].any() and hit[1].any()
        assert len(np.unique(got["instance"][hit])) > 1 and (got["instance"][~hit] == NONE).all()
        assert (got["ao"][~hit] == 1.0).all() and (bits(got["value"][~hit]) == 0).all() and (got["ao"][hit] < 1.0).any()
        assert got["image"].shape == (3, host.options.height, host.options.width) and got["image"].any()
        assert host.last_views() == {"views": 3, "chunks": 1, "ao_points": int(hit.sum())} and host.last_query_ms > 0.0
    finally:
        host.close()


def test_views_chunks_and_subsets(rt, scene_for):
    scene, arrays = scene_for("blob", "sah")
    host = rt.Host(view_options(rt, 2), 0)
    names = rt.INSTANCE_VIEW_OUTPUTS
    try:
        host.upload_scene(scene)
        host.set_instances(cases.family("rotations", arrays))
        plan = host.instances()
        cams = five_cameras(rt, plan)
        whole = check_views(rt, host, arrays, plan, cams, what="five views, one chunk")
        points = int(whole["hit"].sum())
        assert points and host.last_views() == {"views": 5, "chunks": 1, "ao_points": points}
        host.set_views_chunk(2)  # 2 + 2 + 1
        got = host.render_instance_views(cams, names)
        assert host.last_views() == {"views": 5, "chunks": 3, "ao_points": points}
        ivo.assert_layers(got, whole, names, "three chunks")
        for subset in (("instance",), ("image",), ("hit", "ao"), ("value", "instance", "normal")):
            part = host.render_instance_views(cams, subset)
            assert tuple(part) == subset
            ivo.assert_layers(part, whole, subset, ("three chunks", subset))
        host.set_views_chunk(0)
        for subset in (("instance",), ("image",), ("hit", "ao")):
            ivo.assert_layers(host.render_instance_views(cams, subset), whole, subset, ("one chunk", subset))
        assert tuple(host.render_instance_views(cams)) == ("value",)
        assert host.render_instance_views(cams, ()) == {}
        empty = host.render_instance_views([], names)
        assert empty["instance"].shape == (0, host.options.total_height, host.options.total_width) and empty["image"].shape[0] == 0
        # an array the call was not given stays as it is; a call that asks for nothing launches nothing
        lib = rt.load_library()
        poses = np.stack([cam.as_array() for cam in cams])
        nothing = rt.api._InstanceViewArrays()
        assert lib.rt_render_instance_views(host._h, poses.ctypes.data, 5, C.byref(nothing)) == 0
        assert lib.rt_render_instance_views_device(host._h, poses.ctypes.data, 5, C.byref(nothing), None) == 0
        guard = np.full(whole["instance"].shape, 7, np.uint32)
        only = rt.api._InstanceViewArrays(rt.api._ViewArrays(), guard.ctypes.data)
        assert lib.rt_render_instance_views(host._h, poses.ctypes.data, 5, C.byref(only)) == 0
        assert np.array_equal(guard, whole["instance"])
    finally:
        host.close()


def test_views_without_ambient_occlusion_and_without_shading(rt, scene_for):
    scene, arrays = scene_for("blob", "longest")
    W = cases.family("rotations", arrays)
    off = rt.Host(view_options(rt, 2, ao_num_samples=0, enable_ao=0), 0)
    flat = rt.Host(view_options(rt, 1, enable_shading=0), 0)
    try:
        for host in (off, flat):
            host.upload_scene(scene)
            host.set_instances(W)
        plan = off.instances()
        cams = ivo.cameras(rt, plan)
        with pytest.raises(rt.RtError) as e:
            off.render_instance_views(cams, ("ao",))
        assert e.value.code == rt.api.RT_E_STATE and "ambient occlusion off" in e.value.message
        got = check_views(rt, off, arrays, plan, cams, what="ambient occlusion off")
        assert "ao" not in got and np.array_equal(bits(got["value"]), bits(got["shade"])) and got["hit"].any()
        ivo.assert_layers(off.render_instance_views(cams, ("image",)), got, ("image",), "image alone, from shade")
        assert off.last_views() == {"views": 3, "chunks": 1, "ao_points": 0}
        got = check_views(rt, flat, arrays, flat.instances(), cams, what="shading off")
        hit = got["hit"].astype(bool)
        assert (got["shade"][hit] == 1.0).all() and (got["shade"][~hit] == 0.0).all() and hit.any()
        assert np.array_equal(bits(got["value"][hit]), bits(got["ao"][hit]))
    finally:
        off.close()
        flat.close()


# ---- 3. the identity relation to render_views ---------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["blob", "bunny"])
def test_identity_relation_to_render_views(rt, scene_for, mesh):
    scene, arrays = scene_for(mesh, "longest")
    opt = ivo.identity_options(rt)
    params = orc.params_from_options(opt)
    pose = ivo.oblique_pose(rt, arrays)
    host = rt.Host(opt, 0)
    try:
        host.upload_scene(scene)
        host.set_instances(cases.family("identity", arrays))
        want = {f: a[0] for f, a in host.render_views([pose], rt.VIEW_OUTPUTS).items()}
        got = {f: a[0] for f, a in host.render_instance_views([pose], rt.INSTANCE_VIEW_OUTPUTS).items()}
    finally:
        host.close()
    record, ao, hit = ivo.identity_masks(params, arrays, pose, want)
    left_out, ao_left_out = 1.0 - record.mean(), 1.0 - ao[hit].mean()
    print(f"IDENTITY GPU {mesh}: the -0 filter leaves out {left_out:.4f} of the sub-pixels, {ao_left_out:.4f} of the hit ones for ao")
    assert left_out <= ivo.RECORD_CAP and ao_left_out <= ivo.AO_CAP and hit.sum() > 100 and not hit.all()
    n = len(hit)
    at = record & (want["distance"].reshape(-1) < np.inf)
    for f in ("hit", "distance", "leaf", "barycentric", "position", "normal", "direction", "shade"):
        assert ivo.same_words(got[f].reshape(n, -1)[at], want[f].reshape(n, -1)[at]).all(), (mesh, f)
    assert np.array_equal(got["hit"], want["hit"])
    assert (got["instance"].reshape(-1)[at & hit] == 0).all() and (got["instance"].reshape(-1)[~hit] == NONE).all()
    with_ao = ao & (want["distance"].reshape(-1) < np.inf)
    for f in ("ao", "value"):
        assert ivo.same_words(got[f].reshape(-1)[with_ao], want[f].reshape(-1)[with_ao]).all(), (mesh, f)
    if with_ao[hit].all() and at.all():  # (nothing was left out: the finished images are equal too)
        assert np.array_equal(got["image"], want["image"])
    assert (want["ao"][want["hit"].astype(bool)] < 1.0).any()


# ---- 4. float64 grounding --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["rotations", "shear"])
def test_float64_comparator_on_one_views_rays(rt, scene_for, family):
    scene, arrays = scene_for("blob", "longest")
    opt = rt.Options.defaults(width=48, height=40, n_super_samples=1, ao_num_samples=2)
    W = cases.family(family, arrays)
    host = rt.Host(opt, 0)
    try:
        host.upload_scene(scene)
        host.set_instances(W)
        pose = ivo.cameras(rt, host.instances())[0]
        got = host.render_instance_views([pose], ivo.RECORD + ("direction",))
    finally:
        host.close()
    n = opt.total_width * opt.total_height
    flat = {f: got[f][0].reshape((n,) + got[f].shape[3:]) for f in ivo.RECORD}
    d = np.ascontiguousarray(got["direction"][0].reshape(n, 3))
    o = np.ascontiguousarray(np.tile(pose.as_array()[0], (n, 1)), np.float32)
    rep = ir.compare_closest(scene, ir.instanced(scene, W, o, d, 1e5), flat)
    print(f"INSTANCE VIEWS GPU {family}: {rep}")
    assert not rep.failures(tol=ir.TOL), rep.failures(tol=ir.TOL)
    assert flat["hit"].sum() > 20


# ---- 5. everything else is left alone ---------------------------------------------------------------------------------
def test_frames_and_plain_calls_are_left_alone(rt, scene_for):
    scene, arrays = scene_for("bunny", "longest")
    host = rt.Host(rt.Options.defaults(width=96, height=64, n_super_samples=2, ao_num_samples=3), 0)
    try:
        host.upload_scene(scene)
        host.render()
        before, stats = host.download(), host.stats()
        cams = [ivo.oblique_pose(rt, arrays), rt.Camera.default()]
        plan = rt.instance_plan(*cases.root_box(arrays), cases.family("rotations", arrays))
        o, d = cases.rays(plan["nodes"], 3000, seed=71)
        probe = host.trace_closest(o, d, outputs=("hit", "distance", "position", "normal"))
        at = probe["hit"].astype(bool) & (probe["distance"] < np.inf)
        points, normals = np.ascontiguousarray(probe["position"][at]), np.ascontiguousarray(probe["normal"][at])
        plain = (host.render_views(cams, rt.VIEW_OUTPUTS), host.render_layers(), host.ambient_occlusion(points, normals))
        host.set_instances(cases.family("rotations", arrays))
        plan = host.instances()
        first = host.render_instance_views(cams, rt.INSTANCE_VIEW_OUTPUTS)
        first_ao = host.instances_ambient_occlusion(points, normals)
        assert first["hit"].any() and host.stats() == stats
        assert not np.array_equal(first["hit"], plain[0]["hit"])
        host.render()
        assert np.array_equal(bits(host.download()), bits(before))
        host.render_async()  # a frame left in flight while the new calls run
        during = host.render_instance_views(cams, rt.INSTANCE_VIEW_OUTPUTS)
        during_ao = host.instances_ambient_occlusion(points, normals, sort=False)
        host.sync()
        assert np.array_equal(bits(host.download()), bits(before)) and host.stats() == stats
        ivo.assert_layers(during, first, rt.INSTANCE_VIEW_OUTPUTS, "beside a frame")
        ivo.assert_layers(during_ao, first_ao, ("ao", "occluded"), "beside a frame")
        host.render()
        assert np.array_equal(bits(host.download()), bits(before)) and host.stats() == stats
        # the plain entry points with a set in place: their set-free words
        ivo.assert_layers(host.render_views(cams, rt.VIEW_OUTPUTS), plain[0], rt.VIEW_OUTPUTS, "render_views with a set")
        ivo.assert_layers(host.render_layers(), plain[1], tuple(plain[1]), "render_layers with a set")
        ivo.assert_layers(host.ambient_occlusion(points, normals), plain[2], ("ao", "occluded"), "ambient_occlusion with a set")
        # ... and the new ones are the composition's on this host too
        want = ivo.ao(orc.params_from_options(host.options), arrays, plan, points[:500], normals[:500])
        assert np.array_equal(first_ao["occluded"][:500], want["occluded"])
    finally:
        host.close()


# ---- 6. after an update, a build and a new upload ----------------------------------------------------------------------
def test_after_update_vertices_build_scene_and_a_new_upload(rt):
    scene = rc.fresh_scene(rt, "blob", "longest")
    host = rt.Host(view_options(rt, 1), 0)
    try:
        host.upload_scene(scene)
        arrays = orc.SceneArrays.from_scene(scene)
        W = cases.family("rotations", arrays)
        host.set_instances(W)
        first = host.instances()

        def both(arrays, plan, what):
            cams = ivo.cameras(rt, plan)[:2]
            got = check_views(rt, host, arrays, plan, cams, what=what)
            assert got["hit"].any()
            points, normals = surface_points(host, plan, 300, seed=59)
            assert check_ao(host, arrays, plan, points, normals, what=what)["occluded"].any()

        both(arrays, first, "as uploaded")
        moved = rc.steps("twist", scene.vertices)[-1]
        scene.refit(moved)
        host.update_vertices(moved, scene.vnormals)
        arrays = orc.SceneArrays.from_scene(scene)
        plan = host.instances()
        assert plan["nodes"].tobytes() != first["nodes"].tobytes()
        both(arrays, plan, "updated")
        v, f = bc.mesh("blob")
        built = bc.lbvh_scene(rt, "blob")
        host.build_scene(v, f, built.vnormals)
        arrays = orc.SceneArrays.from_scene(built)
        after = host.instances()
        assert after["nodes"].tobytes() != plan["nodes"].tobytes()
        both(arrays, after, "built")
        host.upload_scene(scene)
        arrays = orc.SceneArrays.from_scene(scene)
        again = host.instances()
        assert again["nodes"].tobytes() == plan["nodes"].tobytes()
        both(arrays, again, "uploaded again")
    finally:
        host.close()


# ---- 7. errors -----------------------------------------------------------------------------------------------------------
class _DeviceBytes:
    def __init__(self, size):
        self.hip, self.ptr = C.CDLL("libamdhip64.so"), C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.ptr), C.c_size_t(size)) == 0
        assert self.hip.hipMemset(self.ptr, 0, C.c_size_t(size)) == 0

    def free(self):
        self.hip.hipFree(self.ptr)


def test_error_paths(rt, scene_for):
    lib = rt.load_library()
    scene, arrays = scene_for("blob", "longest")
    STATE, INVALID = rt.api.RT_E_STATE, rt.api.RT_E_INVALID
    W = cases.family("rotations", arrays)
    opt = rt.Options.defaults(width=32, height=24, n_super_samples=1, ao_num_samples=2)
    cams = [rt.Camera.default(), ivo.oblique_pose(rt, arrays)]
    poses = np.stack([cam.as_array() for cam in cams])
    p = np.zeros((4, 3), np.float32)
    p4 = np.zeros((4, 4), np.float32)
    at = p4.ctypes.data
    nothing = rt.api._InstanceViewArrays()
    host = rt.Host(opt, 0)

    def refused(code, *calls):
        for call in calls:
            with pytest.raises(rt.RtError) as e:
                call()
            assert e.value.code == code
        return e.value.message

    both = (lambda: host.instances_ambient_occlusion(p, p), lambda: host.render_instance_views(cams))
    refused(STATE, *both)  # no upload, no set
    host.set_instances(W)
    assert "before a scene was uploaded" in refused(STATE, *both)  # a set, no upload
    assert lib.rt_render_instance_views_device(host._h, poses.ctypes.data, 2, C.byref(nothing), None) == STATE
    host.upload_scene(scene)
    host.set_instances(EMPTY)
    assert "without an instance set" in refused(STATE, *both)  # an upload, no set
    assert lib.rt_trace_instances_ao(host._h, at, at, None, 4, 0, None, None) == STATE
    assert lib.rt_render_instance_views(host._h, poses.ctypes.data, 2, C.byref(nothing)) == STATE
    host.set_instances(W)
    # null inputs, too many points, null arrays
    assert lib.rt_trace_instances_ao(host._h, None, at, None, 4, 0, None, None) == INVALID
    assert lib.rt_trace_instances_ao(host._h, at, None, None, 4, 0, None, None) == INVALID
    assert lib.rt_trace_instances_ao_device(host._h, None, None, None, 4, 0, None, None, None) == INVALID
    assert lib.rt_trace_instances_ao(host._h, None, None, None, 0, 0, None, None) == 0
    assert lib.rt_trace_instances_ao(host._h, at, at, None, 4, 0, None, None) == 0  # (no outputs: nothing is written)
    rays = host.ao_rays_per_point[0]
    assert lib.rt_trace_instances_ao(host._h, at, at, None, (1 << 27) // rays + 1, 0, None, None) == INVALID
    assert "RT_QUERY_MAX_RAYS" in lib.rt_last_error().decode()
    assert lib.rt_trace_instances_ao(None, at, at, None, 4, 0, None, None) == INVALID
    assert lib.rt_render_instance_views(host._h, poses.ctypes.data, 2, None) == INVALID  # a NULL `out`
    assert lib.rt_render_instance_views_device(host._h, poses.ctypes.data, 2, None, None) == INVALID
    assert lib.rt_render_instance_views(None, poses.ctypes.data, 2, C.byref(nothing)) == INVALID
    assert lib.rt_render_instance_views(host._h, None, 2, C.byref(nothing)) == INVALID  # NULL cameras with views > 0
    assert lib.rt_render_instance_views(host._h, None, 0, C.byref(nothing)) == 0  # views == 0: nothing to do
    assert host.render_instance_views([], ("instance",))["instance"].shape[0] == 0
    # misaligned device pointers are refused before anything is enqueued (the addresses are never used)
    for field in ("distance", "leaf", "barycentric", "position", "normal", "direction", "shade", "ao", "value"):
        arrays_ = rt.api._InstanceViewArrays(rt.api._ViewArrays(rt.api._LayerArrays(**{field: 0x1002}), None), None)
        assert lib.rt_render_instance_views_device(host._h, poses.ctypes.data, 2, C.byref(arrays_), None) == INVALID, field
    arrays_ = rt.api._InstanceViewArrays(rt.api._ViewArrays(), 0x1002)
    assert lib.rt_render_instance_views_device(host._h, poses.ctypes.data, 2, C.byref(arrays_), None) == INVALID
    assert "4-byte aligned" in lib.rt_last_error().decode()
    mem = _DeviceBytes(2 * 65 * 16 + 4096)
    a, b, out = mem.ptr.value, mem.ptr.value + 65 * 16, mem.ptr.value + 2 * 65 * 16
    assert lib.rt_trace_instances_ao_device(host._h, a + 4, b, None, 64, 0, out, None, None) == INVALID
    assert lib.rt_trace_instances_ao_device(host._h, a, b + 8, None, 64, 0, out, None, None) == INVALID
    assert lib.rt_trace_instances_ao_device(host._h, a, b, out + 2, 64, 0, out + 1024, None, None) == INVALID
    assert lib.rt_trace_instances_ao_device(host._h, a, b, None, 64, 0, out + 2, None, None) == INVALID
    assert lib.rt_trace_instances_ao_device(host._h, a, b, None, 64, 0, out, out + 1025, None) == INVALID
    assert lib.rt_trace_instances_ao_device(host._h, a, b, out + 2048, 64, 0, out, out + 1024, None) == 0
    assert host.last_query_ms >= 0.0  # (waits for the query)
    mem.free()
    # Python: unknown output names, float64 inputs, mismatched inputs
    with pytest.raises(ValueError):
        host.render_instance_views(cams, ("instance", "colour"))
    with pytest.raises(ValueError):
        host.instances_ambient_occlusion(p, p, outputs=("ao", "mask"))
    with pytest.raises(ValueError):
        host.instances_ambient_occlusion(p.astype(np.float64), p)
    with pytest.raises(ValueError):
        host.instances_ambient_occlusion(p, p[:3])
    with pytest.raises(ValueError):
        host.render_instance_views(poses.astype(np.float64))
    assert host.render_instance_views(cams, ("instance",))["instance"].shape == (2, 24, 32)
    host.close()
    # ambient occlusion off
    off = rt.Host(rt.Options.defaults(width=32, height=24, n_super_samples=1, ao_num_samples=0, enable_ao=0), 0)
    off.upload_scene(scene)
    off.set_instances(W)
    assert "ambient occlusion off" in refused(STATE, lambda: off.instances_ambient_occlusion(p, p),
                                              lambda: off.render_instance_views(cams, rt.INSTANCE_VIEW_OUTPUTS))
    assert lib.rt_trace_instances_ao_device(off._h, None, None, None, 0, 0, None, None, None) == STATE
    assert off.render_instance_views(cams, ("image",))["image"].shape == (2, 24, 32)
    off.close()
    # a band-partitioned host renders a part of the image only
    part = rt.Host(opt, 0, 1, 2)
    part.upload_scene(scene)
    part.set_instances(W)
    assert "band-partitioned" in refused(STATE, lambda: part.render_instance_views(cams, ("hit",)))
    part.close()
    # the hosts of a ring
    ring = rt.FrameRing(opt, scene, device=0, hosts=2)
    assert "frame ring" in refused(STATE, lambda: ring.host(0).render_instance_views(cams, ("hit",)),
                                   lambda: ring.host(0).instances_ambient_occlusion(p, p))
    ring.close()


# ---- 8. the device form ----------------------------------------------------------------------------------------------
def test_torch_path_equals_numpy_path():
    """Device tensors in and out on a non-default stream == the numpy path (tests/instance_views_torch_driver.py, a fresh child
    process that brings torch's runtime up before it loads the library)."""
    driver = os.path.join(os.path.dirname(os.path.abspath(__file__)), "instance_views_torch_driver.py")
    r = subprocess.run([sys.executable, driver], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "INSTANCE_VIEWS_TORCH_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
