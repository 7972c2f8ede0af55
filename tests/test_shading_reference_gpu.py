"""GPU: directional occlusion, the rays it casts, the frame layers, multi-view rendering, and the ray queries on an updated
and on a device-built scene against the BVH-free float64 reference of tests/shading_reference.py, directly: no CPU oracle
stands between the kernels and the geometry.

The inputs, caps, floors and tolerances are those of tests/test_shading_reference_cpu.py (the oracles against the same
reference), imported.  UNIFORM ambient occlusion only."""
import numpy as np
import pytest

import layers_oracle as lo
import shading_reference as sr
import test_geometry_cpu as cases
import test_shading_reference_cpu as shading

pytestmark = pytest.mark.gpu

SORT_MIN = 16384  # RT_QUERY_SORT_MIN (include/rt_hip_query.h): calls with fewer rays are never sorted


def uploaded(rt, scene, opt, cam=None):
    host = rt.Host(opt, 0)
    if cam is not None:
        host.set_camera(cam)
    host.upload_scene(scene)
    return host


def blob16_points(rt, scene_for):
    """The points of the CPU file's cases, through the first tree's own closest hits on the GPU."""
    scene, arrays = cases.scene_of(rt, scene_for, "blob16", cases.BVHS[0])
    host = uploaded(rt, scene, shading.directional_options(rt, shading.SETTINGS[0]))
    try:
        return cases.ao_points(lambda o, d: host.trace_closest(o, d, 100000.0), arrays)
    finally:
        host.close()


# ---- 1. directional occlusion ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bvh", cases.BVHS)
@pytest.mark.parametrize("setting", shading.SETTINGS, ids=shading.setting_id)
def test_directional_occlusion(rt, oracle, scene_for, setting, bvh):
    scene, _ = cases.scene_of(rt, scene_for, "blob16", bvh)
    points, normals = blob16_points(rt, scene_for)
    opt = shading.directional_options(rt, setting)
    ref = shading.directional_reference(oracle, ("directional", setting), scene, opt, points, normals)  # (the table: an input)
    R = ref["rays"]
    what = f"blob/16 {bvh} {shading.setting_id(setting)} R = {R}"
    host = uploaded(rt, scene, opt)
    try:
        assert host.ao_rays_per_point == (R, R) and R == shading.RAYS[setting] and host.ao_mask_words == (R + 31) // 32
        assert len(points) * R >= SORT_MIN  # the sort really runs
        for sort in (True, False):
            got = host.directional_occlusion(points, normals, sort=sort)
            assert set(got) == {"mask", "occluded", "ao", "bent"}
            shading.directional_passes(sr.compare_directional(ref, got), what + (" sorted" if sort else " unsorted"))
        # three points: a partial last packet
        few = sr.compare_directional(sr.first_points(ref, 3), host.directional_occlusion(points[:3], normals[:3]))
        print(f"SHADING {what} three points: {few}")
        assert not few.failures(max_unjudged=1.0), few.failures(max_unjudged=1.0)
        # the branches of the finishing kernel: the mask alone, the sum alone
        for name in ("mask", "bent"):
            alone = host.directional_occlusion(points, normals, outputs=(name,))
            assert set(alone) == {name}
            shading.directional_passes(sr.compare_directional(ref, alone), what + f" {name} alone")
        rays = sr.compare_rays(ref["origins"], ref["directions"], host.ao_rays(points, normals))
        print(f"SHADING {what} rays: {rays}; {rays['differing_share']:.2%} of the direction components differ as words")
        assert not rays.failures(), (what, rays.failures())
    finally:
        host.close()
    shading.directional_floors(ref, what)


# ---- 2. frame layers --------------------------------------------------------------------------------------------------
def rendered_layers(rt, scene, opt, cam):
    host = uploaded(rt, scene, opt, cam)
    try:
        return host.render_layers(shading.layer_names(opt))
    finally:
        host.close()


@pytest.mark.parametrize("pose", shading.LAYER_POSES, ids=lambda p: p or "unposed")
def test_layers_without_ao(rt, oracle, scene_for, pose):
    scene, _ = cases.scene_of(rt, scene_for, "blob", "longest")
    ref = shading.plain_reference(rt, oracle, scene_for, pose)
    got = rendered_layers(rt, scene, shading.layer_options(rt, 0), shading.plain_pose(rt, scene_for, pose))
    assert "ao" not in got
    shading.layers_pass(f"blob {pose or 'unposed'} layers", scene, ref, got)
    assert ref["hit"].mean() >= cases.MIN_HIT_SHARE


def test_plain_layers_leave_few_sub_pixels_unjudged(rt, oracle, scene_for):
    """The cap of the CPU file's test of this name, for the references this file used."""
    assert shading.plain_unjudged_share(rt, oracle, scene_for) <= cases.MAX_UNJUDGED


def test_layers_with_ao(rt, oracle, scene_for):
    scene, _ = cases.scene_of(rt, scene_for, "blob16", "longest")
    shading.ao_layers_check(rt, oracle, scene_for, lambda opt, cam: rendered_layers(rt, scene, opt, cam))


# ---- 3. views ---------------------------------------------------------------------------------------------------------
def test_views(rt, oracle, scene_for):
    """Three views in one call -- one of them sees nothing, one hits everywhere --: the hit list's block sums, their scan and
    the scatter through order[] put every factor where its sub-pixel is.  In reverse order: the reversed result."""
    scene, _ = cases.scene_of(rt, scene_for, "blob16", "longest")
    opt, poses = shading.view_options(rt), shading.view_poses(rt)
    host = uploaded(rt, scene, opt)
    try:
        got = host.render_views(poses, rt.VIEW_OUTPUTS)
        assert tuple(got) == rt.VIEW_OUTPUTS
        assert host.last_views() == {"views": 3, "chunks": 1, "ao_points": int(got["hit"].sum())}
        again = host.render_views(poses[::-1], rt.VIEW_OUTPUTS)
    finally:
        host.close()
    shading.views_check(rt, oracle, scene_for, {n: got[n] for n in lo.NAMES}, got["image"])
    for f in rt.VIEW_OUTPUTS:
        same = lo.same_words(again[f], got[f][::-1])
        assert same.all(), (f, int((~same).sum()))


# ---- 4. an updated scene, a device-built scene ---------------------------------------------------------------------------
def host_ray_checks(what, surface, host, o, d, ref_of):
    shading.ray_checks(what, surface, o, d, ref_of, lambda o, d, md: host.trace_closest(o, d, md), lambda o, d, md: host.trace_occluded(o, d, md),
                       lambda o, d, md: host.count_hits(o, d, md), lambda o, d, md: host.trace_multihit(o, d, md, k=shading.K))


def test_updated_scene(rt, scene_for):
    """After update_vertices no tree-free check has looked: the reference needs the deformed vertices only."""
    host = rt.Host(shading.directional_options(rt, shading.BUILT_SETTING), 0)
    try:
        scene, step = shading.twisted_blob(rt, host)
        surface = shading.updated_surface(scene, step, cases.scene_of(rt, scene_for, "blob", "longest")[0])
        o, d = shading.blob_rays(rt, scene_for)
        host_ray_checks("blob twisted, updated on the device", surface, host, o, d, shading.surface_reference("updated", surface, o, d))
    finally:
        host.close()


def test_built_scene(rt, oracle, scene_for):
    """A tree the device built: leaves through the host's own face_of_leaf.  Then the same mesh at 1 / 16 of its size, built
    over the first scene, for one directional call (the CPU file's built_directional says why at that size)."""
    host = rt.Host(shading.directional_options(rt, shading.BUILT_SETTING), 0)
    try:
        v, f, scene = shading.built_mesh(rt, False)
        host.build_scene(v, f, scene.vnormals)
        surface = shading.built_surface(rt, False, host.face_of_leaf)
        assert np.array_equal(np.sort(host.face_of_leaf()), np.arange(len(f)))
        o, d = shading.blob_rays(rt, scene_for)
        host_ray_checks("blob, built on the device", surface, host, o, d, shading.surface_reference("built", surface, o, d))
        v16, f16, scene16 = shading.built_mesh(rt, True)
        host.build_scene(v16, f16, scene16.vnormals)
        shading.built_directional(rt, oracle, lambda o, d: host.trace_closest(o, d, 100000.0),
                                  lambda points, normals: host.directional_occlusion(points, normals),
                                  f"blob/16, built on the device {shading.setting_id(shading.BUILT_SETTING)}")
    finally:
        host.close()
