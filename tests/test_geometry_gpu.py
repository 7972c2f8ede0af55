"""GPU: ray, multi-hit and ambient-occlusion queries and posed frames against the BVH-free float64 reference of
tests/geometry_reference.py, directly: no CPU oracle stands between the kernels and the geometry.

The inputs, caps, floors and tolerances are those of tests/test_geometry_cpu.py (the oracles against the same reference).
Leaves come back in the tree's order and go through scene.face_of_leaf() before they meet the reference's file-order
faces.  The 6000 generic rays lie below RT_QUERY_SORT_MIN, where a call is never sorted: the sorted calls get three copies
of them, every copy compared."""
import numpy as np
import pytest

import geometry_reference as gr
import orc
import test_geometry_cpu as cases
from test_camera_gpu import STREAM

pytestmark = pytest.mark.gpu

SORT_MIN = 16384  # RT_QUERY_SORT_MIN (include/rt_hip_query.h): calls with fewer rays are never sorted
COPIES = 3  # 18000 or 21600 rays


@pytest.fixture(scope="module")
def hosts(rt, scene_for):
    made = {}

    def get(mesh, bvh, **options):
        key = (mesh, bvh, tuple(sorted(options.items())))
        if key not in made:
            scene, arrays = cases.scene_of(rt, scene_for, mesh, bvh)
            host = rt.Host(rt.Options.defaults(width=64, height=48, n_super_samples=1, **options), 0)
            host.upload_scene(scene)
            made[key] = (host, scene, arrays)
        return made[key]

    yield get
    for host, _, _ in made.values():
        host.close()


def copies(ref, rays):
    """The reference's answer and the rays, COPIES times over."""
    o, d = rays
    tiled = {f: (np.concatenate([v] * COPIES) if isinstance(v, np.ndarray) else v) for f, v in ref.items()}
    return tiled, np.concatenate([o] * COPIES), np.concatenate([d] * COPIES)


def generic(rt, hosts, mesh, bvh, max_distance):
    host, scene, arrays = hosts(mesh, bvh)
    o, d = cases.generic_rays(mesh, arrays)
    ref = cases.generic_reference(mesh, scene, o, d, max_distance)
    return host, scene, ref, o, d


@pytest.mark.parametrize("bvh", cases.BVHS)
@pytest.mark.parametrize("mesh", cases.GENERIC_MESHES)
def test_closest_occluded_and_count(rt, hosts, mesh, bvh):
    assert SORT_MIN <= COPIES * cases.N_RANDOM
    for md in cases.MAX_DISTANCES:
        host, scene, ref, o, d = generic(rt, hosts, mesh, bvh, md)
        what = f"{mesh}/{bvh} max_distance {md:g}"
        for sort in (False, True):
            r, oo, dd = copies(ref, (o, d)) if sort else (ref, o, d)
            how = " sorted" if sort else " unsorted"
            cases.passes(gr.compare_closest(scene, r, host.trace_closest(oo, dd, md, sort=sort)), what + " closest" + how)
            cases.passes(gr.compare_flags(r, host.trace_occluded(oo, dd, md, sort=sort), "occluded"), what + " occluded" + how)
            cases.passes(gr.compare_counts(r, host.count_hits(oo, dd, md, sort=sort)), what + " count" + how)
    ref = generic(rt, hosts, mesh, bvh, cases.MAX_DISTANCES[0])[2]
    assert (ref["count"] > 0).mean() >= cases.MIN_HIT_SHARE


@pytest.mark.parametrize("k", cases.KS)
@pytest.mark.parametrize("bvh", cases.BVHS)
@pytest.mark.parametrize("mesh", cases.GENERIC_MESHES)
def test_multihit_slots(rt, hosts, mesh, bvh, k):
    """k = 5, 9 and 15 run the K = 8 and K = 16 forms of the walk with fewer slots than the form keeps: the write-out of
    a list that is longer than the answer."""
    for md in cases.MAX_DISTANCES:
        host, scene, ref, o, d = generic(rt, hosts, mesh, bvh, md)
        what = f"{mesh}/{bvh} max_distance {md:g} multihit k={k}"
        cases.passes(gr.compare_multihit(scene, ref, host.trace_multihit(o, d, md, k=k, sort=False), k), what + " unsorted")
        if md in (cases.MAX_DISTANCES[0], cases.MAX_DISTANCES[2]):
            r, oo, dd = copies(ref, (o, d))
            cases.passes(gr.compare_multihit(scene, r, host.trace_multihit(oo, dd, md, k=k, sort=True), k), what + " sorted")
    if mesh == "layered":
        ref = generic(rt, hosts, mesh, bvh, cases.MAX_DISTANCES[0])[2]
        assert (ref["count"][:cases.N_AXIS] > 16).sum() >= cases.N_AXIS // 4


def ao_inputs(rt, hosts):
    """The points of tests/test_geometry_cpu.py's AO case, through the first tree's own closest hits."""
    first, _, first_arrays = hosts("blob16", cases.BVHS[0])
    return cases.ao_points(lambda o, d: first.trace_closest(o, d, 100000.0), first_arrays)


@pytest.mark.parametrize("bvh", cases.BVHS)
@pytest.mark.parametrize("samples,reach", cases.AO_SETTINGS)
def test_ao_queries(rt, oracle, hosts, samples, reach, bvh):
    points, normals = ao_inputs(rt, hosts)
    opt = cases.ao_options(rt, samples, reach)
    host, scene, _ = hosts("blob16", bvh, ao_num_samples=samples, ao_max_distance=reach)
    table = oracle.ao_table(orc.params_from_options(opt))  # (the direction table is an input here, as the points are)
    ref = cases.ao_reference(scene, opt, table, points, normals)
    assert host.ao_rays_per_point == (ref["rays"], ref["rays"])
    assert len(points) * ref["rays"] >= SORT_MIN
    for sort in (True, False):
        cases.passes(gr.compare_ao(ref, host.ambient_occlusion(points, normals, sort=sort)),
                     f"blob/16 {bvh} ao {samples} rings reach {reach:g} {'sorted' if sort else 'unsorted'}", cases.MAX_UNJUDGED_AO)
    assert (ref["occluded"] > 0).mean() >= cases.MIN_OCCLUDED_SHARE_EACH
    if (samples, reach) == cases.AO_SETTINGS[-1]:
        refs = [cases.ao_reference(scene, cases.ao_options(rt, s, r), oracle.ao_table(orc.params_from_options(cases.ao_options(rt, s, r))),
                                   points, normals) for s, r in cases.AO_SETTINGS]
        assert np.mean([(r["occluded"] > 0).mean() for r in refs]) >= cases.MIN_OCCLUDED_SHARE


def posed_host(rt, scene, opt, cam, stream):
    host = rt.Host(opt, 0)
    if stream:
        host.expect_frames(STREAM)
    host.set_camera(cam)
    host.upload_scene(scene)
    return host


@pytest.mark.parametrize("mode", ["one_shot", "stream"])
@pytest.mark.parametrize("mesh,pose", cases.FRAME_CASES)
def test_posed_frames(rt, scene_for, mesh, pose, mode):
    scene, arrays = cases.scene_of(rt, scene_for, mesh, "longest")
    cam = cases.frame_pose(rt, mesh, pose, arrays)
    for shading in (0, 1):
        ref = cases.frame_reference(rt, mesh, pose, scene, shading, cam)
        host = posed_host(rt, scene, cases.frame_options(rt, shading), cam, mode == "stream")
        try:
            for _ in range(2 if mode == "stream" else 1):
                host.render()
                cases.passes(gr.compare_frame(ref, host.download()), f"{mesh} {pose} {mode} {'shade' if shading else 'mask'}", max_unjudged=1.0)
        finally:
            host.close()
    assert ref["hit"].mean() >= cases.MIN_HIT_SHARE


def test_posed_frames_leave_few_pixels_unjudged(rt, scene_for):
    """The cap of tests/test_geometry_cpu.py's test of this name, for the references this file used."""
    assert cases.frames_unjudged_share(rt, scene_for) <= cases.MAX_UNJUDGED


def test_posed_frame_with_ambient_occlusion(rt, oracle, scene_for):
    """A posed frame with 3 AO rings on the unit-sized blob: on judged pixels whose AO point is judged the value is
    float32(shade) * float32(1 - occluded / 28) with the REFERENCE's occluded count at the host's own hit point, the shade
    from the host's own closest-hit normal (as tests/test_ao_query_gpu.py composes a frame from its queries)."""
    scene, _ = cases.scene_of(rt, scene_for, "blob16", "longest")
    a = np.radians(135)
    cam = rt.Camera.look_at((2 * np.sin(a) / 16, 0.3 / 16, 2 * np.cos(a) / 16), (0, 0, 0))  # orbit_135, at the blob's scale
    opt = cases.frame_options(rt, 1, ao=3)
    frame = gr.posed_frame(scene, cases.frame_options(rt, 1), cam)
    host = posed_host(rt, scene, opt, cam, False)
    try:
        host.render()
        image = host.download().reshape(-1)
        o, d = frame["origins"], frame["directions"]
        near = host.trace_closest(o, d, 100000.0)
        assert host.ao_rays_per_point == (28, 28)
    finally:
        host.close()
    judged, hit = frame["judged"].reshape(-1), near["hit"].astype(bool)
    assert np.array_equal(hit[judged], frame["hit"].reshape(-1)[judged])
    assert judged.mean() >= 1.0 - cases.MAX_UNJUDGED and hit.mean() >= cases.MIN_HIT_SHARE
    at = np.flatnonzero(hit)
    ref = gr.ao(scene, opt, oracle.ao_table(orc.params_from_options(opt)), near["position"][at], near["normal"][at])
    assert ref["rays"] == 28
    n, dd = near["normal"][at], d[at]
    shade = np.clip(-((n[:, 0] * dd[:, 0] + n[:, 1] * dd[:, 1]) + n[:, 2] * dd[:, 2]), np.float32(0), np.float32(1))
    assert shade.dtype == np.float32
    want = shade * ref["ao"]
    sure = judged[at] & ref["judged"]
    print(f"GEOMETRY posed frame with AO: {judged.mean():.4%} of the pixels judged, {ref['judged'].mean():.4%} of the {len(at)} AO points, "
          f"{(ref['occluded'] > 0).mean():.2%} of them occluded")
    assert ref["judged"].mean() >= 1.0 - cases.MAX_UNJUDGED_AO
    assert (ref["occluded"] > 0).mean() >= cases.MIN_OCCLUDED_SHARE_EACH
    bad = (image[at][sure].view(np.uint32) != want[sure].view(np.uint32)) & ~((image[at][sure] == 0) & (want[sure] == 0))  # (0 is 0)
    assert not bad.any(), (int(bad.sum()), np.flatnonzero(bad)[:5].tolist())
    assert (image[~hit & judged] == 0).all()
