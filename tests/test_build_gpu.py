"""GPU: device-side builds (include/rt_hip_build.h) -- the records of a built host against an upload of Scene.build_lbvh's
arrays and against the numpy restatement of tests/build_cases.py; every query family, the frame layers and the views of a
built host against the CPU oracles over the LBVH scene, and against a host that uploaded the longest-axis scene; updates
and further builds on a built host; what a build closes and what it refuses; what an upload allocates."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import ao_oracle as aoo
import build_cases as bc
import directional_oracle as dro
import layers_oracle as lo
import multihit_oracle as mo
import orc
import query_oracle as qo
import refit_cases as rc
from test_ao_query_gpu import odd_points
from test_refit_gpu import make_host, same_bytes

pytestmark = pytest.mark.gpu

W, H = 64, 48
TIE_RAY_CAP = 0.01  # tests/test_build_cpu.py


def built_host(rt, mesh, **over):
    """(a host that built the mesh from numpy arrays, the LBVH scene of the same mesh, options)."""
    v, f = bc.mesh(mesh)
    scene = bc.lbvh_scene(rt, mesh)
    host, opt = make_host(rt, **over)
    host.build_scene(v, f, scene.vnormals)
    return host, scene, opt


@pytest.mark.parametrize("mesh", bc.MESHES)
def test_records_of_a_build(rt, mesh):
    host, scene, _ = built_host(rt, mesh)
    fresh, _ = make_host(rt, scene)  # (if this upload trips over the tree's depth, that is a finding on the upload side)
    got, want, tree = host.records(), fresh.records(), bc.restated(mesh)
    same_bytes(got, want, ("tris", "shade"), mesh)
    assert np.array_equal(got["nodes"]["skip"], tree["nodes"]) and np.array_equal(got["nodes"]["leaf"], tree["leaf"]), mesh
    rc.node_rule_holds(got["nodes"], got["tris"])
    assert np.array_equal(host.face_of_leaf(), scene.triangles) and np.array_equal(scene.triangles, tree["triangles"])
    leaf = np.array([0, 0xFFFFFFFF, len(scene.triangles) - 1], np.uint32)
    assert np.array_equal(host.face_of_leaf(leaf), scene.face_of_leaf(leaf))
    # the root box is the scene's own
    assert np.array_equal(rc.bits(got["nodes"][0]["lo"]), rc.bits(scene.aabbs[0, :3])) and np.array_equal(rc.bits(got["nodes"][0]["hi"]), rc.bits(scene.aabbs[1, :3]))
    assert host.last_build_ms > 0.0
    times = host.last_build_times()
    assert times["topology_ms"] > 0.0 and times["records_ms"] > 0.0 and times["schedule_host_ms"] >= 0.0
    host.close()
    fresh.close()


def test_normals_computed_for_the_host_form(rt):
    """vnormals=None: the CPU's routine, the normals Scene.from_arrays computes."""
    v, f = bc.mesh("blob")
    host, scene, _ = built_host(rt, "blob")
    other, _ = make_host(rt)
    other.build_scene(v, f)
    same_bytes(other.records(), host.records(), what="vnormals=None")
    host.close()
    other.close()


def test_device_memory_form():
    """Torch device tensors on a non-default stream == numpy arrays, on every mesh; the flag raised on the device
    (tests/build_torch_driver.py, a child process that brings torch's runtime up before it loads the library)."""
    driver = os.path.join(os.path.dirname(os.path.abspath(__file__)), "build_torch_driver.py")
    r = subprocess.run([sys.executable, driver], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "BUILD_TORCH_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def same(got, want, names, what):
    for f in names:
        ok = qo.same_words(got[f], want[f])
        assert ok.all(), (what, f, int((~ok).sum()), np.argwhere(~ok)[:5].tolist())


@pytest.mark.parametrize("mesh", ["blob", "ties"])
def test_every_family_on_a_built_scene(rt, mesh):
    """Against the CPU oracles over the LBVH scene's arrays, every output word: the leaf order is the same on both sides."""
    aod = 1.0 if mesh == "ties" else 0.2
    host, scene, opt = built_host(rt, mesh, ao_max_distance=aod)
    arrays, params = orc.SceneArrays.from_scene(scene), orc.params_from_options(opt)
    o4, d4 = bc.rays_for(rt, arrays)
    closest = host.trace_closest(o4, d4)
    want = qo.closest(arrays, o4, d4, 100000.0)
    assert want["hit"].any() and not want["hit"].all()
    same(closest, want, rt.api.QUERY_OUTPUTS, (mesh, "closest"))
    assert np.array_equal(host.trace_occluded(o4, d4), qo.occluded(arrays, o4, d4, 100000.0)), mesh
    want_multi = mo.multihit(arrays, o4, d4, 100000.0, 4)
    same(host.trace_multihit(o4, d4, k=4), want_multi, rt.api.MULTIHIT_OUTPUTS, (mesh, "multihit"))
    assert want_multi["count"].max() >= 2 and np.array_equal(host.count_hits(o4, d4), want_multi["count"])
    at = want["hit"].astype(bool)
    points, normals = odd_points(arrays, want["position"][at], want["normal"][at])
    same(host.ambient_occlusion(points, normals), aoo.ambient_occlusion(params, arrays, points, normals), rt.api.AO_OUTPUTS, (mesh, "ao"))
    want_dir = dro.directional(params, arrays, points, normals)
    same(host.directional_occlusion(points, normals), want_dir, rt.api.DIRECTIONAL_OUTPUTS, (mesh, "directional"))
    assert want_dir["occluded"].any()
    same(host.render_layers(), lo.render(params, arrays), rt.api.LAYER_OUTPUTS, (mesh, "layers"))
    poses = bc.two_poses(rt, arrays)
    views = host.render_views(poses, outputs=rt.VIEW_OUTPUTS)
    for v, pose in enumerate(poses):
        want_view = lo.render(params, arrays, pose)
        assert want_view["hit"].any(), (mesh, v)
        same({f: views[f][v] for f in rt.api.LAYER_OUTPUTS}, want_view, rt.api.LAYER_OUTPUTS, (mesh, "view", v))
    host.close()


@pytest.mark.parametrize("mesh", ["blob", "ties"])
def test_across_builders(rt, mesh):
    """Built host against a host that uploaded the longest-axis scene: hit, distance, occlusion, counts, AO and masks on all
    rays; faces and the remaining record words off the tie rays of tests/test_build_cpu.py."""
    aod = 1.0 if mesh == "ties" else 0.2
    host, scene, opt = built_host(rt, mesh, ao_max_distance=aod)
    plain = bc.longest_scene(rt, mesh)
    other, _ = make_host(rt, plain, ao_max_distance=aod)
    arrays = orc.SceneArrays.from_scene(plain)
    o4, d4 = bc.rays_for(rt, arrays)
    ties = bc.tie_rays(arrays, o4, d4)
    if mesh == "blob":
        assert ties.mean() <= TIE_RAY_CAP
    got, want = host.trace_closest(o4, d4), other.trace_closest(o4, d4)
    assert want["hit"].any() and not want["hit"].all()
    same(got, want, ("hit", "distance"), (mesh, "closest"))
    assert np.array_equal(host.trace_occluded(o4, d4), other.trace_occluded(o4, d4))
    m_got, m_want = host.trace_multihit(o4, d4, k=4), other.trace_multihit(o4, d4, k=4)
    same(m_got, m_want, ("count", "distance"), (mesh, "multihit"))
    assert np.array_equal(host.count_hits(o4, d4), other.count_hits(o4, d4))
    off = ~ties
    hit = want["hit"].astype(bool) & off
    assert np.array_equal(host.face_of_leaf(got["leaf"][hit]), plain.face_of_leaf(want["leaf"][hit]))
    same({f: got[f][off] for f in ("barycentric", "position", "normal")}, {f: want[f][off] for f in ("barycentric", "position", "normal")},
         ("barycentric", "position", "normal"), (mesh, "records off ties"))
    at = want["hit"].astype(bool)
    points, normals = odd_points(arrays, want["position"][at], want["normal"][at])
    same(host.ambient_occlusion(points, normals), other.ambient_occlusion(points, normals), rt.api.AO_OUTPUTS, (mesh, "ao"))
    same(host.directional_occlusion(points, normals), other.directional_occlusion(points, normals), rt.api.DIRECTIONAL_OUTPUTS, (mesh, "directional"))
    host.close()
    other.close()


@pytest.mark.parametrize("mesh", ["blob", "strip"])
def test_build_then_update(rt, mesh):
    host, scene, _ = built_host(rt, mesh)
    before = host.records()
    new = rc.steps("twist", scene.vertices)[-1]
    scene.refit(new)
    host.update_vertices(new, scene.vnormals)
    assert host.last_update_ms > 0.0
    fresh, _ = make_host(rt, scene)
    got, want = host.records(), fresh.records()
    same_bytes(got, want, ("tris", "shade"), mesh)
    assert np.array_equal(got["nodes"]["skip"], before["nodes"]["skip"]) and np.array_equal(got["nodes"]["leaf"], before["nodes"]["leaf"])
    rc.node_rule_holds(got["nodes"], got["tris"])
    leaves = scene.nodes == 1
    assert np.array_equal(rc.bits(got["tris"]["lo"]), rc.bits(scene.aabbs[0::2, :3][leaves]))
    assert np.array_equal(rc.bits(got["tris"]["hi"]), rc.bits(scene.aabbs[1::2, :3][leaves]))
    assert not np.array_equal(got["tris"]["ta"], before["tris"]["ta"])
    # another group size after the build: the schedule is made again from the skips the build brought back
    host.set_refit_group(7)
    host.update_vertices(new, scene.vnormals)
    same_bytes(host.records(), got, what="S = 7")
    host.close()
    fresh.close()


def test_build_again_and_upload(rt, golden):
    """blob, then ties on the same host: another triangle count, the second scene's answers; then upload_scene reopens
    render() and gives the golden frame."""
    from conftest import GOLDEN_DIR, options_for

    c = golden["renders"]["ties_33_s1_a3"]
    host = rt.Host(options_for(rt, c), 0)
    v, f = bc.mesh("blob")
    host.build_scene(v, f)
    first = host.records()
    v2, f2 = bc.mesh("ties")
    host.build_scene(v2, f2)
    second = host.records()
    assert len(first["tris"]) == len(f) != len(f2) == len(second["tris"])
    scene = bc.lbvh_scene(rt, "ties")
    arrays = orc.SceneArrays.from_scene(scene)
    ro, rd = mo.random_rays(arrays, 4096, 11)
    want = qo.closest(arrays, ro, rd, 100000.0)
    assert want["hit"].any()
    same(host.trace_closest(ro, rd), want, rt.api.QUERY_OUTPUTS, "second build")
    with pytest.raises(rt.RtError) as e:
        host.render()
    assert e.value.code == rt.api.RT_E_STATE
    plain = rt.Scene.load_off(os.path.join(GOLDEN_DIR, "meshes", "ties.off")).build_bvh(0)
    host.upload_scene(plain)
    with pytest.raises(rt.RtError) as e:
        host.face_of_leaf()
    assert e.value.code == rt.api.RT_E_STATE
    host.render()
    assert hashlib.sha256(host.download().tobytes()).hexdigest() == c["float_sha256"]
    assert hashlib.md5(rt.pgm_bytes(host.download_u8())).hexdigest() == c["pgm_md5"]
    host.close()


def test_closed_and_refused(rt):
    E_STATE, E_INVALID = rt.api.RT_E_STATE, rt.api.RT_E_INVALID
    v, f = bc.mesh("ties")

    def refused(call, code, word=None):
        with pytest.raises(rt.RtError) as e:
            call()
        assert e.value.code == code, e.value
        if word:
            assert word in e.value.message, e.value.message

    # a build may come first; it closes what an update closes
    host, scene, _ = built_host(rt, "ties")
    for call in (host.render, host.render_async, lambda: host.expect_frames(64), lambda: host.measure_tile_costs(1)):
        refused(call, E_STATE, "device-side build")
    assert host.render_layers(outputs=("value",))["value"].shape == (H, W)
    # the host form's refusals: the previous scene still answers
    good = host.records()
    arrays = orc.SceneArrays.from_scene(scene)
    ro, rd = mo.random_rays(arrays, 2048, 5)
    want = qo.closest(arrays, ro, rd, 100000.0)
    bad_faces = f.copy()
    bad_faces[len(f) // 2, 2] = len(v)
    bad_vertices = v.copy()
    bad_vertices[3, 1] = np.nan
    for call, word in ((lambda: host.build_scene(v, bad_faces), "out of range"), (lambda: host.build_scene(bad_vertices, f), "not finite"),
                       (lambda: host.build_scene(v, bad_faces, scene.vnormals), "out of range"),
                       (lambda: host.build_scene(v, np.zeros((0, 3), np.uint32)), "no faces")):
        refused(call, E_INVALID, word)
        same_bytes(host.records(), good, what=word)
        same(host.trace_closest(ro, rd), want, rt.api.QUERY_OUTPUTS, word)
    host.close()
    # the hosts of a frame ring share their scene
    ring = rt.FrameRing(rt.Options.defaults(width=32, height=32, ao_num_samples=3), hosts=2)
    ring.set_calibration(False)
    ring.upload_scene(bc.longest_scene(rt, "ties"))
    refused(lambda: ring.host(0).build_scene(v, f), E_STATE, "shared")
    ring.close()


def test_an_upload_allocates_what_it_did(rt, scene_for):
    """DeviceScene::bytes() of a plain upload is the parent commit's: bunny with these options, 20 837 632 bytes."""
    scene, _ = scene_for("bunny", "longest")
    ring = rt.FrameRing(rt.Options.defaults(width=W, height=H, n_super_samples=1, ao_num_samples=3, ao_max_distance=0.2), hosts=2)
    ring.set_calibration(False)
    ring.upload_scene(scene)
    scene_bytes, copies, _ = ring.device_bytes()
    ring.close()
    assert (scene_bytes, copies) == (20837632, 1)
