"""GPU: vertex updates (include/rt_hip_update.h) -- the records after an update against a fresh upload of Scene.refit's arrays
and against the refit rule restated on the host; every query family, the frame layers and the views after an update against
the fresh upload and against the CPU oracles; the forms, the refusals, and what an upload allocates."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import ao_oracle as aoo
import directional_oracle as dro
import layers_oracle as lo
import multihit_oracle as mo
import orc
import query_oracle as qo
import refit_cases as rc
from test_ao_query_gpu import camera_hits, odd_points

pytestmark = pytest.mark.gpu

W, H = 64, 48
RECORDS = ("nodes", "tris", "shade")


def make_host(rt, scene=None, **over):
    base = dict(width=W, height=H, n_super_samples=1, ao_num_samples=3, ao_max_distance=0.2)
    base.update(over)
    opt = rt.Options.defaults(**base)
    host = rt.Host(opt, 0)
    if scene is not None:
        host.upload_scene(scene)
    return host, opt


def same_bytes(a: dict, b: dict, names=RECORDS, what=""):
    for name in names:
        assert a[name].dtype == b[name].dtype and a[name].shape == b[name].shape, (what, name)
        differ = np.flatnonzero((a[name].view(np.uint8).reshape(len(a[name]), -1) != b[name].view(np.uint8).reshape(len(b[name]), -1)).any(axis=1))
        assert differ.size == 0, (what, name, differ.size, differ[:5].tolist())


def updated_pair(rt, mesh, bvh, deformation, group_nodes=0):
    """(the scene after Scene.refit, the host that uploaded the original and was updated, its records before, a fresh host
    that uploaded the refit scene, options)."""
    scene = rc.fresh_scene(rt, mesh, bvh)
    host, opt = make_host(rt, scene)
    if group_nodes:
        host.set_refit_group(group_nodes)
    before = host.records()
    for step in rc.steps(deformation, scene.vertices):
        scene.refit(step)
        host.update_vertices(step, scene.vnormals)
    fresh, _ = make_host(rt, scene)
    return scene, host, before, fresh, opt


def check_records(scene, host, before, fresh, what):
    got, want = host.records(), fresh.records()
    same_bytes(got, want, ("tris", "shade"), what)  # by leaf index: whichever tree either host walks
    assert np.array_equal(got["nodes"]["skip"], before["nodes"]["skip"]) and np.array_equal(got["nodes"]["leaf"], before["nodes"]["leaf"]), what
    rc.node_rule_holds(got["nodes"], got["tris"])
    # the leaf records' boxes are the refit scene's own leaf boxes
    leaves = scene.nodes == 1
    assert np.array_equal(rc.bits(got["tris"]["lo"]), rc.bits(scene.aabbs[0::2, :3][leaves]))
    assert np.array_equal(rc.bits(got["tris"]["hi"]), rc.bits(scene.aabbs[1::2, :3][leaves]))
    return got


@pytest.mark.parametrize("deformation", rc.MOVING)
@pytest.mark.parametrize("bvh", ["longest", "sah"])
@pytest.mark.parametrize("mesh", ["ties", "blob", "bunny"])
def test_records_after_an_update(rt, mesh, bvh, deformation):
    scene, host, before, fresh, _ = updated_pair(rt, mesh, bvh, deformation)
    got = check_records(scene, host, before, fresh, (mesh, bvh, deformation))
    assert not np.array_equal(got["tris"]["ta"], before["tris"]["ta"])
    assert host.last_update_ms > 0.0
    host.close()
    fresh.close()


@pytest.mark.parametrize("mesh,group_nodes,passes", [("blob", 2, 3), ("blob", 7, 3), ("single", 0, 0)])
def test_records_through_several_passes(rt, mesh, group_nodes, passes):
    """blob at S = 2 and S = 7: an update of three passes or more; single: no inner node at all."""
    for deformation in rc.MOVING:
        scene, host, before, fresh, _ = updated_pair(rt, mesh, "longest", deformation, group_nodes)
        assert scene.refit_schedule(group_nodes, packed_tree=True)["passes"] >= passes
        check_records(scene, host, before, fresh, (mesh, group_nodes, deformation))
        host.close()
        fresh.close()


@pytest.mark.parametrize("mesh", ["ties", "bunny"])
def test_identity_and_return(rt, mesh):
    """Deformation 1 leaves all three arrays as the upload made them; after deformation 5 they are those again: no state
    accumulates."""
    scene, host, before, fresh, _ = updated_pair(rt, mesh, "longest", "identity")
    after_identity = host.records()
    same_bytes(after_identity, before, RECORDS, (mesh, "identity"))
    same_bytes(after_identity, fresh.records(), RECORDS, (mesh, "fresh"))
    for step in rc.steps("back", scene.vertices):
        scene.refit(step)
        host.update_vertices(step, scene.vnormals)
        assert np.array_equal(rc.bits(scene.vertices), rc.bits(step))
    same_bytes(host.records(), after_identity, RECORDS, (mesh, "back"))
    host.close()
    fresh.close()


def two_poses(rt, arrays):
    lo_, hi_ = mo.box_of(arrays)
    centre, size = (lo_ + hi_) / 2, float(np.max(hi_ - lo_))
    return [rt.Camera.look_at(tuple(centre + np.array(e) * size), tuple(centre)) for e in ((0.3, 0.4, 1.6), (-1.5, 0.2, -0.7))]


@pytest.mark.parametrize("deformation", ["far", "twist"])
@pytest.mark.parametrize("mesh", ["blob", "ties"])
def test_every_family_sees_the_update(rt, mesh, deformation):
    scene, host, _, fresh, opt = updated_pair(rt, mesh, "longest", deformation)
    arrays = orc.SceneArrays.from_scene(scene)
    params = orc.params_from_options(opt)
    what = (mesh, deformation)

    def same(got, want, names, tag):
        for f in names:
            ok = qo.same_words(got[f], want[f])
            assert ok.all(), (what, tag, f, int((~ok).sum()), np.argwhere(~ok)[:5].tolist())

    # the old camera's rays: after the far translation nothing is where it was, and nothing stale is walked
    d4, cam, hit, _ = camera_hits(rt, host)
    o4 = qo.camera_rays(orc.params_from_options(rt.Options.defaults(width=W, height=H, n_super_samples=1)))[0]
    if deformation == "far":
        assert not hit.any() and not host.trace_occluded(o4, d4).any() and not host.count_hits(o4, d4).any()
    else:
        assert hit.any()
    same(cam, qo.closest(arrays, o4, d4, 100000.0), rt.api.QUERY_OUTPUTS, "camera")
    # 4 096 random rays in and around the new root box
    ro, rd = mo.random_rays(arrays, 4096, 11)
    closest = host.trace_closest(ro, rd)
    assert closest["hit"].any() and not closest["hit"].all()
    same(closest, fresh.trace_closest(ro, rd), rt.api.QUERY_OUTPUTS, "closest / fresh")
    same(closest, qo.closest(arrays, ro, rd, 100000.0), rt.api.QUERY_OUTPUTS, "closest / oracle")
    occluded = host.trace_occluded(ro, rd)
    assert np.array_equal(occluded, fresh.trace_occluded(ro, rd)) and np.array_equal(occluded, qo.occluded(arrays, ro, rd, 100000.0)), what
    multi = host.trace_multihit(ro, rd, k=4)
    same(multi, fresh.trace_multihit(ro, rd, k=4), rt.api.MULTIHIT_OUTPUTS, "multihit / fresh")
    want_multi = mo.multihit(arrays, ro, rd, 100000.0, 4)
    same(multi, want_multi, rt.api.MULTIHIT_OUTPUTS, "multihit / oracle")
    assert want_multi["count"].any()
    assert np.array_equal(host.count_hits(ro, rd), want_multi["count"]), what
    # ambient and directional occlusion at the points those rays hit, odd ones among them
    at = closest["hit"].astype(bool)
    points, normals = odd_points(arrays, closest["position"][at], closest["normal"][at])
    ao = host.ambient_occlusion(points, normals)
    same(ao, fresh.ambient_occlusion(points, normals), rt.api.AO_OUTPUTS, "ao / fresh")
    same(ao, aoo.ambient_occlusion(params, arrays, points, normals), rt.api.AO_OUTPUTS, "ao / oracle")
    directional = host.directional_occlusion(points, normals)
    same(directional, fresh.directional_occlusion(points, normals), rt.api.DIRECTIONAL_OUTPUTS, "directional / fresh")
    same(directional, dro.directional(params, arrays, points, normals), rt.api.DIRECTIONAL_OUTPUTS, "directional / oracle")
    assert directional["occluded"].any()
    # the frame's own rays, and two poses around the new place
    layers = host.render_layers()
    same(layers, fresh.render_layers(), rt.api.LAYER_OUTPUTS, "layers / fresh")
    same(layers, lo.render(params, arrays), rt.api.LAYER_OUTPUTS, "layers / oracle")
    poses = two_poses(rt, arrays)
    views = host.render_views(poses, outputs=rt.VIEW_OUTPUTS)
    fresh_views = fresh.render_views(poses, outputs=rt.VIEW_OUTPUTS)
    same(views, fresh_views, rt.api.LAYER_OUTPUTS, "views / fresh")
    assert np.array_equal(views["image"], fresh_views["image"]), what
    for v, pose in enumerate(poses):
        want = lo.render(params, arrays, pose)
        assert want["hit"].any(), (what, v)
        same({f: views[f][v] for f in rt.api.LAYER_OUTPUTS}, want, rt.api.LAYER_OUTPUTS, ("view", v))
    host.close()
    fresh.close()


def test_sorted_queries_after_an_update(rt):
    """16 384 rays make the sort run: its key is cut from the root box, which an update must read afresh -- a stale box
    changes no result, so the box itself is looked at too: the records' root is the refit scene's."""
    scene, host, _, fresh, _ = updated_pair(rt, "blob", "longest", "far")
    arrays = orc.SceneArrays.from_scene(scene)
    ro, rd = mo.random_rays(arrays, 16384, 3)
    # (a second host whose sorted query before the update has cached the old box)
    again, _ = make_host(rt, rc.fresh_scene(rt, "blob", "longest"))
    again.trace_closest(ro, rd)
    again.update_vertices(scene.vertices, scene.vnormals)
    want = qo.closest(arrays, ro, rd, 100000.0)
    assert want["hit"].any()
    for h in (host, again):
        for sort in (True, False):
            got = h.trace_closest(ro, rd, sort=sort)
            for f in rt.api.QUERY_OUTPUTS:
                assert qo.same_words(got[f], want[f]).all(), (f, sort)
        root = h.records()["nodes"][0]
        assert np.array_equal(rc.bits(root["lo"]), rc.bits(scene.aabbs[0, :3])) and np.array_equal(rc.bits(root["hi"]), rc.bits(scene.aabbs[1, :3]))
    for h in (host, again, fresh):
        h.close()


def test_device_memory_form_equals_host_memory_form():
    """A torch device-tensor update on a non-default stream == the numpy update (tests/refit_torch_driver.py, a child
    process that brings torch's runtime up before it loads the library)."""
    driver = os.path.join(os.path.dirname(os.path.abspath(__file__)), "refit_torch_driver.py")
    r = subprocess.run([sys.executable, driver], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "REFIT_TORCH_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_forms_and_errors(rt, golden):
    E_STATE, E_INVALID = rt.api.RT_E_STATE, rt.api.RT_E_INVALID
    scene = rc.fresh_scene(rt, "ties", "longest")
    original = scene.vertices
    new = rc.deformed("twist", original)

    def refused(call, code, word=None):
        with pytest.raises(rt.RtError) as e:
            call()
        assert e.value.code == code, e.value
        if word:
            assert word in e.value.message, e.value.message

    # before an upload
    host, opt = make_host(rt)
    refused(lambda: host.update_vertices(new), E_STATE, "before a scene was uploaded")
    assert host.last_update_ms == 0.0
    host.upload_scene(scene)
    uploaded = host.records()
    # another vertex count; a vertex that is not a number: nothing is written
    refused(lambda: host.update_vertices(new[:-1]), E_INVALID, "number of vertices")
    for value in (np.nan, np.inf, 2e37):
        bad = new.copy()
        bad[3, 2] = value
        refused(lambda: host.update_vertices(bad), E_INVALID, "nothing was written")
    same_bytes(host.records(), uploaded, RECORDS, "refused updates")
    host.render()  # (a refused update closes nothing)
    frame = host.download().tobytes()
    # without normals the shading records stay and the leaf records change
    host.update_vertices(new)
    got = host.records()
    same_bytes(got, uploaded, ("shade",), "vnormals=None")
    assert not np.array_equal(got["tris"]["ta"], uploaded["tris"]["ta"])
    assert host.last_update_ms > 0.0
    # the frame path is closed until the next upload, and says why; layers and views are the way to images
    for call in (host.render, host.render_async, lambda: host.expect_frames(64), lambda: host.measure_tile_costs(1)):
        refused(call, E_STATE, "after a vertex update")
    assert host.render_layers(outputs=("value",))["value"].shape == (H, W)
    host.upload_scene(scene)
    host.render()
    assert host.download().tobytes() == frame
    host.close()
    # ... and that frame is the golden one
    c = golden["renders"]["ties_33_s1_a3"]
    from conftest import GOLDEN_DIR, options_for

    sized = rt.Host(options_for(rt, c), 0)
    plain = rt.Scene.load_off(os.path.join(GOLDEN_DIR, "meshes", "ties.off")).build_bvh(0)
    sized.upload_scene(plain)
    sized.update_vertices(rc.deformed("far", plain.vertices))
    refused(sized.render, E_STATE, "after a vertex update")
    sized.upload_scene(plain)
    sized.render()
    assert hashlib.sha256(sized.download().tobytes()).hexdigest() == c["float_sha256"]
    assert hashlib.md5(rt.pgm_bytes(sized.download_u8())).hexdigest() == c["pgm_md5"]
    sized.close()
    # the hosts of a frame ring share their scene
    ring = rt.FrameRing(rt.Options.defaults(width=32, height=32, ao_num_samples=3), hosts=2)
    ring.set_calibration(False)
    ring.upload_scene(scene)
    refused(lambda: ring.host(0).update_vertices(new), E_STATE, "shared")
    ring.close()


def test_an_upload_allocates_what_it_did(rt, scene_for):
    """A host that never updates: the bytes of the bunny's scene on the device, as a frame ring reports them (what a stream
    host's DeviceScene::create asks for), are 20 837 632 with these options -- the value the parent commit's library reports for
    the same call, read from a run of that library on the GPU -- and an update adds nothing to them: its faces, map and
    schedule live in an allocation of their own."""
    scene, _ = scene_for("bunny", "longest")
    ring = rt.FrameRing(rt.Options.defaults(width=W, height=H, n_super_samples=1, ao_num_samples=3, ao_max_distance=0.2), hosts=2)
    ring.set_calibration(False)
    ring.upload_scene(scene)
    scene_bytes, copies, _ = ring.device_bytes()
    ring.close()
    assert (scene_bytes, copies) == (PARENT_BUNNY_SCENE_BYTES, 1)


PARENT_BUNNY_SCENE_BYTES = 20837632
