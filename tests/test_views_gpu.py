"""GPU: multi-view rendering (include/rt_hip_views.h) against the CPU oracle of the frame layers, against freshly posed
hosts and their frames, and against itself (subsets, chunks, permutations), word for word (NaN equal to NaN)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import layers_cases as lc
import layers_oracle as lo
import orc
from conftest import bits
from test_camera_gpu import poses_for

pytestmark = pytest.mark.gpu

NAMED = [p for p in lc.POSES if p is not None]  # the six named poses; Camera.default() is the seventh view


def _parity_cases():
    """One call per (mesh, size): the trees alternate and the (shading, AO rings) of layers_cases.OPTIONS go round, so that
    every mesh meets both trees, shading on and off and both ring counts; the bunny at 64 x 48 on both trees."""
    out, k = [], 0
    for mesh in ("blob", "ties", "single"):
        for size in lc.SIZES:
            shading, ao = lc.OPTIONS[k % 4]
            out.append((mesh, lc.TREES[(k // 4 + k) % 2], *size, shading, ao))
            k += 1
    for tree in lc.TREES:
        shading, ao = lc.OPTIONS[k % 4]
        out.append(("bunny", tree, 64, 48, 1, shading, ao))
        k += 1
    return out


PARITY_CASES = _parity_cases()


def parity_id(c) -> str:
    return f"{c[0]}_{c[1]}_{c[2]}x{c[3]}_s{c[4]}_sh{c[5]}_a{c[6]}"


def cameras_of(rt, scene_for) -> dict:
    return poses_for(rt, scene_for("bunny", "longest")[1])


_DEFAULT_POSED = {}


def oracle_view(rt, scene_for, c, pose):
    """The oracle's layers of one view of a parity case: the POSED form, for the default pose too."""
    mesh, tree, w, h, ss, shading, ao = c
    if pose is not None:
        return lc.oracle_layers(rt, scene_for, (mesh, tree, w, h, ss, pose, shading, ao))
    if c not in _DEFAULT_POSED:
        opt = lc.options_of(rt, (mesh, tree, w, h, ss, None, shading, ao))
        _DEFAULT_POSED[c] = lo.render(orc.params_from_options(opt), scene_for(mesh, tree)[1], rt.Camera.default())
    return _DEFAULT_POSED[c]


def assert_block(got, v, want, names, what=""):
    for f in names:
        block = got[f][v]
        assert block.shape == want[f].shape and block.dtype == want[f].dtype, (what, f, v, block.shape, block.dtype)
        same = lo.same_words(block, want[f])
        assert same.all(), (what, f, v, int((~same).sum()), np.argwhere(~same)[:5].tolist())


def assert_same(a, b, names, what=""):
    for f in names:
        assert a[f].shape == b[f].shape and a[f].dtype == b[f].dtype, (what, f)
        same = lo.same_words(a[f], b[f])
        assert same.all(), (what, f, int((~same).sum()), np.argwhere(~same)[:5].tolist())


def upload(rt, scene, opt, cam=None, frames=None):
    host = rt.Host(opt, 0)
    if frames:
        host.expect_frames(frames)
    if cam is not None:
        host.set_camera(cam)
    host.upload_scene(scene)
    return host


# ---- 1. oracle parity ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", PARITY_CASES, ids=parity_id)
def test_oracle_parity(rt, scene_for, c):
    mesh, tree, w, h, ss, shading, ao = c
    scene, _ = scene_for(mesh, tree)
    opt = lc.options_of(rt, (mesh, tree, w, h, ss, None, shading, ao))
    named = cameras_of(rt, scene_for)
    cams = [named[p] for p in NAMED] + [rt.Camera.default()]
    poses = NAMED + [None]
    plain = upload(rt, scene, opt)                  # a host without a pose ...
    posed = upload(rt, scene, opt, named["below"])  # ... and one uploaded for some other pose
    try:
        got = plain.render_views(cams, rt.VIEW_OUTPUTS)
        assert tuple(got) == rt.VIEW_OUTPUTS
        assert got["hit"].shape == (7, opt.total_height, opt.total_width) and got["normal"].shape == (7, opt.total_height, opt.total_width, 3)
        assert got["image"].shape == (7, opt.height, opt.width) and got["image"].dtype == np.uint8
        for v, pose in enumerate(poses):
            want = oracle_view(rt, scene_for, c, pose)
            assert_block(got, v, want, lo.NAMES, parity_id(c) + f" view {v} {pose}")
            assert np.array_equal(got["image"][v], rt.resize_cpu(opt, want["value"])), (v, pose)
            if pose in lc.SEES_NOTHING:
                assert not got["hit"][v].any()
        if (w, h) != (1, 1):
            assert got["hit"].any() and not got["hit"].all()
        assert plain.last_views() == {"views": 7, "chunks": 1, "ao_points": int(got["hit"].sum())}
        other = posed.render_views(cams, rt.VIEW_OUTPUTS)
        assert_same(other, got, rt.VIEW_OUTPUTS, "a host with a pose of its own")
        if (w, h, ss) == (37, 23, 1):  # 3 views x 15 tiles: no multiple of the four waves of a workgroup either
            three = plain.render_views(np.stack([cam.as_array() for cam in cams[:3]]), rt.VIEW_OUTPUTS)
            for f in rt.VIEW_OUTPUTS:
                assert lo.same_words(three[f], got[f][:3]).all(), f
    finally:
        plain.close()
        posed.close()


# ---- 2. against a freshly posed host and its frame -----------------------------------------------------------------
FRESH_CASES = [("bunny", "longest", 64, 48, 1, None, 1, 3), ("blob", "sah", 37, 23, 1, "roll", 1, 2),
                          ("ties", "longest", 11, 6, 9, "orbit_135", 0, 3), ("blob", "longest", 8, 8, 4, "skewed", 1, 2)]


def test_fresh_cases_hold_the_layers_tests_frame_cases():
    from test_layers_gpu import FRAME_CASES

    assert FRESH_CASES[:3] == FRAME_CASES
    assert {c[2:5] for c in FRESH_CASES} >= {(11, 6, 9), (8, 8, 4)}


@pytest.mark.parametrize("ao", ["uniform", "random", "off"])
@pytest.mark.parametrize("case", FRESH_CASES, ids=lc.case_id)
def test_views_are_freshly_posed_hosts(rt, scene_for, case, ao):
    """Views 1 and 3 of a four-view call == a host created, posed, uploaded and rendered for that pose alone: every layer,
    the float image, the 8-bit image.  Neither is the call's first view: a seed counted through the batch would show in
    the RANDOM method's `ao`."""
    over = {"uniform": {}, "random": {"ao_method": 1}, "off": {"ao_num_samples": 0, "enable_ao": 0}}[ao]
    scene, _ = scene_for(case[0], case[1])
    opt = lc.options_of(rt, case, **over)
    named = cameras_of(rt, scene_for)
    mine = rt.Camera.default() if case[5] is None else named[case[5]]
    cams = [named["orbit_40"], mine, named["far_1e7"], named["orbit_225"]]
    names = tuple(n for n in rt.VIEW_OUTPUTS if ao != "off" or n != "ao")
    host = upload(rt, scene, opt)
    try:
        got = host.render_views(cams, names)
        assert got["hit"][1].any() and not got["hit"][2].any()
        for v in (1, 3):
            fresh = upload(rt, scene, opt, cams[v])
            try:
                layers = fresh.render_layers(tuple(n for n in names if n != "image"))
                fresh.render()
                img, u8 = fresh.download(), fresh.download_u8()
            finally:
                fresh.close()
            assert_block(got, v, layers, tuple(layers), f"view {v}")
            assert np.array_equal(bits(got["value"][v]), bits(img)), v
            assert np.array_equal(got["image"][v], u8), v
            assert np.array_equal(got["image"][v], rt.resize_cpu(opt, got["value"][v])), v
            if ao == "off":
                assert np.array_equal(bits(got["value"][v]), bits(got["shade"][v]))
    finally:
        host.close()


# ---- 3. compaction ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1], ids=["uniform", "random"])
def test_only_hit_sub_pixels_reach_the_ao_step(rt, scene_for, method):
    scene, _ = scene_for("bunny", "sah")
    opt = rt.Options.defaults(width=37, height=23, n_super_samples=4, ao_num_samples=3, ao_method=method, bvh_method=1)
    named = cameras_of(rt, scene_for)
    order = ["orbit_135", "far_1e7", "roll", "infinite", "skewed"]
    cams = [named[p] for p in order]
    host = upload(rt, scene, opt)
    try:
        got = host.render_views(cams, rt.VIEW_OUTPUTS)
        hit = got["hit"].astype(bool)
        assert [bool(hit[v].any()) for v in range(5)] == [True, False, True, False, True]
        assert host.last_views() == {"views": 5, "chunks": 1, "ao_points": int(hit.sum())}
        assert (got["ao"][~hit] == 1.0).all() and (bits(got["value"][~hit]) == 0).all()
        assert not got["image"][1].any() and not got["image"][3].any() and got["image"][0].any()
        # in reverse, and in another order: the blocks go with their cameras
        for perm in ([4, 3, 2, 1, 0], [3, 0, 4, 1, 2]):
            again = host.render_views([cams[j] for j in perm], rt.VIEW_OUTPUTS)
            assert host.last_views()["ao_points"] == int(hit.sum())
            for f in rt.VIEW_OUTPUTS:
                assert lo.same_words(again[f], got[f][perm]).all(), (f, perm)
        # a camera given twice gives the same block twice
        twice = host.render_views([cams[0], cams[2], cams[0]], rt.VIEW_OUTPUTS)
        assert host.last_views()["ao_points"] == int(2 * hit[0].sum() + hit[2].sum())
        for f in rt.VIEW_OUTPUTS:
            assert lo.same_words(twice[f][0], twice[f][2]).all() and lo.same_words(twice[f], got[f][[0, 2, 0]]).all(), f
        # views that all see nothing: no point at all, and still every default
        none = host.render_views([cams[1], cams[3], cams[1]], rt.VIEW_OUTPUTS)
        assert host.last_views() == {"views": 3, "chunks": 1, "ao_points": 0}
        assert not none["hit"].any() and (none["ao"] == 1.0).all() and (bits(none["value"]) == 0).all() and not none["image"].any()
        assert np.isposinf(none["distance"]).all() and (none["leaf"] == 0xFFFFFFFF).all() and host.last_query_ms > 0.0
    finally:
        host.close()


# ---- 4. chunks -------------------------------------------------------------------------------------------------------
def test_chunks(rt, scene_for):
    scene, _ = scene_for("blob", "longest")
    opt = rt.Options.defaults(width=37, height=23, n_super_samples=1, ao_num_samples=2, ao_max_distance=0.2)
    named = cameras_of(rt, scene_for)
    cams = [named[p] for p in ("orbit_135", "roll", "far_1e7", "skewed", "inside_root_box")]
    host = upload(rt, scene, opt)
    try:
        auto = host.render_views(cams, rt.VIEW_OUTPUTS)
        points = int(auto["hit"].sum())
        assert points and host.last_views() == {"views": 5, "chunks": 1, "ao_points": points}
        host.set_views_chunk(2)  # 2 + 2 + 1
        got = host.render_views(cams, rt.VIEW_OUTPUTS)
        assert host.last_views() == {"views": 5, "chunks": 3, "ao_points": points}
        assert_same(got, auto, rt.VIEW_OUTPUTS, "three chunks")
        one = host.render_views(cams[3:4], rt.VIEW_OUTPUTS)  # the scratch shrinks ...
        assert host.last_views() == {"views": 1, "chunks": 1, "ao_points": int(auto["hit"][3].sum())}
        for f in rt.VIEW_OUTPUTS:
            assert lo.same_words(one[f][0], auto[f][3]).all(), f
        assert_same(host.render_views(cams, rt.VIEW_OUTPUTS), auto, rt.VIEW_OUTPUTS, "... and grows again")
        host.set_views_chunk(1)
        assert_same(host.render_views(cams, ("image", "ao")), auto, ("image", "ao"), "a view per chunk")
        assert host.last_views()["chunks"] == 5
        host.set_views_chunk(0)
        assert_same(host.render_views(cams, rt.VIEW_OUTPUTS), auto, rt.VIEW_OUTPUTS, "automatic again")
        assert host.last_views()["chunks"] == 1
    finally:
        host.close()


# ---- 5. subsets ------------------------------------------------------------------------------------------------------
def test_subsets(rt, scene_for):
    scene, _ = scene_for("blob", "sah")
    opt = rt.Options.defaults(width=11, height=6, n_super_samples=9, ao_num_samples=2, ao_max_distance=0.2, bvh_method=1)
    named = cameras_of(rt, scene_for)
    cams = [named["roll"], named["infinite"], named["orbit_135"]]
    host = upload(rt, scene, opt)
    try:
        everything = host.render_views(cams, rt.VIEW_OUTPUTS)
        assert everything["hit"].any() and everything["image"].any()
        for name in rt.VIEW_OUTPUTS:
            alone = host.render_views(cams, (name,))
            assert tuple(alone) == (name,)
            assert_same(alone, everything, (name,), "alone")
        assert tuple(host.render_views(cams)) == ("value",)
        assert_same(host.render_views(cams, ("image", "leaf")), everything, ("image", "leaf"), "pair")
        # nothing to do: no view, no output
        assert host.render_views(cams, ()) == {}
        empty = host.render_views([], rt.VIEW_OUTPUTS)
        assert empty["value"].shape == (0, opt.total_height, opt.total_width) and empty["image"].shape == (0, opt.height, opt.width)
        assert host.render_views(np.zeros((0, 4, 3), np.float32), ("hit",))["hit"].shape[0] == 0
        lib = rt.load_library()
        nothing = rt.api._ViewArrays()
        poses = np.stack([cam.as_array() for cam in cams])
        assert lib.rt_render_views(host._h, poses.ctypes.data, 3, C.byref(nothing)) == 0
        assert lib.rt_render_views_device(host._h, poses.ctypes.data, 3, C.byref(nothing), None) == 0
        assert lib.rt_render_views(host._h, None, 0, C.byref(nothing)) == 0
        # an array the call was not given stays as it is
        guard = np.full((3, opt.total_height, opt.total_width), 7.0, np.float32)
        only = rt.api._ViewArrays(rt.api._LayerArrays(shade=guard.ctypes.data), None)
        assert lib.rt_render_views(host._h, poses.ctypes.data, 3, C.byref(only)) == 0
        assert np.array_equal(bits(guard), bits(everything["shade"]))
    finally:
        host.close()
    # ambient occlusion off: value and image come from the head-light term; no `ao`
    off = upload(rt, scene, rt.Options.defaults(width=11, height=6, n_super_samples=9, ao_num_samples=0, enable_ao=0, bvh_method=1))
    try:
        with pytest.raises(rt.RtError) as e:
            off.render_views(cams, ("ao",))
        assert e.value.code == rt.api.RT_E_STATE and "ambient occlusion off" in e.value.message
        got = off.render_views(cams, tuple(n for n in rt.VIEW_OUTPUTS if n != "ao"))
        assert np.array_equal(bits(got["value"]), bits(got["shade"])) and got["hit"].any()
        assert np.array_equal(bits(got["shade"]), bits(everything["shade"]))
        for v in range(3):
            assert np.array_equal(got["image"][v], rt.resize_cpu(off.options, got["shade"][v]))
        assert_same(off.render_views(cams, ("image",)), got, ("image",), "image alone, from shade")
        assert off.last_views() == {"views": 3, "chunks": 1, "ao_points": 0}
    finally:
        off.close()


# ---- 6. non-interference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", [None, 16], ids=["one_shot", "stream"])
def test_frames_are_left_alone(rt, scene_for, frames):
    scene, _ = scene_for("bunny", "longest")
    opt = rt.Options.defaults(width=64, height=48, n_super_samples=1, ao_num_samples=3)
    named = cameras_of(rt, scene_for)
    host = upload(rt, scene, opt, named["roll"], frames)
    try:
        host.render()
        img, u8, stats, launches, kernel_ms = host.download(), host.download_u8(), host.stats(), host.kernel_launches, host.last_kernel_ms
        got = host.render_views([named["orbit_135"], named["roll"], named["far_1e7"]], rt.VIEW_OUTPUTS)
        assert np.array_equal(bits(host.download()), bits(img)) and np.array_equal(host.download_u8(), u8)
        assert host.stats() == stats and host.kernel_launches == launches and host.last_kernel_ms == kernel_ms
        assert np.array_equal(bits(got["value"][1]), bits(img)) and np.array_equal(got["image"][1], u8)
        assert not np.array_equal(got["image"][0], u8) and host.last_query_ms > 0.0
        host.render()
        assert np.array_equal(bits(host.download()), bits(img)) and np.array_equal(host.download_u8(), u8)
        assert host.stats() == stats and host.kernel_launches > launches
        host.render_async()  # a views call behind a frame in flight on the host's stream
        again = host.render_views([named["roll"]], ("value", "image"))
        host.sync()
        assert np.array_equal(bits(again["value"][0]), bits(img)) and np.array_equal(bits(host.download()), bits(img))
        assert host.camera_is_set and np.array_equal(bits(host.camera().as_array()), bits(named["roll"].as_array()))
    finally:
        host.close()


# ---- 7. errors -------------------------------------------------------------------------------------------------------
def test_errors(rt, scene_for):
    E_INVALID, E_STATE = rt.api.RT_E_INVALID, rt.api.RT_E_STATE
    lib = rt.load_library()
    scene, _ = scene_for("blob", "longest")
    opt = rt.Options.defaults(width=32, height=24, n_super_samples=1, ao_num_samples=2)
    cams = [rt.Camera.default(), cameras_of(rt, scene_for)["roll"]]
    poses = np.stack([cam.as_array() for cam in cams])
    nothing = rt.api._ViewArrays()
    host = rt.Host(opt, 0)
    with pytest.raises(rt.RtError) as e:  # before the upload
        host.render_views(cams)
    assert e.value.code == E_STATE
    assert lib.rt_render_views_device(host._h, poses.ctypes.data, 2, C.byref(nothing), None) == E_STATE
    assert host.last_views() == {"views": 0, "chunks": 0, "ao_points": 0}
    host.upload_scene(scene)
    assert lib.rt_render_views(host._h, poses.ctypes.data, 2, None) == E_INVALID  # a NULL `out`
    assert lib.rt_render_views_device(host._h, poses.ctypes.data, 2, None, None) == E_INVALID
    assert lib.rt_render_views(None, poses.ctypes.data, 2, C.byref(nothing)) == E_INVALID
    assert lib.rt_render_views(host._h, None, 2, C.byref(nothing)) == E_INVALID  # NULL cameras with views > 0
    assert lib.rt_render_views_device(host._h, None, 1, C.byref(nothing), None) == E_INVALID
    # a misaligned device pointer is refused before anything is enqueued (the address is never used)
    for field in ("distance", "leaf", "barycentric", "position", "normal", "direction", "shade", "ao", "value"):
        arrays = rt.api._ViewArrays(rt.api._LayerArrays(**{field: 0x1002}), None)
        assert lib.rt_render_views_device(host._h, poses.ctypes.data, 2, C.byref(arrays), None) == E_INVALID, field
    assert "4-byte aligned" in lib.rt_last_error().decode()
    assert host.render_views(cams, ("hit",))["hit"].any()
    host.close()
    # ambient occlusion off: no `ao`
    off = rt.Host(rt.Options.defaults(width=32, height=24, n_super_samples=1, ao_num_samples=0, enable_ao=0), 0)
    off.upload_scene(scene)
    with pytest.raises(rt.RtError) as e:
        off.render_views(cams, rt.VIEW_OUTPUTS)
    assert e.value.code == E_STATE and "ambient occlusion off" in e.value.message
    assert off.render_views(cams, ("image",))["image"].any()
    off.close()
    # a band-partitioned host renders a part of the image only
    for rank in range(2):
        part = rt.Host(opt, 0, rank, 2)
        part.upload_scene(scene)
        with pytest.raises(rt.RtError) as e:
            part.render_views(cams, ("hit",))
        assert e.value.code == E_STATE and "band-partitioned" in e.value.message
        part.close()
    # the hosts of a ring
    ring = rt.FrameRing(opt, scene, device=0, hosts=2)
    with pytest.raises(rt.RtError) as e:
        ring.host(0).render_views(cams, ("hit",))
    assert e.value.code == E_STATE and "frame ring" in e.value.message
    assert lib.rt_debug_set_views_chunk(ring.host(0)._h, 2) == E_STATE and lib.rt_debug_last_views(ring.host(0)._h, None, None, None) == E_STATE
    ring.close()
    # ONE view beyond what an ambient-occlusion query takes: 1920 x 1080 x 71 rays > RT_QUERY_MAX_RAYS
    big = rt.Host(rt.Options.defaults(width=1920, height=1080, n_super_samples=1, ao_num_samples=5), 0)
    big.upload_scene(scene)
    assert big.ao_rays_per_point[0] == 71 and 1920 * 1080 * 71 > 1 << 27
    for names in (("ao",), ("value",), ("image",)):
        with pytest.raises(rt.RtError) as e:
            big.render_views(cams[:1], names)
        assert e.value.code == E_INVALID and "RT_QUERY_MAX_RAYS" in e.value.message
    assert big.render_views(cams[:1], ("hit",))["hit"].any()  # (the other layers have no such limit)
    big.close()


# ---- 8. the device form ----------------------------------------------------------------------------------------------
def test_torch_path_equals_numpy_path():
    """as_torch=True under a stream of the caller's == the numpy path, one chunk and several (tests/views_torch_driver.py, a
    fresh child process that brings torch's runtime up before it loads the library)."""
    driver = os.path.join(os.path.dirname(os.path.abspath(__file__)), "views_torch_driver.py")
    r = subprocess.run([sys.executable, driver], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "VIEWS_TORCH_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
