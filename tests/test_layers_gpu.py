"""GPU: the frame layers (include/rt_hip_layers.h) against the CPU oracle of tests/layers_oracle.c, the frame, the ray and
ambient-occlusion queries, word for word (NaN equal to NaN)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import layers_cases as lc
import layers_oracle as lo
from conftest import bits

pytestmark = pytest.mark.gpu

STREAM = 16  # frames announced before the upload (tests/test_camera_gpu.py)


def make_host(rt, scene_for, case, frames=None, **overrides):
    scene, _ = scene_for(case[0], case[1])
    opt = lc.options_of(rt, case, **overrides)
    host = rt.Host(opt, 0)
    if frames:
        host.expect_frames(frames)
    cam = lc.camera_of(rt, scene_for, case)
    if cam is not None:
        host.set_camera(cam)
    host.upload_scene(scene)
    return host, opt


def assert_layers(got, want, names, what=""):
    for f in names:
        assert got[f].shape == want[f].shape and got[f].dtype == want[f].dtype, (what, f, got[f].shape, got[f].dtype)
        same = lo.same_words(got[f], want[f])
        assert same.all(), (what, f, int((~same).sum()), np.argwhere(~same)[:5].tolist())


@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_oracle_parity(rt, scene_for, case):
    want = lc.oracle_layers(rt, scene_for, case)
    host, opt = make_host(rt, scene_for, case)
    try:
        got = host.render_layers()
        assert tuple(got) == rt.LAYER_OUTPUTS
        assert got["hit"].shape == (opt.total_height, opt.total_width) and got["normal"].shape == (opt.total_height, opt.total_width, 3)
        hit = got["hit"].astype(bool)
        if lc.must_see_both(case):
            assert hit.any() and (~hit).any()
        assert_layers(got, want, lo.NAMES, lc.case_id(case))
    finally:
        host.close()


# what `value` is compared with here is the frame of the same host: the same device, the same libm for RANDOM
FRAME_CASES = [("bunny", "longest", 64, 48, 1, None, 1, 3), ("blob", "sah", 37, 23, 1, "roll", 1, 2), ("ties", "longest", 11, 6, 9, "orbit_135", 0, 3)]


@pytest.mark.parametrize("frames", [None, STREAM], ids=["one_shot", "stream"])
@pytest.mark.parametrize("ao", ["uniform", "random", "off"])
@pytest.mark.parametrize("case", FRAME_CASES, ids=lc.case_id)
def test_value_is_the_frames_image(rt, scene_for, case, ao, frames):
    over = {"uniform": {}, "random": {"ao_method": 1}, "off": {"ao_num_samples": 0, "enable_ao": 0}}[ao]
    host, opt = make_host(rt, scene_for, case, frames, **over)
    try:
        names = tuple(n for n in rt.LAYER_OUTPUTS if ao != "off" or n != "ao")
        before = host.render_layers(names)  # (before the first frame, too)
        host.render()
        img = host.download()
        got = host.render_layers(names)
        assert np.array_equal(bits(got["value"]), bits(img))
        assert got["hit"].any()
        if ao == "off":
            assert np.array_equal(bits(got["shade"]), bits(img))
        else:
            assert lo.same_words(got["value"], got["shade"] * got["ao"]).all()
            assert (got["ao"][got["hit"] == 0] == 1.0).all()
        assert_layers(before, got, names, "before / after the frame")
        if ao != "random":
            want = lc.oracle_layers(rt, scene_for, case, **over)
            assert_layers(got, want, names)
        assert host.stats()["primary_hits"] == int(got["hit"].sum())
    finally:
        host.close()


QUERY_CASES = [("bunny", "sah", 64, 48, 1, "skewed", 1, 3), ("ties", "longest", 37, 23, 1, None, 1, 2), ("blob", "longest", 11, 6, 9, "inside_root_box", 0, 5),
               ("bunny", "longest", 64, 48, 1, "infinite", 1, 3)]


@pytest.mark.parametrize("method", [0, 1], ids=["uniform", "random"])
@pytest.mark.parametrize("case", QUERY_CASES, ids=lc.case_id)
def test_layers_are_the_queries_answers(rt, scene_for, case, method):
    """`direction` and the eye through trace_closest: every record layer; ambient_occlusion(position, normal) over all the
    sub-pixels in index order (seeds None: 0 .. N-1): `ao` where hit."""
    host, opt = make_host(rt, scene_for, case, ao_method=method)
    try:
        got = host.render_layers()
        eye = host.camera().as_array()[0]
        assert np.array_equal(bits(eye), bits(lc.eye_of(rt, scene_for, case)))
        o, d = lc.rays_of(rt, scene_for, case, got["direction"])
        for sort in (True, False):
            rec = host.trace_closest(o, d, 100000.0, sort=sort)
            for f in lo.RECORD:
                assert lo.same_words(got[f].reshape(rec[f].shape), rec[f]).all(), (f, sort)
        hit = got["hit"].reshape(-1).astype(bool)
        ao = host.ambient_occlusion(got["position"].reshape(-1, 3), got["normal"].reshape(-1, 3), outputs=("ao",), sort=False)["ao"]
        assert np.array_equal(bits(ao[hit]), bits(got["ao"].reshape(-1)[hit]))
        assert (got["ao"].reshape(-1)[~hit] == 1.0).all()
        assert host.last_query_ms > 0.0
    finally:
        host.close()


def test_one_layer_at_a_time(rt, scene_for):
    case = ("blob", "longest", 37, 23, 1, "orbit_135", 1, 2)
    host, opt = make_host(rt, scene_for, case)
    try:
        everything = host.render_layers()
        for name in rt.LAYER_OUTPUTS:
            one = host.render_layers((name,))
            assert tuple(one) == (name,)
            assert_layers(one, everything, (name,), "alone")
        pair = host.render_layers(("value", "leaf"))
        assert_layers(pair, everything, ("value", "leaf"), "pair")
        assert host.render_layers(()) == {}
        lib = rt.load_library()
        empty = rt.api._LayerArrays()
        assert lib.rt_render_layers(host._h, C.byref(empty)) == 0
        assert lib.rt_render_layers_device(host._h, C.byref(empty), None) == 0
        # an empty request writes nothing: the arrays it was not given stay as they are
        guard = np.full((opt.total_height, opt.total_width), 7.0, np.float32)
        only = rt.api._LayerArrays(shade=guard.ctypes.data)
        assert lib.rt_render_layers(host._h, C.byref(only)) == 0
        assert np.array_equal(bits(guard), bits(everything["shade"]))
    finally:
        host.close()


@pytest.mark.parametrize("frames", [None, STREAM], ids=["one_shot", "stream"])
def test_frames_are_left_alone(rt, scene_for, frames):
    case = ("bunny", "longest", 64, 48, 1, "roll", 1, 3)
    host, opt = make_host(rt, scene_for, case, frames)
    try:
        host.render()
        img, u8, stats, launches = host.download(), host.download_u8(), host.stats(), host.kernel_launches
        kernel_ms = host.last_kernel_ms
        layers = host.render_layers()
        assert np.array_equal(bits(host.download()), bits(img)) and np.array_equal(host.download_u8(), u8)
        assert host.stats() == stats and host.kernel_launches == launches and host.last_kernel_ms == kernel_ms
        assert np.array_equal(bits(layers["value"]), bits(img))
        host.render()
        assert np.array_equal(bits(host.download()), bits(img)) and np.array_equal(host.download_u8(), u8)
        assert host.stats() == stats and host.kernel_launches > launches
        host.render_async()  # a layers call behind a frame in flight on the host's stream
        again = host.render_layers(("value", "hit"))
        host.sync()
        assert np.array_equal(bits(again["value"]), bits(img)) and np.array_equal(bits(host.download()), bits(img))
    finally:
        host.close()


def test_torch_path_equals_numpy_path():
    """as_torch=True, on the default stream and under a stream of the caller's == the numpy path (tests/layers_torch_driver.py,
    a child process that brings torch's runtime up before it loads the library)."""
    driver = os.path.join(os.path.dirname(os.path.abspath(__file__)), "layers_torch_driver.py")
    r = subprocess.run([sys.executable, driver], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "LAYERS_TORCH_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_errors(rt, scene_for):
    E_INVALID, E_STATE = rt.api.RT_E_INVALID, rt.api.RT_E_STATE
    lib = rt.load_library()
    scene, _ = scene_for("blob", "longest")
    opt = rt.Options.defaults(width=32, height=24, n_super_samples=1, ao_num_samples=2)
    host = rt.Host(opt, 0)
    with pytest.raises(rt.RtError) as e:  # before the upload
        host.render_layers()
    assert e.value.code == E_STATE
    empty = rt.api._LayerArrays()
    assert lib.rt_render_layers_device(host._h, C.byref(empty), None) == E_STATE
    host.upload_scene(scene)
    assert lib.rt_render_layers(host._h, None) == E_INVALID  # a NULL `out`
    assert lib.rt_render_layers_device(host._h, None, None) == E_INVALID
    assert lib.rt_render_layers(None, C.byref(empty)) == E_INVALID
    # a misaligned device pointer is refused before anything is enqueued (the address is never used)
    for field in ("distance", "leaf", "barycentric", "position", "normal", "direction", "shade", "ao", "value"):
        assert lib.rt_render_layers_device(host._h, C.byref(rt.api._LayerArrays(**{field: 0x1002})), None) == E_INVALID, field
    assert "4-byte aligned" in lib.rt_last_error().decode()
    assert host.render_layers(("hit",))["hit"].any()
    host.close()
    # ambient occlusion off: no `ao`; everything else, and value == shade
    off = rt.Host(rt.Options.defaults(width=32, height=24, n_super_samples=1, ao_num_samples=0, enable_ao=0), 0)
    off.upload_scene(scene)
    with pytest.raises(rt.RtError) as e:
        off.render_layers()
    assert e.value.code == E_STATE and "ambient occlusion off" in e.value.message
    got = off.render_layers(tuple(n for n in rt.LAYER_OUTPUTS if n != "ao"))
    assert np.array_equal(bits(got["value"]), bits(got["shade"])) and got["hit"].any()
    off.close()
    # a band-partitioned host renders a part of the image only
    for rank in range(2):
        part = rt.Host(opt, 0, rank, 2)
        part.upload_scene(scene)
        with pytest.raises(rt.RtError) as e:
            part.render_layers(("hit",))
        assert e.value.code == E_STATE and "band-partitioned" in e.value.message
        part.close()
    # the hosts of a ring
    ring = rt.FrameRing(opt, scene, device=0, hosts=2)
    with pytest.raises(rt.RtError) as e:
        ring.host(0).render_layers(("hit",))
    assert e.value.code == E_STATE and "frame ring" in e.value.message
    ring.close()
    # more sub-pixels than an ambient-occlusion query takes points: 1920 x 1080 x 71 rays > RT_QUERY_MAX_RAYS
    big = rt.Host(rt.Options.defaults(width=1920, height=1080, n_super_samples=1, ao_num_samples=5), 0)
    big.upload_scene(scene)
    assert big.ao_rays_per_point[0] == 71 and 1920 * 1080 * 71 > 1 << 27
    for names in (("ao",), ("value",)):
        with pytest.raises(rt.RtError) as e:
            big.render_layers(names)
        assert e.value.code == E_INVALID and "RT_QUERY_MAX_RAYS" in e.value.message
    assert big.render_layers(("hit",))["hit"].any()  # (the other layers have no such limit)
    big.close()
