"""GPU: directional occlusion queries (include/rt_hip_directional.h) -- UNIFORM word for word against the CPU oracle of
tests/directional_oracle.c; RANDOM, and UNIFORM again, exact on the GPU's own terms: the masks against occlusion queries over
the rays rt_ao_rays writes, the counts and values against rt_trace_ao, the sums against the ordered float32 sum in numpy."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ao_direction_cases as adc
import directional_oracle as dro
import orc
import query_oracle as qo
from conftest import bits, options_for
from test_ao_query_gpu import _DeviceBytes, camera_hits, odd_points

pytestmark = pytest.mark.gpu

W, H = 64, 48
GOLDEN_CASES = ["bunny_64_s1_a3", "ties_33_s1_a3", "blob_40x24_s4_a2_d03_f08", "blob_80_s1_a5_noshade"]
FIELDS = ("mask", "occluded", "ao", "bent")


def make_host(rt, scene, **over):
    base = dict(width=W, height=H, n_super_samples=1, ao_num_samples=3, ao_max_distance=0.2)
    base.update(over)
    opt = rt.Options.defaults(**base)
    host = rt.Host(opt, 0)
    host.upload_scene(scene)
    return host, opt


def assert_same(got, want, what="", fields=FIELDS):
    for f in fields:
        assert got[f].shape == want[f].shape and got[f].dtype == want[f].dtype, (what, f, got[f].shape, want[f].shape)
        same = qo.same_words(got[f], want[f])
        assert same.all(), (what, f, int((~same).sum()), np.argwhere(~same)[:5].tolist())


def assert_rays(rays, want, what=""):
    """Host.ao_rays against the oracle's origins and directions (.w is 0)."""
    n, R = want["directions"].shape[:2]
    assert rays["origins"].shape == (n, 4) and rays["directions"].shape == (n, R, 4), what
    assert not rays["origins"][:, 3].any() and not rays["directions"][:, :, 3].any(), what
    assert qo.same_words(rays["origins"][:, :3], want["origins"]).all(), what
    same = qo.same_words(rays["directions"][:, :, :3], want["directions"])
    assert same.all(), (what, int((~same).sum()), np.argwhere(~same)[:5].tolist())


def check_on_gpu_terms(rt, host, opt, points, normals, seeds, got, what=""):
    """The three checks that need no oracle: counts and values are ambient_occlusion's, every mask bit is the occlusion query of
    that ray, the sum is the ordered float32 sum of the open rays' directions."""
    n, (R, _) = len(points), host.ao_rays_per_point
    ao = host.ambient_occlusion(points, normals, seeds=seeds)
    assert np.array_equal(got["occluded"], ao["occluded"]), what
    assert qo.same_words(got["ao"], ao["ao"]).all(), what
    rays = host.ao_rays(points, normals, seeds=seeds)
    assert rays["origins"].shape == (n, 4) and rays["directions"].shape == (n, R, 4)
    hit = host.trace_occluded(np.repeat(rays["origins"], R, axis=0), rays["directions"].reshape(n * R, 4),
                              max_distance=float(opt.ao_max_distance), sort=False).reshape(n, R).astype(bool)
    flags = rt.unpack_ao_mask(got["mask"], R)
    assert np.array_equal(flags, hit), (what, np.argwhere(flags != hit)[:5].tolist())
    same = qo.same_words(got["bent"], dro.ordered_sum(rays["directions"], ~hit))
    assert same.all(), (what, "bent", int((~same).sum()), np.argwhere(~same)[:5].tolist())
    return rays


@pytest.mark.parametrize("bvh", ["longest", "sah"])
@pytest.mark.parametrize("name", GOLDEN_CASES + ["blob_25x17"])
def test_uniform_matches_oracle(rt, golden, scene_for, name, bvh):
    if name == "blob_25x17":
        scene, arrays = scene_for("blob", bvh)
        host, opt = make_host(rt, scene)
        camera = orc.params_from_options(rt.Options.defaults(width=25, height=17, n_super_samples=1))
    else:
        c = golden["renders"][name]
        scene, arrays = scene_for(c["mesh"], bvh)
        opt = options_for(rt, c)
        host = rt.Host(opt, 0)
        host.upload_scene(scene)
        camera = orc.params_from_options(opt)  # the case's own sub-pixels
    cam = host.trace_closest(*qo.camera_rays(camera))
    hit = cam["hit"].astype(bool)
    index = np.flatnonzero(hit).astype(np.uint32)
    assert hit.any()
    points, normals = cam["position"][hit], cam["normal"][hit]
    want = dro.directional(orc.params_from_options(opt), arrays, points, normals, seeds=index)
    R = want["rays"]
    assert host.ao_rays_per_point == (R, R) and host.ao_mask_words == (R + 31) // 32
    got = host.directional_occlusion(points, normals, seeds=index)
    assert set(got) == set(FIELDS)
    assert_same(got, want, (name, bvh))
    assert ((want["occluded"] > 0) & (want["occluded"] < R)).any()
    rays = check_on_gpu_terms(rt, host, opt, points, normals, index, got, (name, bvh))
    assert_rays(rays, want, (name, bvh))
    host.close()


COUNTS = {"d4": 4, "d14": 14, "d28": 28, "d71": 71, "d79_alpha": 79, "d262": 262}


@pytest.mark.parametrize("case", sorted(COUNTS))
def test_direction_counts_and_point_counts(rt, scene_for, case):
    """Rows below a word with several points per packet, rows that straddle words and packets; point counts that make
    n x R a multiple of 64 and not."""
    scene, arrays = scene_for("blob", "longest")
    rung = adc.rung(3, 28) if case == "d28" else adc.SMALL[case]
    assert rung.dirs == COUNTS[case]
    host, opt = make_host(rt, scene, ao_num_samples=rung.rings, ao_alpha_min=rung.amin, ao_alpha_max=rung.amax, ao_max_distance=rung.aod)
    R = rung.dirs
    assert host.ao_rays_per_point == (R, R) and host.ao_mask_words == (R + 31) // 32
    _, cam, hit, _ = camera_hits(rt, host)
    points, normals = cam["position"][hit], cam["normal"][hit]
    everything = len(points)
    assert everything > 65
    want = dro.directional(orc.params_from_options(opt), arrays, points, normals)
    assert want["rays"] == R and want["occluded"].any()
    for n in (1, 2, 63, 64, 65, everything):
        got = host.directional_occlusion(points[:n], normals[:n])
        assert_same(got, {f: want[f][:n] for f in FIELDS}, (case, n))
        if R & 31:  # the bits from R upwards
            assert not (got["mask"][:, -1] >> np.uint32(R & 31)).any(), (case, n)
    rays = check_on_gpu_terms(rt, host, opt, points[:65], normals[:65], None, host.directional_occlusion(points[:65], normals[:65]), case)
    assert_rays(rays, {f: want[f][:65] for f in ("origins", "directions")}, case)
    host.close()


@pytest.mark.parametrize("mesh", ["blob", "ties"])
def test_odd_inputs(rt, scene_for, mesh):
    scene, arrays = scene_for(mesh, "longest")
    host, opt = make_host(rt, scene, ao_max_distance=1.0 if mesh == "ties" else 0.2)
    _, cam, hit, _ = camera_hits(rt, host)
    points, normals = odd_points(arrays, cam["position"][hit], cam["normal"][hit])
    want = dro.directional(orc.params_from_options(opt), arrays, points, normals)
    assert want["occluded"].any() and (want["occluded"] == 0).any() and np.isnan(want["bent"]).any()
    for sort in (True, False):
        got = host.directional_occlusion(points, normals, sort=sort)
        assert_same(got, want, (mesh, sort))
    rays = check_on_gpu_terms(rt, host, opt, points, normals, None, got, mesh)
    assert_rays(rays, want, mesh)
    host.close()


@pytest.mark.parametrize("samples", [8, 30, 31, 62, 63])
def test_random_is_exact_on_the_gpu(rt, scene_for, samples):
    """R = samples + 2 = 10, 32, 33, 64, 65: a row that ends with its word, one bit into the next, with the packet, one ray
    into the next."""
    scene, _ = scene_for("blob", "longest")
    host, opt = make_host(rt, scene, ao_method=1, ao_num_samples=samples)
    R = samples + 2
    assert host.ao_rays_per_point == (R, samples + 1) and host.ao_mask_words == (R + 31) // 32
    _, cam, hit, index = camera_hits(rt, host)
    points, normals = cam["position"][hit], cam["normal"][hit]
    n = len(points)
    defaulted = host.directional_occlusion(points, normals)
    assert_same(defaulted, host.directional_occlusion(points, normals, seeds=np.arange(n, dtype=np.uint32)), "arange")
    assert_same(defaulted, host.directional_occlusion(points, normals, sort=False), "unsorted")
    for seeds in (index, None):
        got = defaulted if seeds is None else host.directional_occlusion(points, normals, seeds=seeds)
        assert got["occluded"].any() and (got["occluded"] < R).any()
        assert np.array_equal(dro.popcount(got["mask"]), got["occluded"])
        if R & 31:
            assert not (got["mask"][:, -1] >> np.uint32(R & 31)).any()
        rays = check_on_gpu_terms(rt, host, opt, points, normals, seeds, got, (samples, seeds is None))
        # ray 0 is the normal as given, the others are unit vectors
        assert np.array_equal(bits(rays["directions"][:, 0, :3]), bits(normals))
        assert np.allclose(np.linalg.norm(rays["directions"][:, 1:, :3].astype(np.float64), axis=2), 1.0, atol=1e-5)
    assert not np.array_equal(host.directional_occlusion(points, normals, seeds=index)["mask"], defaulted["mask"])
    host.close()


def test_rows_words_and_order(rt, scene_for):
    """Sorted, unsorted and shuffled calls give identical words; single outputs are the full call's; a call that asks for
    nothing, and one with no points, launch nothing."""
    scene, arrays = scene_for("bunny", "longest")
    host, opt = make_host(rt, scene)
    _, cam, hit, _ = camera_hits(rt, host, 96, 72)
    points, normals = cam["position"][hit], cam["normal"][hit]
    n = len(points)
    assert n * 28 >= 16384  # RT_QUERY_SORT_MIN: the sort runs
    a = host.directional_occlusion(points, normals, sort=True)
    assert_same(a, host.directional_occlusion(points, normals, sort=False), "sorted / unsorted")
    assert_same(a, dro.directional(orc.params_from_options(opt), arrays, points, normals), "oracle")
    assert not (a["mask"] >> np.uint32(28)).any()
    perm = np.random.default_rng(5).permutation(n)
    for sort in (True, False):
        c = host.directional_occlusion(points[perm], normals[perm], sort=sort)
        assert_same(c, {f: a[f][perm] for f in FIELDS}, ("shuffled", sort))
    for f in FIELDS:
        one = host.directional_occlusion(points, normals, outputs=(f,))
        assert set(one) == {f}
        assert_same(one, a, ("alone", f), (f,))
    assert_same(host.directional_occlusion(points, normals, outputs=("bent", "ao")), a, "two", ("bent", "ao"))
    ms = host.last_query_ms
    assert ms > 0.0
    # nothing asked for, no points: nothing is launched, the last query's time stands
    assert host.directional_occlusion(points, normals, outputs=()) == {}
    lib = rt.load_library()
    p4, n4 = qo.as4(points), qo.as4(normals)
    nothing = rt.api._DirectionalArrays(None, None, None, None)
    assert lib.rt_trace_ao_directional(host._h, p4.ctypes.data, n4.ctypes.data, None, n, 0, C.byref(nothing)) == 0
    assert lib.rt_trace_ao_directional(host._h, p4.ctypes.data, n4.ctypes.data, None, n, 0, None) == 0
    assert lib.rt_ao_rays(host._h, p4.ctypes.data, n4.ctypes.data, None, n, None, None) == 0
    empty = host.directional_occlusion(points[:0], normals[:0])
    assert empty["mask"].shape == (0, 1) and empty["bent"].shape == (0, 3) and empty["ao"].shape == (0,)
    none = host.ao_rays(points[:0], normals[:0])
    assert none["origins"].shape == (0, 4) and none["directions"].shape == (0, 28, 4)
    assert host.last_query_ms == ms
    host.close()


def test_device_memory_form_equals_host_memory_form():
    """Device tensors in and out on a non-default stream == the numpy path (tests/directional_torch_driver.py, a child
    process that brings torch's runtime up before it loads the library)."""
    driver = os.path.join(os.path.dirname(os.path.abspath(__file__)), "directional_torch_driver.py")
    r = subprocess.run([sys.executable, driver], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DIRECTIONAL_TORCH_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_vertex_bent_normals(rt, scene_for):
    scene, arrays = scene_for("blob", "longest")
    host, opt = make_host(rt, scene)
    got = host.vertex_bent_normals(scene)
    assert got.shape == (scene.num_vertices, 3) and got.dtype == np.float32
    want = dro.directional(orc.params_from_options(opt), arrays, scene.vertices, scene.vnormals)
    assert qo.same_words(got, want["bent"]).all()
    assert qo.same_words(host.vertex_ao(scene), want["ao"]).all() and (want["occluded"] > 0).any()
    host.close()


def test_error_paths(rt, scene_for):
    lib = rt.load_library()
    E_STATE, E_INVALID = rt.api.RT_E_STATE, rt.api.RT_E_INVALID
    scene, _ = scene_for("blob", "longest")
    pts = np.zeros((4, 3), np.float32)
    p4 = qo.as4(pts)
    words = C.c_uint32()
    out4 = (np.zeros(4, np.float32), np.zeros(4, np.uint32), np.zeros((4, 1), np.uint32), np.zeros((4, 3), np.float32))
    arrays = rt.api._DirectionalArrays(*[a.ctypes.data for a in out4])

    def all_refuse(host, code):
        for call in (lambda: host.directional_occlusion(pts, pts), lambda: host.ao_rays(pts, pts), lambda: host.ao_mask_words):
            with pytest.raises(rt.RtError) as e:
                call()
            assert e.value.code == code
        assert lib.rt_ao_mask_words(host._h, C.byref(words)) == code
        assert lib.rt_trace_ao_directional(host._h, p4.ctypes.data, p4.ctypes.data, None, 4, 0, C.byref(arrays)) == code
        assert lib.rt_trace_ao_directional_device(host._h, None, None, None, 0, 0, None, None) == code
        assert lib.rt_ao_rays(host._h, p4.ctypes.data, p4.ctypes.data, None, 4, None, None) == code
        assert lib.rt_ao_rays_device(host._h, None, None, None, 0, None, None, None) == code

    # before an upload
    host = rt.Host(rt.Options.defaults(width=W, height=H, ao_num_samples=3), 0)
    all_refuse(host, E_STATE)
    host.upload_scene(scene)
    assert host.ao_mask_words == 1 and lib.rt_ao_mask_words(host._h, None) == 0
    # null points or normals with n > 0; n == 0 succeeds
    for points, normals in ((None, None), (p4.ctypes.data, None), (None, p4.ctypes.data)):
        assert lib.rt_trace_ao_directional(host._h, points, normals, None, 4, 0, C.byref(arrays)) == E_INVALID
        assert lib.rt_trace_ao_directional_device(host._h, points, normals, None, 4, 0, C.byref(arrays), None) == E_INVALID
        assert lib.rt_ao_rays(host._h, points, normals, None, 4, None, None) == E_INVALID
        assert lib.rt_ao_rays_device(host._h, points, normals, None, 4, None, None, None) == E_INVALID
    assert lib.rt_trace_ao_directional(host._h, None, None, None, 0, 0, C.byref(arrays)) == 0
    assert lib.rt_trace_ao_directional_device(host._h, None, None, None, 0, 0, None, None) == 0
    assert lib.rt_ao_rays(host._h, None, None, None, 0, None, None) == 0
    assert lib.rt_ao_rays_device(host._h, None, None, None, 0, None, None, None) == 0
    # n above RT_QUERY_MAX_RAYS / R
    limit = (1 << 27) // 28
    assert lib.rt_trace_ao_directional(host._h, p4.ctypes.data, p4.ctypes.data, None, limit + 1, 0, None) == E_INVALID
    assert lib.rt_ao_rays(host._h, p4.ctypes.data, p4.ctypes.data, None, limit + 1, None, None) == E_INVALID
    # alignment of device pointers
    n = 64
    mem = _DeviceBytes(2 * 65 * 16 + 65 * 16 + 65 * 28 * 16 + 8 * 65 * 4 + 64)
    vec = mem.ptr.value
    nrm, org, dirs = vec + 65 * 16, vec + 2 * 65 * 16, vec + 3 * 65 * 16
    out = dirs + 65 * 28 * 16
    good = dict(ao=out, occluded=out + 65 * 4, mask=out + 2 * 65 * 4, bent=out + 3 * 65 * 4)

    def directional_device(points=vec, normals=nrm, seeds=None, **change):
        a = rt.api._DirectionalArrays(**{**good, **change})
        return lib.rt_trace_ao_directional_device(host._h, points, normals, seeds, n, 0, C.byref(a), None)

    assert directional_device(points=vec + 4) == E_INVALID and directional_device(normals=nrm + 8) == E_INVALID
    for name in good:
        assert directional_device(**{name: good[name] + 2}) == E_INVALID, name
    assert directional_device(seeds=out + 6 * 65 * 4 + 1) == E_INVALID
    assert lib.rt_ao_rays_device(host._h, vec + 4, nrm, None, n, org, dirs, None) == E_INVALID
    assert lib.rt_ao_rays_device(host._h, vec, nrm + 8, None, n, org, dirs, None) == E_INVALID
    assert lib.rt_ao_rays_device(host._h, vec, nrm, None, n, org + 4, dirs, None) == E_INVALID
    assert lib.rt_ao_rays_device(host._h, vec, nrm, None, n, org, dirs + 8, None) == E_INVALID
    assert lib.rt_ao_rays_device(host._h, vec, nrm, out + 6 * 65 * 4 + 2, n, org, dirs, None) == E_INVALID
    assert directional_device(seeds=out + 6 * 65 * 4) == 0
    assert lib.rt_ao_rays_device(host._h, vec, nrm, out + 6 * 65 * 4, n, org, dirs, None) == 0
    host.sync()
    # the binding's own refusals
    with pytest.raises(ValueError):
        host.directional_occlusion(pts, pts, outputs=("hit",))
    with pytest.raises(ValueError):
        host.directional_occlusion(pts, pts, seeds=np.zeros(3, np.uint32))
    host.close()
    mem.free()
    # ambient occlusion off: no direction table on the device
    for off in (dict(enable_ao=0), dict(ao_num_samples=0)):
        host = rt.Host(rt.Options.defaults(width=W, height=H, **{"ao_num_samples": 3, **off}), 0)
        host.upload_scene(scene)
        all_refuse(host, E_STATE)
        host.close()
    # the hosts of a frame ring
    ring = rt.FrameRing(rt.Options.defaults(width=32, height=32, ao_num_samples=3), hosts=2)
    ring.set_calibration(False)
    ring.upload_scene(scene)
    all_refuse(ring.host(0), E_STATE)
    ring.close()


def test_directional_queries_leave_frames_alone(rt, oracle, scene_for):
    scene, arrays = scene_for("bunny", "longest")
    opt = rt.Options.defaults(width=96, height=64, n_super_samples=4, ao_num_samples=3)
    host = rt.Host(opt, 0)
    host.upload_scene(scene)
    host.render()
    frame, u8 = host.download().tobytes(), host.download_u8().tobytes()
    stats = host.stats()
    _, cam, hit, _ = camera_hits(rt, host)
    points, normals = cam["position"][hit], cam["normal"][hit]
    ao_before = host.ambient_occlusion(points, normals)
    before = host.directional_occlusion(points, normals)
    rays = host.ao_rays(points, normals)
    assert host.stats() == stats
    host.render()
    assert host.download().tobytes() == frame and host.download_u8().tobytes() == u8
    host.render_async()  # a frame left in flight while the queries run
    during = host.directional_occlusion(points, normals)
    rays_during = host.ao_rays(points, normals)
    host.sync()
    assert host.download().tobytes() == frame and host.download_u8().tobytes() == u8
    assert host.stats() == stats
    assert_same(before, during)
    assert np.array_equal(bits(rays["directions"]), bits(rays_during["directions"]))
    ao_after = host.ambient_occlusion(points, normals)
    for f in ("ao", "occluded"):
        assert qo.same_words(ao_before[f], ao_after[f]).all() and qo.same_words(ao_before[f], before[f]).all()
    assert host.last_query_ms > 0.0
    host.close()
