"""GPU: ambient-occlusion queries (include/rt_hip_ao.h) against the CPU oracle of tests/ao_oracle.c -- UNIFORM word for
word, RANDOM within the frames' own criterion."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ao_oracle as aoo
import multihit_oracle as mo
import orc
import query_oracle as qo
from conftest import bits

pytestmark = pytest.mark.gpu

W, H = 64, 48


def options(rt, **over):
    base = dict(width=W, height=H, n_super_samples=1, ao_num_samples=3, ao_max_distance=0.2)
    base.update(over)
    return rt.Options.defaults(**base)


def make_host(rt, scene, **over):
    opt = options(rt, **over)
    host = rt.Host(opt, 0)
    host.upload_scene(scene)
    return host, opt


def camera_hits(rt, host, w=W, h=H):
    """The closest hits of the w x h reference camera through the host's own ray queries: (rays, result, hit mask, the
    sub-pixels' indices y * w + x)."""
    p = orc.params_from_options(rt.Options.defaults(width=w, height=h, n_super_samples=1))
    o4, d4 = qo.camera_rays(p)
    cam = host.trace_closest(o4, d4)
    hit = cam["hit"].astype(bool)
    return d4, cam, hit, np.flatnonzero(hit).astype(np.uint32)


def assert_same(got, want, what=""):
    for f in ("ao", "occluded"):
        same = qo.same_words(got[f], want[f])
        assert same.all(), (what, f, int((~same).sum()), np.argwhere(~same)[:5].tolist())


@pytest.mark.parametrize("bvh", ["longest", "sah"])
@pytest.mark.parametrize("mesh", ["bunny", "blob", "ties", "single"])
def test_uniform_matches_oracle_and_frame(rt, scene_for, mesh, bvh):
    scene, arrays = scene_for(mesh, bvh)
    host, opt = make_host(rt, scene, ao_max_distance=1.0 if mesh == "ties" else 0.2)
    p = orc.params_from_options(opt)
    assert host.ao_rays_per_point == (28, 28)
    d4, cam, hit, index = camera_hits(rt, host)
    assert hit.any()
    points, normals = cam["position"][hit], cam["normal"][hit]
    got = host.ambient_occlusion(points, normals, seeds=index)
    assert got["ao"].dtype == np.float32 and got["occluded"].dtype == np.uint32 and got["ao"].shape == (len(index),)
    want = aoo.ambient_occlusion(p, arrays, points, normals, seeds=index)
    assert want["rays"] == 28
    assert_same(got, want, (mesh, bvh))
    # one output at a time
    assert np.array_equal(bits(host.ambient_occlusion(points, normals, outputs=("ao",))["ao"]), bits(want["ao"]))
    assert np.array_equal(host.ambient_occlusion(points, normals, outputs=("occluded",))["occluded"], want["occluded"])
    # query and frame agree: shade x ao is the frame's own float image
    host.render()
    img = host.download()
    value = qo.shade(cam["hit"], cam["normal"], d4, True)
    value[hit] = value[hit] * got["ao"]
    assert np.array_equal(bits(value.reshape(img.shape)), bits(img))
    assert host.stats()["ao_occluded"] == int(got["occluded"].sum(dtype=np.uint64))
    host.close()


@pytest.mark.parametrize("samples,amin,amax,rays", [(1, 4, 90, 4), (2, 4, 90, 14), (5, 4, 90, 71), (4, 10, 60, 79)])
def test_packet_edges(rt, scene_for, samples, amin, amax, rays):
    """Direction counts that straddle a wave, point counts that make n x rays a multiple of 64 and not."""
    scene, arrays = scene_for("blob", "longest")
    host, opt = make_host(rt, scene, ao_num_samples=samples, ao_alpha_min=amin, ao_alpha_max=amax)
    assert host.ao_rays_per_point == (rays, rays)
    _, cam, hit, _ = camera_hits(rt, host)
    points, normals = np.resize(cam["position"][hit], (1000, 3)), np.resize(cam["normal"][hit], (1000, 3))
    want = aoo.ambient_occlusion(orc.params_from_options(opt), arrays, points, normals)
    assert want["rays"] == rays
    for n in (0, 1, 2, 63, 64, 65, 1000):
        got = host.ambient_occlusion(points[:n], normals[:n])
        assert got["ao"].shape == (n,) and got["occluded"].shape == (n,)
        assert_same(got, {k: want[k][:n] for k in ("ao", "occluded")}, n)
    host.close()


def test_order(rt, scene_for):
    """Sorted and unsorted calls give identical words; a shuffled copy of the points gives the shuffled results."""
    scene, arrays = scene_for("bunny", "longest")
    host, opt = make_host(rt, scene)
    _, cam, hit, _ = camera_hits(rt, host, 96, 72)
    points, normals = cam["position"][hit], cam["normal"][hit]
    n = len(points)
    assert n >= 2000 and n * 28 >= 16384
    a = host.ambient_occlusion(points, normals, sort=True)
    b = host.ambient_occlusion(points, normals, sort=False)
    assert_same(a, b, "sorted / unsorted")
    assert_same(a, aoo.ambient_occlusion(orc.params_from_options(opt), arrays, points, normals), "oracle")
    perm = np.random.default_rng(5).permutation(n)
    for sort in (True, False):
        c = host.ambient_occlusion(points[perm], normals[perm], sort=sort)
        assert_same(c, {k: a[k][perm] for k in ("ao", "occluded")}, ("shuffled", sort))
    assert host.last_query_ms > 0.0
    host.close()


def odd_points(arrays, points, normals, n=2000):
    points, normals = np.resize(points, (n, 3)).copy(), np.resize(normals, (n, 3)).copy()
    k = np.arange(n)
    normals[k % 7 == 0] = 0.0                                  # zero normals
    normals[k % 11 == 0, 1] = -0.0                             # a zero component
    normals[k % 13 == 0] *= np.float32(37.0)                   # not unit
    normals[k % 17 == 0] *= np.float32(1e-30)                  # tiny (denormal products)
    normals[k % 19 == 0, 2] = np.float32(1e-41)                # a denormal component
    normals[k % 23 == 0] *= np.float32(1e30)                   # huge (the squared length overflows)
    lo, hi = arrays.aabbs[0, :3].astype(np.float64), arrays.aabbs[1, :3].astype(np.float64)
    far = np.float32(float(np.max(hi - lo)) * 50)
    points[k % 29 == 0, 0] += far                              # 50 boxes away
    points[k % 31 == 0] -= far
    points[k % 37 == 0] = np.float32(3e38)
    points[k % 41 == 0, 1] = np.nan
    normals[k % 43 == 0, 2] = np.nan
    points[k % 47 == 0, 0] = np.inf
    normals[k % 53 == 0, 0] = -np.inf
    points[k % 59 == 0, 2] = -np.inf
    return points.astype(np.float32), normals.astype(np.float32)


@pytest.mark.parametrize("mesh", ["blob", "ties"])
def test_odd_inputs(rt, scene_for, mesh):
    scene, arrays = scene_for(mesh, "longest")
    host, opt = make_host(rt, scene, ao_max_distance=1.0 if mesh == "ties" else 0.2)
    _, cam, hit, _ = camera_hits(rt, host)
    points, normals = odd_points(arrays, cam["position"][hit], cam["normal"][hit])
    want = aoo.ambient_occlusion(orc.params_from_options(opt), arrays, points, normals)
    assert want["occluded"].any() and (want["occluded"] == 0).any()
    for sort in (True, False):
        assert_same(host.ambient_occlusion(points, normals, sort=sort), want, (mesh, sort))
    host.close()


# RANDOM: the share of points whose `occluded` differs from the CPU oracle's (device libm against the host's: a ray that
# grazes an edge flips between hit and miss).  Measured on one MI355X (ROCm 7.2) for the four cases below -- the values
# and how the bound follows from them stand in DESIGN.md section 11 and profiles/ao_query_notes.md:
RANDOM_MEASURED_SHARES = {("blob", 8): 0.0, ("blob", 32): 0.0, ("bunny", 8): 0.0, ("bunny", 32): 0.0}
RANDOM_SHARE_BOUND = 2.0 * max(RANDOM_MEASURED_SHARES.values())  # twice the largest measured share


@pytest.mark.parametrize("samples", [8, 32])
@pytest.mark.parametrize("mesh", ["blob", "bunny"])
def test_random(rt, scene_for, mesh, samples):
    scene, arrays = scene_for(mesh, "longest")
    host, opt = make_host(rt, scene, ao_method=1, ao_num_samples=samples)
    assert host.ao_rays_per_point == (samples + 2, samples + 1)
    _, cam, hit, index = camera_hits(rt, host)
    points, normals = cam["position"][hit], cam["normal"][hit]
    n = len(points)
    # defaulted seeds are 0 .. n-1
    defaulted = host.ambient_occlusion(points, normals)
    assert_same(defaulted, host.ambient_occlusion(points, normals, seeds=np.arange(n, dtype=np.uint32)), "arange")
    assert_same(defaulted, host.ambient_occlusion(points, normals, sort=False), "unsorted")
    p = orc.params_from_options(opt)
    for seeds in (index, None):
        got = host.ambient_occlusion(points, normals, seeds=seeds)
        want = aoo.ambient_occlusion(p, arrays, points, normals, seeds=seeds)
        assert want["rays"] == samples + 2 and want["occluded"].any()
        delta = np.abs(got["ao"].astype(np.float64) - want["ao"].astype(np.float64))
        share = float((got["occluded"] != want["occluded"]).mean())
        print(f"AO_RANDOM_MEASURE mesh={mesh} samples={samples} seeds={'given' if seeds is not None else 'default'} n={n} "
              f"mean_abs_delta_ao={delta.mean():.6g} differing_share={share:.6g} "
              f"max_hits_delta={int(np.abs(got['occluded'].astype(np.int64) - want['occluded'].astype(np.int64)).max())}")
        assert delta.mean() <= 0.25 / 255.0, delta.mean()
        assert share <= 0.10, share  # (gross: a defect, whatever the bound says)
        assert share <= RANDOM_SHARE_BOUND, (share, RANDOM_SHARE_BOUND)
        # the values follow from the counts exactly
        assert np.array_equal(bits(got["ao"]), bits(np.float32(1.0) - got["occluded"].astype(np.float32) / np.float32(samples + 1)))
    host.close()


def test_torch_path_equals_numpy_path():
    """Device tensors in and out on a non-default stream == the numpy path (tests/ao_query_torch_driver.py, a child process
    that brings torch's runtime up before it loads the library)."""
    driver = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ao_query_torch_driver.py")
    r = subprocess.run([sys.executable, driver], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "AO_QUERY_TORCH_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_ao_queries_leave_frames_alone(rt, oracle, scene_for):
    scene, arrays = scene_for("bunny", "longest")
    opt = rt.Options.defaults(width=96, height=64, n_super_samples=4, ao_num_samples=3)
    ref_img, counters, _ = oracle.render(orc.params_from_options(opt), arrays)
    host = rt.Host(opt, 0)
    host.upload_scene(scene)
    host.render()
    assert np.array_equal(bits(host.download()), bits(ref_img))
    stats = host.stats()
    _, cam, hit, _ = camera_hits(rt, host)
    points, normals = cam["position"][hit], cam["normal"][hit]
    before = host.ambient_occlusion(points, normals)
    assert host.stats() == stats
    host.render()
    assert np.array_equal(bits(host.download()), bits(ref_img))
    host.render_async()  # a frame left in flight while a query runs
    during = host.ambient_occlusion(points, normals)
    host.sync()
    assert np.array_equal(bits(host.download()), bits(ref_img))
    assert host.stats() == stats
    assert host.stats()["ao_occluded"] == counters["ao_occluded"]
    assert_same(before, during)
    assert host.last_query_ms > 0.0
    host.close()


def test_interleaved_families_share_one_host(rt, scene_for):
    """Closest-hit, occlusion, multi-hit and AO queries in turn on ONE host, sorted and unsorted, with fewer and with more
    items than the call before: the families share the sort's scratch, the staging buffer and the events, so what one call
    leaves behind (an order for more items, a histogram, a staging layout for other outputs) must not reach the next.
    Every result is compared with its CPU oracle, computed once per ray set."""
    scene, arrays = scene_for("blob", "longest")
    host, opt = make_host(rt, scene)
    assert host.ao_rays_per_point == (28, 28)
    md = 100000.0
    o, d = mo.random_rays(arrays, 16384 + 65, seed=17)  # RT_QUERY_SORT_MIN and a partial last packet
    cam_o, cam_d = qo.camera_rays(orc.params_from_options(rt.Options.defaults(width=W, height=H, n_super_samples=1)))
    cam = qo.closest(arrays, cam_o, cam_d, md)
    on = cam["hit"].astype(bool)
    assert on.any()
    points, normals = np.resize(cam["position"][on], (600, 3)), np.resize(cam["normal"][on], (600, 3))  # 600 x 28 >= 16384
    want_closest, want_occluded = qo.closest(arrays, o, d, md), qo.occluded(arrays, o, d, md)
    want_multi = mo.multihit(arrays, o, d, md, mo.MAX_K)
    want_ao = aoo.ambient_occlusion(orc.params_from_options(opt), arrays, points, normals)
    assert want_closest["hit"].any() and want_ao["occluded"].any() and (want_multi["count"] > 1).any()

    def same(got, want, fields, what):
        assert set(got) == set(fields), (what, sorted(got))
        for f in fields:
            assert got[f].shape == want[f].shape, (what, f, got[f].shape, want[f].shape)
            words = qo.same_words(got[f], want[f])
            assert words.all(), (what, f, int((~words).sum()), np.argwhere(~words)[:5].tolist())

    def closest_then_ao(what):
        same(host.trace_closest(o, d, md, sort=True), want_closest, rt.api.QUERY_OUTPUTS, (what, "closest"))
        same(host.ambient_occlusion(points, normals, sort=True), want_ao, rt.api.AO_OUTPUTS, (what, "ao"))

    closest_then_ao("first")
    same(host.trace_multihit(o[:257], d[:257], md, k=4, sort=False), {f: v[:257] for f, v in mo.first_slots(want_multi, 4).items()},
         mo.FIELDS, "multihit k=4")
    same(host.ambient_occlusion(points[:65], normals[:65], outputs=("ao",), sort=False), {"ao": want_ao["ao"][:65]}, ("ao",), "ao alone")
    same({"hit": host.trace_occluded(o, d, md, sort=True)}, {"hit": want_occluded}, ("hit",), "occluded")
    same(host.trace_multihit(o, d, md, k=16, sort=True), mo.first_slots(want_multi, 16), mo.FIELDS, "multihit k=16")
    closest_then_ao("again")
    assert host.last_query_ms > 0.0
    host.close()


class _DeviceBytes:
    """Device memory straight from the HIP runtime the library uses (as in tests/test_query_gpu.py)."""

    def __init__(self, size):
        self.hip, self.ptr = C.CDLL("libamdhip64.so"), C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.ptr), C.c_size_t(size)) == 0
        assert self.hip.hipMemset(self.ptr, 0, C.c_size_t(size)) == 0

    def free(self):
        self.hip.hipFree(self.ptr)


def test_error_paths(rt, scene_for):
    lib = rt.load_library()
    scene, _ = scene_for("blob", "longest")
    pts = np.zeros((4, 3), np.float32)
    rays, divisor = C.c_uint32(), C.c_uint32()
    # before an upload
    host = rt.Host(options(rt), 0)
    with pytest.raises(rt.RtError) as e:
        host.ambient_occlusion(pts, pts)
    assert e.value.code == rt.api.RT_E_STATE
    assert lib.rt_ao_rays_per_point(host._h, C.byref(rays), C.byref(divisor)) == rt.api.RT_E_STATE
    host.upload_scene(scene)
    assert host.ao_rays_per_point == (28, 28)
    assert lib.rt_trace_ao(host._h, None, None, None, 4, 0, None, None) == rt.api.RT_E_INVALID
    assert lib.rt_trace_ao_device(host._h, None, None, None, 4, 0, None, None, None) == rt.api.RT_E_INVALID
    assert lib.rt_trace_ao(host._h, None, None, None, 0, 0, None, None) == 0
    limit = (1 << 27) // 28
    assert lib.rt_trace_ao(host._h, pts.ctypes.data, pts.ctypes.data, None, limit + 1, 0, None, None) == rt.api.RT_E_INVALID
    with pytest.raises(ValueError):
        host.ambient_occlusion(pts.astype(np.float64), pts)
    with pytest.raises(ValueError):
        host.ambient_occlusion(pts, pts, seeds=np.zeros(3, np.uint32))
    with pytest.raises(ValueError):
        host.ambient_occlusion(pts, pts, outputs=("hit",))
    mem = _DeviceBytes(2 * 65 * 16 + 3 * 65 * 4 + 64)
    vec, out = mem.ptr.value, mem.ptr.value + 2 * 65 * 16
    assert lib.rt_trace_ao_device(host._h, vec + 4, vec, None, 64, 0, out, None, None) == rt.api.RT_E_INVALID
    assert lib.rt_trace_ao_device(host._h, vec, vec + 8, None, 64, 0, out, None, None) == rt.api.RT_E_INVALID
    assert lib.rt_trace_ao_device(host._h, vec, vec + 16 * 65, None, 64, 0, out + 2, None, None) == rt.api.RT_E_INVALID
    assert lib.rt_trace_ao_device(host._h, vec, vec + 16 * 65, None, 64, 0, None, out + 1, None) == rt.api.RT_E_INVALID
    assert lib.rt_trace_ao_device(host._h, vec, vec + 16 * 65, out + 2, 64, 0, out + 65 * 4, None, None) == rt.api.RT_E_INVALID
    assert lib.rt_trace_ao_device(host._h, vec, vec + 16 * 65, None, 64, 0, out, out + 65 * 4, None) == 0
    host.sync()
    host.close()
    mem.free()
    # ambient occlusion off: no direction table on the device
    for off in (dict(enable_ao=0), dict(ao_num_samples=0)):
        host = rt.Host(options(rt, **off), 0)
        host.upload_scene(scene)
        with pytest.raises(rt.RtError) as e:
            host.ambient_occlusion(pts, pts)
        assert e.value.code == rt.api.RT_E_STATE
        assert lib.rt_ao_rays_per_point(host._h, C.byref(rays), C.byref(divisor)) == rt.api.RT_E_STATE
        host.close()
    # the hosts of a frame ring
    ring = rt.FrameRing(rt.Options.defaults(width=32, height=32, ao_num_samples=3), hosts=2)
    ring.set_calibration(False)
    ring.upload_scene(scene)
    with pytest.raises(rt.RtError) as e:
        ring.host(0).ambient_occlusion(pts, pts)
    assert e.value.code == rt.api.RT_E_STATE
    ring.close()


def test_vertex_ao(rt, scene_for):
    scene, arrays = scene_for("blob", "longest")
    host, opt = make_host(rt, scene)
    got = host.vertex_ao(scene)
    assert got.shape == (scene.num_vertices,) and got.dtype == np.float32
    want = aoo.ambient_occlusion(orc.params_from_options(opt), arrays, scene.vertices, scene.vnormals)
    assert qo.same_words(got, want["ao"]).all()
    assert (got < 1.0).any()
    host.close()
