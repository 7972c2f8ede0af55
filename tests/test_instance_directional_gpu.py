"""GPU: instanced directional occlusion queries (include/rt_hip_instance_directional.h) against their expected values BY
COMPOSITION (tests/instance_directional_oracle.py: the ambient-occlusion rays of the directional oracle, the instanced walk of
the instance oracle on the plan read back from the host, numpy for the packing, the ordered float32 sum), every output word
for word in UNIFORM mode; in RANDOM mode on the GPU's own terms -- trace_instances_occluded on the rays host.ao_rays() writes,
instances_ambient_occlusion's counts; and against directional_occlusion under one identity instance."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import directional_oracle as dro
import instance_cases as cases
import instance_directional_oracle as ido
import instance_views_oracle as ivo
import orc

pytestmark = pytest.mark.gpu

SORT_MIN = 16384  # RT_QUERY_SORT_MIN, in rays
SIZES = (1, 2, 3, 64, 65, 600)
# rays per point -> (ao_num_samples, ao_alpha_min, ao_alpha_max): one word; a row that straddles packets; a word that is not
# full; a word that ends with its row; three words
RUNGS = {4: (1, 4, 90), 14: (2, 4, 90), 28: (3, 4, 90), 32: (3, 10, 80), 71: (5, 4, 90)}
FIELDS = ido.OUTPUTS
EMPTY = np.zeros((0, 3, 4), np.float32)


def ao_host(rt, scene, rays=14, **over):
    rings, amin, amax = RUNGS[rays]
    opt = rt.Options.defaults(width=32, height=24, n_super_samples=1, ao_num_samples=rings, ao_alpha_min=amin, ao_alpha_max=amax,
                              ao_max_distance=over.pop("ao_max_distance", 0.5), **over)
    host = rt.Host(opt, 0)
    if scene is not None:
        host.upload_scene(scene)
        if not over.get("ao_method"):
            assert host.ao_rays_per_point == (rays, rays) and host.ao_mask_words == (rays + 31) // 32
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


def assert_same(got, want, what="", fields=FIELDS):
    for f in fields:
        assert got[f].shape == want[f].shape and got[f].dtype == want[f].dtype, (what, f, got[f].shape, want[f].shape, got[f].dtype)
        ok = ido.same_words(got[f], want[f])
        assert ok.all(), (what, f, int((~ok).sum()), np.argwhere(~ok)[:5].tolist())


def check(host, arrays, plan, points, normals, seeds=None, sort=True, rays=None, what=""):
    got = host.instances_directional_occlusion(points, normals, seeds, sort=sort)
    assert tuple(got) == FIELDS
    want = ido.directional(orc.params_from_options(host.options), arrays, plan, points, normals, seeds, rays)
    assert_same(got, want, (what, sort))
    R = host.ao_rays_per_point[0]
    if R & 31 and len(points):  # the bits from R upwards
        assert not (got["mask"][:, -1] >> np.uint32(R & 31)).any(), what
    return got


@pytest.mark.parametrize("rays", sorted(RUNGS))
def test_uniform_matches_the_composition(rt, scene_for, rays):
    scene, arrays = scene_for("blob", "sah" if rays % 2 else "longest")
    host = ao_host(rt, scene, rays)
    blocked = 0
    try:
        sets = (("rotations", cases.family("rotations", arrays)), ("tie_pair", cases.family("tie_pair", arrays)),
                ("many65", cases.many(arrays, 65, seed=3)), ("one", cases.many(arrays, 1, seed=3)))
        for k, (name, W) in enumerate(sets):
            host.set_instances(W)
            plan = host.instances()
            points, normals = surface_points(host, plan, max(SIZES), seed=31 + k)
            for n in SIZES:
                got = check(host, arrays, plan, points[:n], normals[:n], sort=bool((n + k) % 2), what=(rays, name, n))
                assert got["mask"].shape == (n, (rays + 31) // 32) and got["bent"].shape == (n, 3)
            blocked += int(got["occluded"].sum())
            # `occluded` and `ao` are instances_ambient_occlusion's, word for word
            ao = host.instances_ambient_occlusion(points, normals)
            assert np.array_equal(got["occluded"], ao["occluded"]) and ido.same_words(got["ao"], ao["ao"]).all(), (rays, name)
        assert blocked > 0 and host.last_query_ms > 0.0
        empty = host.instances_directional_occlusion(points[:0], normals[:0])
        assert empty["mask"].shape == (0, (rays + 31) // 32) and empty["bent"].shape == (0, 3)
    finally:
        host.close()


def test_both_sides_of_the_sort_threshold_and_shuffled_points(rt, scene_for):
    """14 rays a point: 1170 points make 16380 rays, 1171 make 16394 -- one call on each side of RT_QUERY_SORT_MIN; sorted,
    unsorted and a shuffled copy give the same words by point."""
    scene, arrays = scene_for("blob", "longest")
    host = ao_host(rt, scene)
    try:
        host.set_instances(cases.many(arrays, 65, seed=5))
        plan = host.instances()
        points, normals = surface_points(host, plan, 1171, seed=47)
        assert 1170 * 14 < SORT_MIN <= 1171 * 14
        for n in (1170, 1171):
            want = check(host, arrays, plan, points[:n], normals[:n], what=("threshold", n))
            assert_same(host.instances_directional_occlusion(points[:n], normals[:n], sort=False), want, ("unsorted", n))
            assert want["occluded"].any()
        shuffle = np.random.default_rng(3).permutation(1171)
        seeds = np.arange(1171, dtype=np.uint32)  # (UNIFORM reads no seed; given all the same)
        moved = host.instances_directional_occlusion(np.ascontiguousarray(points[shuffle]), np.ascontiguousarray(normals[shuffle]),
                                                     np.ascontiguousarray(seeds[shuffle]))
        assert_same(moved, {f: want[f][shuffle] for f in FIELDS}, "shuffled")
    finally:
        host.close()


def test_subsets_nothing_and_odd_points(rt, scene_for):
    scene, arrays = scene_for("blob", "sah")
    host = ao_host(rt, scene, 71)
    try:
        host.set_instances(cases.family("overlap_pair", arrays))
        plan = host.instances()
        points, normals = surface_points(host, plan, 700, seed=43)
        want = check(host, arrays, plan, points, normals, what="all four")
        assert want["occluded"].any() and (want["occluded"] == 0).any()
        for subset in (("mask",), ("bent",), ("occluded",), ("ao", "bent"), ("mask", "occluded")):
            part = host.instances_directional_occlusion(points, normals, outputs=subset)
            assert tuple(part) == subset
            assert_same(part, want, subset, fields=subset)
        # a call that asks for nothing launches nothing: the last query's time stays what it was
        before = host.last_query_ms
        assert host.instances_directional_occlusion(points, normals, outputs=()) == {}
        lib = rt.load_library()
        p4 = np.zeros((8, 4), np.float32)
        assert lib.rt_trace_instances_ao_directional(host._h, p4.ctypes.data, p4.ctypes.data, None, 8, 0, None) == 0
        assert host.last_query_ms == before
        with pytest.raises(ValueError):
            host.instances_directional_occlusion(points, normals, outputs=("mask", "instance"))
        # odd points, zero normals among them
        p, q = odd_points(points[:520], normals[:520])
        for sort in (True, False):
            got = check(host, arrays, plan, p, q, sort=sort, what="odd points")
        assert np.isnan(got["bent"]).any()
    finally:
        host.close()


def test_random_method_on_the_gpus_own_terms(rt, scene_for):
    """RANDOM: the sampler depends on the device's libm, so the rays come from host.ao_rays(): every mask bit is
    trace_instances_occluded's flag of that ray, `occluded` is instances_ambient_occlusion's, `bent` the ordered sum."""
    scene, arrays = scene_for("blob", "sah")
    host = ao_host(rt, scene, 14, ao_method=1)
    try:
        host.set_instances(cases.family("rotations", arrays))
        plan = host.instances()
        points, normals = surface_points(host, plan, 700, seed=53)
        seeds = (np.arange(700, dtype=np.uint32) * np.uint32(2654435761)) ^ np.uint32(0x9E3779B9)
        R, divisor = host.ao_rays_per_point
        for given in (seeds, None):
            rays = host.ao_rays(points, normals, given)
            got = check(host, arrays, plan, points, normals, given, sort=given is None, rays=(rays["origins"], rays["directions"]),
                        what=("random", given is None))
            flags = host.trace_instances_occluded(np.repeat(rays["origins"], R, axis=0), rays["directions"].reshape(700 * R, 4),
                                                  max_distance=float(host.options.ao_max_distance), sort=False).reshape(700, R).astype(bool)
            assert np.array_equal(rt.unpack_ao_mask(got["mask"], R), flags)
            ao = host.instances_ambient_occlusion(points, normals, given)
            assert np.array_equal(got["occluded"], ao["occluded"]) and ido.same_words(got["ao"], ao["ao"]).all()
            assert ido.same_words(got["bent"], dro.ordered_sum(rays["directions"], ~flags)).all()
            assert got["occluded"].any()
        other = host.instances_directional_occlusion(points, normals, seeds[::-1].copy(), outputs=("mask",))  # (the seeds are read)
        assert not np.array_equal(other["mask"], host.instances_directional_occlusion(points, normals, seeds, outputs=("mask",))["mask"])
    finally:
        host.close()


@pytest.mark.parametrize("mesh", ["blob", "bunny"])
def test_identity_relation_to_directional_occlusion(rt, scene_for, mesh):
    """One identity instance: on points whose rays hold no -0 every output is directional_occlusion's -- which a set leaves
    what it was."""
    scene, arrays = scene_for(mesh, "longest")
    host = ao_host(rt, scene, 28, ao_max_distance=0.2)
    try:
        W = cases.family("identity", arrays)
        probe = rt.instance_plan(*cases.root_box(arrays), W)
        o, d = cases.rays(probe["nodes"], 6000, seed=61)
        near = host.trace_closest(o, d)
        at = near["hit"].astype(bool) & (near["distance"] < np.inf)
        points, normals = np.ascontiguousarray(near["position"][at][:1500]), np.ascontiguousarray(near["normal"][at][:1500])
        assert len(points) > 300
        plain = host.directional_occlusion(points, normals)
        host.set_instances(W)
        assert_same(host.directional_occlusion(points, normals), plain, "the plain query with a set")
        got = host.instances_directional_occlusion(points, normals)
        rays = host.ao_rays(points, normals)
        clean = ivo.identity_filter(rays["origins"][:, None, :3], rays["directions"][:, :, :3]).all(axis=1)
        print(f"INSTANCE DIRECTIONAL identity {mesh}: {int(clean.sum())} of {len(clean)} points have rays without -0")
        assert clean.mean() > 0.9 and plain["occluded"][clean].any()
        assert_same({f: got[f][clean] for f in FIELDS}, {f: plain[f][clean] for f in FIELDS}, ("identity", mesh))
    finally:
        host.close()


class _DeviceBytes:
    def __init__(self, size):
        self.hip, self.ptr = C.CDLL("libamdhip64.so"), C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.ptr), C.c_size_t(size)) == 0
        assert self.hip.hipMemset(self.ptr, 0, C.c_size_t(size)) == 0

    def free(self):
        self.hip.hipFree(self.ptr)


def test_error_paths(rt, scene_for):
    lib = rt.load_library()
    api = rt.api
    scene, arrays = scene_for("blob", "longest")
    STATE, INVALID = api.RT_E_STATE, api.RT_E_INVALID
    W = cases.family("rotations", arrays)
    p = np.zeros((4, 3), np.float32)
    host = ao_host(rt, None)
    with pytest.raises(rt.RtError) as e:  # no upload, no set
        host.instances_directional_occlusion(p, p, outputs=("bent",))
    assert e.value.code == STATE
    host.set_instances(W)
    with pytest.raises(rt.RtError) as e:  # a set, no upload
        host.instances_directional_occlusion(p, p, outputs=("bent",))
    assert e.value.code == STATE
    host.upload_scene(scene)
    host.set_instances(EMPTY)
    with pytest.raises(rt.RtError) as e:  # an upload, no set
        host.instances_directional_occlusion(p, p, outputs=("bent",))
    assert e.value.code == STATE
    assert host.directional_occlusion(p, p, outputs=("bent",))["bent"].shape == (4, 3)  # (the plain form needs none)
    host.set_instances(W)
    p4 = np.zeros((4, 4), np.float32)
    at = p4.ctypes.data
    call, device = lib.rt_trace_instances_ao_directional, lib.rt_trace_instances_ao_directional_device
    assert call(host._h, None, at, None, 4, 0, None) == INVALID
    assert call(host._h, at, None, None, 4, 0, None) == INVALID
    assert call(host._h, None, None, None, 0, 0, None) == 0
    assert call(None, at, at, None, 4, 0, None) == INVALID
    assert call(host._h, at, at, None, (1 << 27) // 14 + 1, 0, None) == INVALID
    mem = _DeviceBytes(2 * 65 * 16 + 8192)
    a, b, out = mem.ptr.value, mem.ptr.value + 65 * 16, mem.ptr.value + 2 * 65 * 16

    def arrays_of(ao=None, occluded=None, mask=None, bent=None):
        return C.byref(api._DirectionalArrays(ao, occluded, mask, bent))

    assert device(host._h, a + 4, b, None, 64, 0, arrays_of(out), None) == INVALID
    assert device(host._h, a, b + 8, None, 64, 0, arrays_of(out), None) == INVALID
    assert device(host._h, a, b, out + 2, 64, 0, arrays_of(out + 1024), None) == INVALID
    assert device(host._h, a, b, None, 64, 0, arrays_of(mask=out + 1), None) == INVALID
    assert device(host._h, a, b, None, 64, 0, arrays_of(bent=out + 2), None) == INVALID
    assert device(host._h, a, b, None, 64, 0, arrays_of(out, out + 1024, out + 2048, out + 4096), None) == 0
    assert device(host._h, a, b, None, 64, 0, None, None) == 0
    assert host.last_query_ms >= 0.0  # (waits for the query)
    host.close()
    mem.free()
    off = rt.Host(rt.Options.defaults(width=32, height=24, enable_ao=0), 0)  # ambient occlusion off
    off.upload_scene(scene)
    off.set_instances(W)
    assert lib.rt_trace_instances_ao_directional(off._h, at, at, None, 4, 0, None) == STATE
    off.close()
    ring = rt.FrameRing(rt.Options.defaults(width=32, height=32, ao_num_samples=3), hosts=2)
    ring.set_calibration(False)
    ring.upload_scene(scene)
    with pytest.raises(rt.RtError) as e:
        ring.host(0).instances_directional_occlusion(p, p, outputs=("bent",))
    assert e.value.code == STATE
    ring.close()


def test_torch_path_equals_numpy_path():
    """Device tensors in and device tensors out on a non-default stream == the numpy path
    (tests/instance_directional_torch_driver.py, a child process that brings torch's runtime up before it loads the library)."""
    driver = os.path.join(os.path.dirname(os.path.abspath(__file__)), "instance_directional_torch_driver.py")
    r = subprocess.run([sys.executable, driver], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "INSTANCE_DIRECTIONAL_TORCH_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
