"""GPU: multi-hit ray queries (include/rt_hip_multihit.h) against the CPU oracle of tests/multihit_oracle.c, every output
word for word."""
import numpy as np
import pytest

import multihit_oracle as mo
import orc
import query_oracle as qo
from conftest import bits

pytestmark = pytest.mark.gpu

CASES = [("single", "longest"), ("single", "sah"), ("ties", "longest"), ("ties", "sah"), ("blob", "longest"), ("blob", "sah"),
         ("bunny", "longest")]
BVHS = ["longest", "sah"]
CLOSEST_FIELDS = ("distance", "leaf", "barycentric", "position", "normal")


@pytest.fixture(scope="module")
def hosts(rt, scene_for):
    made = {}

    def get(mesh, bvh):
        if (mesh, bvh) not in made:
            scene, arrays = mo.layered_scene(rt, bvh) if mesh == "layered" else scene_for(mesh, bvh)
            host = rt.Host(rt.Options.defaults(width=64, height=48, n_super_samples=1), 0)
            host.upload_scene(scene)
            made[(mesh, bvh)] = (host, scene, arrays)
        return made[(mesh, bvh)]

    yield get
    for host, _, _ in made.values():
        host.close()


_WANT = {}


def oracle_for(tag, arrays, o, d, max_distance):
    """The oracle's answer with RT_MULTIHIT_MAX_K slots, computed once per ray set (`tag` names it) and never changed:
    the answer for fewer slots is its first slots."""
    key = (tag, repr(float(max_distance)))
    if key not in _WANT:
        _WANT[key] = mo.multihit(arrays, o, d, max_distance, mo.MAX_K)
        for v in _WANT[key].values():
            v.setflags(write=False)
    return _WANT[key]


def assert_same(got, want, fields=mo.FIELDS):
    for f in fields:
        assert got[f].shape == want[f].shape, (f, got[f].shape, want[f].shape)
        same = mo.same_words(got[f], want[f])
        assert same.all(), (f, int((~same).sum()), np.argwhere(~same)[:5].tolist())


def check(host, full, o, d, max_distance, k, sort=True):
    got = host.trace_multihit(o, d, max_distance, k=k, sort=sort)
    assert_same(got, mo.first_slots(full, k))
    return got


def camera_rays(rt, w=64, h=48):
    opt = rt.Options.defaults(width=w, height=h, n_super_samples=1, enable_ao=0)
    return qo.camera_rays(orc.params_from_options(opt))


@pytest.mark.parametrize("mesh,bvh", CASES)
def test_multihit_matches_oracle(rt, hosts, mesh, bvh):
    host, _, arrays = hosts(mesh, bvh)
    o4, d4 = camera_rays(rt)
    ro, rd = mo.random_rays(arrays, 20000, seed=3 + 2 * CASES.index((mesh, bvh)))
    cam = oracle_for(("camera", mesh, bvh), arrays, o4, d4, 100000.0)
    rnd = oracle_for(("random", mesh, bvh), arrays, ro, rd, 100000.0)
    for k in (1, 3, 16):
        check(host, cam, o4, d4, 100000.0, k)
        a = check(host, rnd, ro, rd, 100000.0, k, sort=True)  # (above RT_QUERY_SORT_MIN: sorted)
        b = check(host, rnd, ro, rd, 100000.0, k, sort=False)
        for f in mo.FIELDS:
            assert mo.same_words(a[f], b[f]).all(), f


@pytest.mark.parametrize("bvh", BVHS)
def test_layered_scene_overflow_and_ties(rt, hosts, bvh):
    """Lists that overflow and evict (more than 16 layers along a ray) and equal distances ordered by the leaf index, for
    every k: each instantiation of the walk (1, 2, 4, 8, 16 slots a lane) with a full list and with k below its slots."""
    host, _, arrays = hosts("layered", bvh)
    o, d, _ = mo.layered_rays(arrays)
    full = oracle_for(("layered", bvh), arrays, o, d, 100000.0)
    for k in range(1, mo.MAX_K + 1):
        check(host, full, o, d, 100000.0, k)
    check(host, full, o, d, 100000.0, 16, sort=False)
    assert np.array_equal(host.count_hits(o, d), full["count"])  # k = 0: the count alone


def odd_rays(arrays, n=4000, seed=3):
    """The generator of tests/test_query_gpu.py's odd_rays: zero / denormal / huge / NaN / inf components, far origins."""
    lo, hi = mo.box_of(arrays)
    o, d = mo.random_rays(arrays, n, seed)
    k = np.arange(n)
    d[k % 7 == 0, 0] = 0.0                                     # zero components
    d[k % 11 == 0, 1] = -0.0
    d[k % 13 == 0] *= np.float32(37.0)                          # non-unit
    d[k % 17 == 0] *= np.float32(1e-30)                         # tiny (denormal products)
    d[k % 19 == 0, 2] = np.float32(1e-41)                       # a denormal component
    d[k % 23 == 0] *= np.float32(1e30)                          # huge
    d[k % 29 == 0] = 0.0                                        # no direction at all
    far = float(np.max(np.abs(np.concatenate([lo, hi])))) * 50 + 100
    o[k % 31 == 0] += np.float32(far)                           # far origins
    o[k % 37 == 0] = np.float32(3e38)
    o[k % 41 == 0, 1] = np.nan
    d[k % 43 == 0, 2] = np.nan
    o[k % 47 == 0, 0] = np.inf
    d[k % 53 == 0, 0] = -np.inf
    back = (k % 31 == 0)                                        # aim the far origins back at the scene
    centre = ((lo + hi) / 2).astype(np.float32)
    d[back] = (centre - o[back]).astype(np.float32)
    return o.astype(np.float32), d.astype(np.float32)


@pytest.mark.parametrize("max_distance", [1e5, 0.2, 0.0, -1.0, np.inf, np.nan])
def test_odd_inputs_and_max_distances(rt, hosts, max_distance):
    host, _, arrays = hosts("blob", "longest")
    o, d = odd_rays(arrays)
    md = np.float32(max_distance)
    check(host, oracle_for(("odd", "blob"), arrays, o, d, md), o, d, md, 4)


def test_batch_sizes(rt, hosts):
    host, _, arrays = hosts("blob", "longest")
    o, d = mo.random_rays(arrays, 257, seed=11, grow=0.0)
    full = oracle_for(("batch", "blob"), arrays, o, d, 100000.0)
    for n in (0, 1, 63, 64, 65, 257):
        got = host.trace_multihit(o[:n], d[:n], k=3)
        assert got["count"].shape == (n,) and got["leaf"].shape == (n, 3) and got["normal"].shape == (n, 3, 3)
        assert_same(got, {f: v[:n] for f, v in mo.first_slots(full, 3).items()})
        assert host.count_hits(o[:n], d[:n]).shape == (n,)


def test_agrees_with_the_other_entry_points(rt, hosts):
    host, _, arrays = hosts("blob", "sah")
    o4, d4 = camera_rays(rt)
    ro, rd = mo.random_rays(arrays, 20000, seed=17)
    o, d = np.concatenate([o4[:, :3], ro]), np.concatenate([d4[:, :3], rd])
    for md in (100000.0, 0.5):
        multi = host.trace_multihit(o, d, md, k=2)
        assert np.array_equal(multi["count"] > 0, host.trace_occluded(o, d, md).astype(bool))
        near = host.trace_closest(o, d, md)
        kept = near["hit"].astype(bool) & (near["distance"] < np.inf)
        assert kept.sum() > 100
        for f in CLOSEST_FIELDS:
            assert mo.same_words(multi[f][:, 0], near[f])[kept].all(), f
        assert np.array_equal(host.count_hits(o, d, md), multi["count"])


def test_output_subsets(rt, hosts):
    host, _, arrays = hosts("blob", "longest")
    o, d = mo.random_rays(arrays, 20000, seed=3 + 2 * CASES.index(("blob", "longest")))
    want = mo.first_slots(oracle_for(("random", "blob", "longest"), arrays, o, d, 100000.0), 3)
    for outputs in (("count",), ("leaf",), ("count", "distance", "leaf", "barycentric", "position")):
        got = host.trace_multihit(o, d, k=3, outputs=outputs)
        assert set(got) == set(outputs)
        assert_same(got, want, outputs)


def test_error_paths(rt, scene_for):
    scene, _ = scene_for("blob", "longest")
    opt = rt.Options.defaults(width=32, height=32)
    host = rt.Host(opt, 0)
    o = np.zeros((4, 3), np.float32)
    with pytest.raises(rt.RtError) as e:
        host.trace_multihit(o, o)
    assert e.value.code == rt.api.RT_E_STATE == -4
    with pytest.raises(rt.RtError) as e:
        host.count_hits(o, o)
    assert e.value.code == rt.api.RT_E_STATE
    host.upload_scene(scene)
    with pytest.raises(rt.RtError) as e:
        host.trace_multihit(o, o, k=17)
    assert e.value.code == rt.api.RT_E_INVALID == -1
    with pytest.raises(rt.RtError) as e:
        host.trace_multihit(o, o, k=0, outputs=("count", "leaf"))
    assert e.value.code == rt.api.RT_E_INVALID
    lib = rt.load_library()
    assert lib.rt_trace_multihit(host._h, None, None, 4, 1.0, 2, 0, None) == rt.api.RT_E_INVALID
    assert lib.rt_trace_multihit_device(host._h, None, None, 4, 1.0, 2, 0, None, None) == rt.api.RT_E_INVALID
    assert lib.rt_trace_multihit(host._h, None, None, 0, 1.0, 2, 0, None) == 0
    assert lib.rt_trace_multihit(host._h, o.ctypes.data, o.ctypes.data, (1 << 27) // 16 + 1, 1.0, 16, 0, None) == rt.api.RT_E_INVALID
    assert host.trace_multihit(o, o, k=0, outputs=("count",))["count"].shape == (4,)
    host.close()
    ring = rt.FrameRing(opt, hosts=2)
    ring.set_calibration(False)
    ring.upload_scene(scene)
    with pytest.raises(rt.RtError) as e:
        ring.host(0).trace_multihit(o, o)
    assert e.value.code == rt.api.RT_E_STATE
    ring.close()


def test_multihit_leaves_frames_alone(rt, scene_for):
    scene, arrays = scene_for("blob", "longest")
    host = rt.Host(rt.Options.defaults(width=64, height=48, n_super_samples=1, ao_num_samples=3), 0)
    host.upload_scene(scene)
    host.render()
    first = host.download()
    stats = host.stats()
    o, d = mo.random_rays(arrays, 20000, seed=9)
    host.trace_multihit(o, d, k=4)
    host.count_hits(o, d)
    assert host.last_query_ms > 0.0
    assert host.stats() == stats
    host.render()
    assert np.array_equal(bits(host.download()), bits(first))
    assert host.stats() == stats
    host.close()


def test_torch_path_equals_numpy_path():
    """Device tensors in and out on a non-default stream == the numpy path (tests/multihit_torch_driver.py, a child
    process that brings torch's runtime up before it loads the library)."""
    import os
    import subprocess
    import sys

    driver = os.path.join(os.path.dirname(os.path.abspath(__file__)), "multihit_torch_driver.py")
    r = subprocess.run([sys.executable, driver], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "MULTIHIT_TORCH_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
