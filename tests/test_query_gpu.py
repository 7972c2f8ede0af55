"""GPU: ray queries (include/rt_hip_query.h) against the CPU oracle of tests/query_oracle.c, every output word for word."""
import ctypes as C

import numpy as np
import pytest

import orc
import query_oracle as qo
from conftest import bits

pytestmark = pytest.mark.gpu

MESHES = ["bunny", "blob", "ties", "single", "interior_hard"]
BVHS = ["longest", "sah"]
FIELDS = ("hit", "distance", "leaf", "barycentric", "position", "normal")
AO_MAX = 0.2


def check(host, arrays, o, d, max_distance, sort=True):
    """Closest hit and occlusion of the rays on the GPU == the oracle's, bit for bit; occluded == closest hit."""
    got = host.trace_closest(o, d, max_distance, sort=sort)
    want = qo.closest(arrays, o, d, max_distance)
    for f in FIELDS:
        same = qo.same_words(got[f], want[f])
        assert same.all(), (f, int((~same).sum()), np.argwhere(~same)[:5].tolist())
    occ = host.trace_occluded(o, d, max_distance, sort=sort)
    assert np.array_equal(occ, got["hit"])
    return got


def box_of(arrays):
    lo, hi = arrays.aabbs[0, :3], arrays.aabbs[1, :3]
    return lo.astype(np.float64), hi.astype(np.float64)


def random_rays(arrays, n, seed, grow=0.25):
    rng = np.random.default_rng(seed)
    lo, hi = box_of(arrays)
    ext = hi - lo
    o = (lo - grow * ext + rng.random((n, 3)) * (1 + 2 * grow) * ext).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    return o, d.astype(np.float32)


def camera(rt, w=64, h=48):
    opt = rt.Options.defaults(width=w, height=h, n_super_samples=1, enable_ao=0)
    return opt, qo.camera_rays(orc.params_from_options(opt))


@pytest.fixture(scope="module")
def hosts(rt, scene_for):
    made = {}

    def get(mesh, bvh):
        if (mesh, bvh) not in made:
            scene, arrays = scene_for(mesh, bvh)
            host = rt.Host(rt.Options.defaults(width=64, height=48, n_super_samples=1, ao_max_distance=AO_MAX), 0)
            host.upload_scene(scene)
            made[(mesh, bvh)] = (host, scene, arrays)
        return made[(mesh, bvh)]

    yield get
    for host, _, _ in made.values():
        host.close()


@pytest.mark.parametrize("bvh", BVHS)
@pytest.mark.parametrize("mesh", MESHES)
def test_queries_match_oracle(rt, hosts, mesh, bvh):
    host, scene, arrays = hosts(mesh, bvh)
    # camera rays: every field, and the float image they rebuild equals the oracle's (-a 0)
    _, (o4, d4) = camera(rt)
    cam = check(host, arrays, o4, d4, 100000.0)
    # AO-like rays: the camera hits offset by normal * 1e-5, a few unit directions each, ao_max_distance
    hit = cam["hit"].astype(bool) & (cam["distance"] < np.inf)
    p = cam["position"][hit][:400]
    nrm = cam["normal"][hit][:400]
    if len(p):
        origin = (p + nrm * np.float32(1e-5)).astype(np.float32)
        rng = np.random.default_rng(7)
        dirs = rng.normal(size=(len(origin) * 8, 3)).astype(np.float32)
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True).astype(np.float32)
        check(host, arrays, np.repeat(origin, 8, axis=0), dirs, AO_MAX)
    # random rays inside and around the box, sorted and not (above the sort threshold)
    o, d = random_rays(arrays, 20000, seed=2 * MESHES.index(mesh) + BVHS.index(bvh))
    a = check(host, arrays, o, d, 100000.0, sort=True)
    b = check(host, arrays, o, d, 100000.0, sort=False)
    for f in FIELDS:
        assert qo.same_words(a[f], b[f]).all()
    # rays aimed exactly at shared vertices and edge midpoints
    verts = arrays.vertices[:, :3]
    f3 = arrays.faces.reshape(-1, 3)[:300]
    targets = np.concatenate([verts[f3[:, 0]], (verts[f3[:, 0]] + verts[f3[:, 1]]) * np.float32(0.5)]).astype(np.float32)
    src = np.array([0.0, 0.0, 2.0], np.float32)
    dd = (targets - src).astype(np.float32)
    check(host, arrays, np.repeat(src[None], len(dd), axis=0), dd, 100000.0)
    # leaf -> file-order face
    leaves = cam["leaf"]
    faces = scene.face_of_leaf(leaves)
    assert np.array_equal(faces[leaves == qo.NONE], leaves[leaves == qo.NONE])
    assert np.array_equal(faces[leaves != qo.NONE], scene.triangles[leaves[leaves != qo.NONE]])


def odd_rays(arrays, n=4000, seed=3):
    rng = np.random.default_rng(seed)
    lo, hi = box_of(arrays)
    o, d = random_rays(arrays, n, seed)
    k = np.arange(n)
    d[k % 7 == 0, 0] = 0.0                                     # zero components
    d[k % 11 == 0, 1] = -0.0
    d[k % 13 == 0] *= np.float32(37.0)                          # non-unit
    d[k % 17 == 0] *= np.float32(1e-30)                         # tiny (denormal products)
    d[k % 19 == 0, 2] = np.float32(1e-41)                       # a denormal component
    d[k % 23 == 0] *= np.float32(1e30)                          # huge
    d[k % 29 == 0] = 0.0                                        # no direction at all
    far = float(np.max(np.abs(np.concatenate([lo, hi])))) * 50 + 100
    o[k % 31 == 0] += np.float32(far)                           # beyond origin_limit
    o[k % 37 == 0] = np.float32(3e38)
    o[k % 41 == 0, 1] = np.nan
    d[k % 43 == 0, 2] = np.nan
    o[k % 47 == 0, 0] = np.inf
    d[k % 53 == 0, 0] = -np.inf
    # aim the far origins back at the scene
    back = (k % 31 == 0)
    centre = ((lo + hi) / 2).astype(np.float32)
    d[back] = (centre - o[back]).astype(np.float32)
    return o.astype(np.float32), d.astype(np.float32)


@pytest.mark.parametrize("mesh", ["blob", "ties", "interior_hard"])
def test_odd_inputs_and_max_distances(rt, hosts, mesh):
    host, _, arrays = hosts(mesh, "longest")
    o, d = odd_rays(arrays)
    for md in (1e5, AO_MAX, 0.01, np.inf, 0.0, -1.0, np.nan):
        check(host, arrays, o, d, np.float32(md))


def test_batch_sizes(rt, hosts):
    host, _, arrays = hosts("blob", "longest")
    o, d = random_rays(arrays, 100003, seed=11, grow=0.0)
    for n in (0, 1, 63, 64, 65, 100003):
        got = host.trace_closest(o[:n], d[:n])
        assert got["hit"].shape == (n,)
        if n:
            check(host, arrays, o[:n], d[:n], 100000.0)


@pytest.mark.parametrize("damage", ["inverted_box", "nan_leaf_box", "huge_box", "inf_box", "nan_vertex", "child_outside_parent",
                                    "collinear_triangle"])
def test_damaged_scene_arrays(rt, scene_for, damage):
    """The irregular arrays of tests/test_hip_parity.py's upload test, made again here."""
    _, arrays = scene_for("blob", "longest")
    nodes, aabbs, verts, faces = arrays.nodes.copy(), arrays.aabbs.copy(), arrays.vertices.copy(), arrays.faces.copy()
    inner = int(np.flatnonzero(nodes > 8)[5])
    leaf = int(np.flatnonzero(nodes == 1)[40])
    if damage == "inverted_box":
        aabbs[2 * inner, 0], aabbs[2 * inner + 1, 0] = aabbs[2 * inner + 1, 0], aabbs[2 * inner, 0]
    elif damage == "nan_leaf_box":
        aabbs[2 * leaf, 1] = np.nan
    elif damage == "huge_box":
        aabbs[0, :3] = -3.0e38
        aabbs[1, :3] = 3.0e38
    elif damage == "inf_box":
        aabbs[0, 2] = -np.inf
        aabbs[1, 0] = np.inf
    elif damage == "nan_vertex":
        verts[int(arrays.faces[3 * 17]), 1] = np.nan
    elif damage == "child_outside_parent":
        aabbs[2 * inner + 1, 0] = aabbs[2 * inner, 0] + 1.0e-3
    elif damage == "collinear_triangle":
        for face in (17, 40, 41):
            faces[3 * face + 2] = faces[3 * face + 1]
    damaged = orc.SceneArrays(faces, nodes, aabbs, verts, arrays.normals)
    host = rt.Host(rt.Options.defaults(width=64, height=48, n_super_samples=1, ao_max_distance=0.5), 0)
    host.upload(damaged.faces, damaged.nodes, damaged.aabbs, damaged.vertices, damaged.normals)
    _, (o4, d4) = camera(rt)
    check(host, damaged, o4, d4, 100000.0)
    o, d = random_rays(arrays, 20000, seed=5)
    check(host, damaged, o, d, 0.5)
    check(host, damaged, *odd_rays(arrays, 2000), 100000.0)
    host.close()


def test_camera_queries_rebuild_the_hip_render(rt, scene_for):
    """hit / normal of the camera rays give the HIP render's own float image (-a 0), shading on and off; a stream host."""
    scene, arrays = scene_for("bunny", "longest")
    for shading in (1, 0):
        opt = rt.Options.defaults(width=160, height=120, n_super_samples=1, enable_ao=0, enable_shading=shading)
        host = rt.Host(opt, 0)
        host.expect_frames(1000)
        host.upload_scene(scene)
        host.render()
        img = host.download()
        o4, d4 = qo.camera_rays(orc.params_from_options(opt))
        got = check(host, arrays, o4, d4, 100000.0)
        value = qo.shade(got["hit"], got["normal"], d4, bool(shading)).reshape(img.shape)
        assert np.array_equal(bits(value), bits(img))
        host.close()


def test_queries_leave_frames_alone(rt, oracle, scene_for):
    scene, arrays = scene_for("bunny", "longest")
    opt = rt.Options.defaults(width=96, height=64, n_super_samples=4, ao_num_samples=3)
    ref_img, counters, _ = oracle.render(orc.params_from_options(opt), arrays)
    host = rt.Host(opt, 0)
    host.upload_scene(scene)
    host.render()
    assert np.array_equal(bits(host.download()), bits(ref_img))
    stats = host.stats()
    o, d = random_rays(arrays, 30000, seed=9)
    before = host.trace_closest(o, d)
    assert host.stats() == stats
    host.render()
    assert np.array_equal(bits(host.download()), bits(ref_img))
    host.render_async()  # a frame left in flight while a batch of queries runs
    during = host.trace_closest(o, d)
    host.trace_occluded(o, d, AO_MAX)
    host.sync()
    assert np.array_equal(bits(host.download()), bits(ref_img))
    assert host.stats() == stats
    assert host.stats()["ao_occluded"] == counters["ao_occluded"]
    for f in FIELDS:
        assert qo.same_words(before[f], during[f]).all()
    assert host.last_query_ms > 0.0
    host.close()


class _DeviceBytes:
    """Device memory straight from the HIP runtime the library uses (torch brings its own copy of the runtime, which
    cannot be initialised in a process that loaded the library first: the torch path runs in a child process)."""

    def __init__(self, size):
        self.hip, self.ptr = C.CDLL("libamdhip64.so"), C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.ptr), C.c_size_t(size)) == 0
        assert self.hip.hipMemset(self.ptr, 0, C.c_size_t(size)) == 0

    def free(self):
        self.hip.hipFree(self.ptr)


def test_error_paths(rt, scene_for):
    lib = rt.load_library()
    scene, _ = scene_for("blob", "longest")
    host = rt.Host(rt.Options.defaults(width=32, height=32), 0)
    o = np.zeros((4, 3), np.float32)
    with pytest.raises(rt.RtError) as e:
        host.trace_closest(o, o)
    assert e.value.code == rt.api.RT_E_STATE
    with pytest.raises(rt.RtError) as e:
        host.trace_occluded(o, o)
    assert e.value.code == rt.api.RT_E_STATE
    host.upload_scene(scene)
    assert lib.rt_trace_closest(host._h, None, None, 4, 1.0, 0, None) == rt.api.RT_E_INVALID
    assert lib.rt_trace_occluded(host._h, None, None, 4, 1.0, 0, None) == rt.api.RT_E_INVALID
    assert lib.rt_trace_closest_device(host._h, None, None, 4, 1.0, 0, None, None) == rt.api.RT_E_INVALID
    assert lib.rt_trace_closest(host._h, None, None, 0, 1.0, 0, None) == 0
    assert lib.rt_trace_closest(host._h, o.ctypes.data, o.ctypes.data, (1 << 27) + 1, 1.0, 0, None) == rt.api.RT_E_INVALID
    with pytest.raises(ValueError):
        host.trace_closest(o.astype(np.float64), o)
    mem = _DeviceBytes(2 * 65 * 16 + 64)
    rays, out = mem.ptr.value, mem.ptr.value + 2 * 65 * 16
    assert lib.rt_trace_occluded_device(host._h, rays + 4, rays, 64, 1.0, 0, out, None) == rt.api.RT_E_INVALID
    assert lib.rt_trace_closest_device(host._h, rays, rays + 8, 64, 1.0, 0, None, None) == rt.api.RT_E_INVALID
    assert lib.rt_trace_occluded_device(host._h, rays, rays + 16 * 65, 64, 1.0, 0, out, None) == 0
    host.close()
    mem.free()
    import torch  # (CPU tensors: the checks come before any device work)

    t = torch.zeros((65, 4), dtype=torch.float32)
    with pytest.raises(ValueError):
        host.trace_closest(t[:, :3], t[:, :3])  # (65, 3), not contiguous
    with pytest.raises(ValueError):
        host.trace_closest(t.double(), t.double())


def test_torch_path_equals_numpy_path():
    """Device tensors in and out on a non-default stream == the numpy path (tests/query_torch_driver.py, a child process
    that brings torch's runtime up before it loads the library)."""
    import os
    import subprocess
    import sys

    driver = os.path.join(os.path.dirname(os.path.abspath(__file__)), "query_torch_driver.py")
    r = subprocess.run([sys.executable, driver], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "QUERY_TORCH_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
