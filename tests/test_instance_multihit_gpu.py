"""GPU: instanced multi-hit queries (include/rt_hip_instance_multihit.h) against the CPU oracle of
tests/instance_multihit_oracle.c on the plan read back from the host, every output word for word; the header's relations
against the GPU's own trace_instances_closest, trace_instances_occluded and trace_multihit; the float64 comparator of
tests/instance_multihit_reference.py on the GPU's answers; and what the calls leave alone."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import build_cases as bc
import instance_cases as cases
import instance_multihit_oracle as imo
import instance_multihit_reference as imr
import multihit_oracle as mo
import orc
import refit_cases as rc
from conftest import bits

pytestmark = pytest.mark.gpu

SORT_MIN = 16384  # RT_QUERY_SORT_MIN
SIZES = (1, 63, 64, 65, 257, 16383, 16421)
KS = (0, 1, 2, 3, 4, 5, 8, 15, 16)
FAMILIES = ("identity", "tie_pair", "overlap_pair", "shear", "mirror", "grid")
CASES = [(mesh, bvh) for mesh in ("single", "ties", "blob", "layered") for bvh in ("longest", "sah")]
K = imo.MAX_K
NONE = imo.NONE
EMPTY = np.zeros((0, 3, 4), np.float32)


def new_host(rt, scene=None, **options):
    host = rt.Host(rt.Options.defaults(width=64, height=48, n_super_samples=1, **options), 0)
    if scene is not None:
        host.upload_scene(scene)
    return host


@pytest.fixture(scope="module")
def hosts(rt, scene_for):
    made = {}

    def get(mesh, bvh):
        if (mesh, bvh) not in made:
            scene, arrays = mo.layered_scene(rt, bvh) if mesh == "layered" else scene_for(mesh, bvh)
            made[(mesh, bvh)] = (new_host(rt, scene), scene, arrays)
        return made[(mesh, bvh)]

    yield get
    for host, _, _ in made.values():
        host.close()


def ask(host, o, d, max_distance, k, sort=True, outputs=None):
    """trace_instances_multihit with every output k allows (k = 0: the count alone)."""
    if outputs is None:
        outputs = rt_outputs() if k else ("count",)
    return host.trace_instances_multihit(o, d, max_distance, k=k, outputs=outputs, sort=sort)


def rt_outputs():
    import opencl_raytracer_amd as rt

    return rt.INSTANCE_MULTIHIT_OUTPUTS


def expected(full, n, k):
    """The first n rays and the first k slots of the oracle's answer with 16 slots (k = 0: the count alone)."""
    part = {f: np.ascontiguousarray(v[:n]) for f, v in full.items()}
    return imo.first_slots(part, k) if k else {"count": part["count"]}


def check(host, full, o, d, max_distance, n, k, sort=True, what=""):
    got = ask(host, o[:n], d[:n], max_distance, k, sort)
    want = expected(full, n, k)
    assert set(got) == set(want), (what, sorted(got))
    for f in want:
        assert got[f].shape == want[f].shape and got[f].dtype == want[f].dtype, (what, f, got[f].shape, want[f].shape, got[f].dtype)
    imo.assert_same(got, want, (what, n, k, sort, max_distance))
    return got


def rays_for(mesh, plan, arrays, W, n, seed):
    if mesh != "layered":
        return cases.rays(plan["nodes"], n, seed)
    o, d, _ = imo.layered_rays(plan, arrays, W, n_axis=n // 2, n_oblique=n - n // 2, seed=seed)
    shuffle = np.random.default_rng(seed).permutation(n)  # (every prefix holds rays of both kinds)
    return np.ascontiguousarray(o[shuffle]), np.ascontiguousarray(d[shuffle])


@pytest.mark.parametrize("mesh,bvh", CASES)
def test_every_word_matches_the_oracle(rt, hosts, mesh, bvh):
    """Every family, every k and every ray count: each family takes all the counts with k going round, and all the k with the
    counts going round; sorted and unsorted calls alternate; max_distance goes round 1e5, 5 and 0.3."""
    host, _, arrays = hosts(mesh, bvh)
    members, most = 0, 0
    for i, family in enumerate(FAMILIES):
        W = cases.family(family, arrays)
        host.set_instances(W)
        plan = host.instances()
        o, d = rays_for(mesh, plan, arrays, W, max(SIZES), seed=90 + i)
        max_distance = cases.MAX_DISTANCES[i % 3]
        full = imo.multihit(arrays, plan, o, d, max_distance, K)
        what = (mesh, bvh, family)
        for j, n in enumerate(SIZES):
            check(host, full, o, d, max_distance, n, KS[(i + j) % len(KS)], sort=bool((i + j) % 2), what=what)
        for j, k in enumerate(KS):
            check(host, full, o, d, max_distance, SIZES[(2 * i + j + 3) % len(SIZES)], k, sort=bool((i + j + 1) % 2), what=what)
        check(host, full, o, d, max_distance, max(SIZES), K, sort=True, what=what)
        check(host, full, o, d, max_distance, max(SIZES), K, sort=False, what=what)
        assert np.array_equal(host.count_instances_hits(o, d, max_distance), full["count"]), what
        members += int(full["count"].sum())
        most = max(most, int(full["count"].max()))
    assert members > 0 and host.last_query_ms > 0.0
    if mesh == "layered":
        assert most > K  # (lists that overflow and evict)
    empty = ask(host, o[:0], d[:0], 1e5, 3)
    assert empty["count"].shape == (0,) and empty["instance"].shape == (0, 3) and empty["normal"].shape == (0, 3, 3)
    host.set_instances(EMPTY)


def test_three_calls_return_identical_words(rt, hosts):
    host, _, arrays = hosts("blob", "sah")
    host.set_instances(cases.family("grid", arrays))
    plan = host.instances()
    o, d = cases.rays(plan["nodes"], 16421, seed=7)
    first = ask(host, o, d, 1e5, K)
    for sort in (True, False):
        imo.assert_same(ask(host, o, d, 1e5, K, sort), first, ("again", sort))
    assert first["count"].max() >= 2
    host.set_instances(EMPTY)


@pytest.mark.parametrize("count", cases.COUNTS)
def test_instance_counts(rt, hosts, count):
    host, _, arrays = hosts("blob", "longest")
    host.set_instances(cases.many(arrays, count, seed=3))
    plan = host.instances()
    o, d = cases.rays(plan["nodes"], 500, seed=41 + count)
    full = imo.multihit(arrays, plan, o, d, 1e5, K)
    for k in (4, 16):
        got = check(host, full, o, d, 1e5, 500, k, what=("count", count))
    used = got["instance"] != NONE
    assert used.any() and (got["instance"][used] < count).all()
    host.set_instances(EMPTY)


def test_output_subsets_count_alone_and_odd_rays(rt, hosts):
    host, _, arrays = hosts("blob", "longest")
    host.set_instances(cases.family("overlap_pair", arrays))
    plan = host.instances()
    o, d = cases.rays(plan["nodes"], 3000, seed=13)
    full = imo.multihit(arrays, plan, o, d, 1e5, K)
    want = imo.first_slots(full, 3)
    for outputs in (("count",), ("instance",), ("leaf", "instance"), ("distance",), ("count", "normal"), ("position", "barycentric", "instance")):
        got = ask(host, o, d, 1e5, 3, outputs=outputs)
        assert set(got) == set(outputs)
        imo.assert_same(got, want, outputs)
    assert ask(host, o, d, 1e5, 3, outputs=()) == {}
    assert np.array_equal(ask(host, o, d, 1e5, 5, outputs=("count",))["count"], full["count"])  # (count alone with k > 0: no list)
    with pytest.raises(ValueError):
        ask(host, o, d, 1e5, 3, outputs=("count", "hit"))
    # odd rays, odd max_distance values
    for family in ("shear", "mirror", "tie_pair"):
        host.set_instances(cases.family(family, arrays))
        plan = host.instances()
        oo, od = cases.odd_rays(plan["nodes"])
        for max_distance in cases.MAX_DISTANCES + (np.inf, np.nan, -1.0, 0.0):
            full = imo.multihit(arrays, plan, oo, od, max_distance, K)
            got = check(host, full, oo, od, max_distance, len(oo), 4, what=(family, "odd rays"))
            quiet = (od == 0).all(axis=1) | np.isnan(oo).any(axis=1) | np.isnan(od).any(axis=1)
            assert not got["count"][quiet].any()
    host.set_instances(EMPTY)


def test_relations_on_the_gpu(rt, hosts):
    """count > 0 is trace_instances_occluded's flag; slot 0 is trace_instances_closest's record; k slots are the first k of 16;
    one identity instance gives trace_multihit's words."""
    for mesh in ("blob", "layered"):
        host, _, arrays = hosts(mesh, "longest")
        for family in ("tie_pair", "overlap_pair", "grid"):
            W = cases.family(family, arrays)
            host.set_instances(W)
            plan = host.instances()
            o, d = rays_for(mesh, plan, arrays, W, 3000, seed=21)
            oo, od = cases.odd_rays(plan["nodes"])
            o, d = np.concatenate([o, oo]), np.concatenate([d, od])
            for max_distance in (1e5, 0.3):
                full = ask(host, o, d, max_distance, K)
                assert np.array_equal(full["count"] > 0, host.trace_instances_occluded(o, d, max_distance).astype(bool)), (mesh, family)
                near = host.trace_instances_closest(o, d, max_distance)
                at = near["distance"] < np.inf
                assert at.any()
                for f in imo.SLOT_FIELDS:
                    assert imo.same_words(full[f][:, 0][at], near[f][at]).all(), (mesh, family, f)
                for k in (1, 3, 8):
                    imo.assert_same(ask(host, o, d, max_distance, k), imo.first_slots(full, k), (mesh, family, k))
                assert imo.in_contract_order(full).all() and imo.fill_values_hold(full).all()
        host.set_instances(cases.family("identity", arrays))
        plan = host.instances()
        o, d = rays_for(mesh, plan, arrays, cases.family("identity", arrays), 3000, seed=23)
        oo, od = cases.odd_rays(plan["nodes"])
        o, d = cases.without_negative_zero(np.concatenate([o, oo]), np.concatenate([d, od]))
        for max_distance in (1e5, 0.3):
            for k in (4, 16):
                got = ask(host, o, d, max_distance, k)
                want = host.trace_multihit(o, d, max_distance, k=k)
                assert want["count"].any()
                for f in mo.FIELDS:
                    assert imo.same_words(got[f], want[f]).all(), (mesh, max_distance, k, f)
                used = want["leaf"] != NONE
                assert (got["instance"][used] == 0).all() and (got["instance"][~used] == NONE).all()
            assert np.array_equal(host.count_instances_hits(o, d, max_distance), host.count_hits(o, d, max_distance))
        host.set_instances(EMPTY)


@pytest.mark.parametrize("family", ["rotations", "tie_pair", "overlap_pair", "grid"])
def test_float64_comparator_gives_the_cpu_runs_report(rt, hosts, family):
    """The comparator on the GPU's answers reports what it reports on the oracle's (tests/test_instance_multihit_cpu.py)."""
    ref = None
    for bvh in ("longest", "sah"):
        host, scene, arrays = hosts("blob", bvh)
        W = cases.family(family, arrays)
        host.set_instances(W)
        plan = host.instances()
        o, d = cases.rays(plan["nodes"], 3000, seed=700 + cases.FAMILIES.index(family))
        max_distance = cases.MAX_DISTANCES[cases.FAMILIES.index(family) % 3]
        if ref is None:  # (the reference knows no tree: one answer for both builders)
            ref = imr.instanced(scene, W, o, d, max_distance)
        got = ask(host, o, d, max_distance, K)
        rep = imr.compare_multihit(scene, ref, got, K)
        print(f"INSTANCE MULTIHIT GPU blob/{bvh} {family} max_distance {max_distance}: {rep}")
        assert not rep.failures(tol=imr.TOL, max_unjudged=0.01), (family, bvh, rep.failures(tol=imr.TOL, max_unjudged=0.01))
        assert rep == imr.compare_multihit(scene, ref, imo.multihit(arrays, plan, o, d, max_distance, K), K), (family, bvh)
        host.set_instances(EMPTY)


def test_after_update_vertices_build_scene_and_a_new_upload(rt):
    scene = rc.fresh_scene(rt, "blob", "longest")
    host = new_host(rt, scene)
    arrays = orc.SceneArrays.from_scene(scene)
    W = cases.family("overlap_pair", arrays)
    host.set_instances(W)
    first = host.instances()
    moved = rc.steps("twist", scene.vertices)[-1]
    scene.refit(moved)
    host.update_vertices(moved, scene.vnormals)
    arrays = orc.SceneArrays.from_scene(scene)
    plan = host.instances()  # (the set persists; the tree is made again from the new root box)
    assert plan["nodes"].tobytes() != first["nodes"].tobytes()
    o, d = cases.rays(plan["nodes"], 2000, seed=59)
    got = check(host, imo.multihit(arrays, plan, o, d, 1e5, K), o, d, 1e5, 2000, K, what="updated")
    assert got["count"].max() >= 2
    # a build: the leaf order is the LBVH scene's
    v, f = bc.mesh("blob")
    built = bc.lbvh_scene(rt, "blob")
    host.build_scene(v, f, built.vnormals)
    arrays = orc.SceneArrays.from_scene(built)
    after = host.instances()
    o, d = cases.rays(after["nodes"], 2000, seed=67)
    check(host, imo.multihit(arrays, after, o, d, 1e5, K), o, d, 1e5, 2000, 5, what="built")
    # a new upload: the set is still there
    host.upload_scene(scene)
    arrays = orc.SceneArrays.from_scene(scene)
    again = host.instances()
    assert again["nodes"].tobytes() == plan["nodes"].tobytes()
    check(host, imo.multihit(arrays, again, o, d, 1e5, K), o, d, 1e5, 2000, K, sort=False, what="uploaded again")
    host.close()


def test_plain_multihit_and_frames_are_left_alone(rt, scene_for):
    """A plain trace_multihit and a rendered frame give the same bits before, during and after."""
    scene, arrays = scene_for("bunny", "longest")
    host = rt.Host(rt.Options.defaults(width=96, height=64, n_super_samples=4, ao_num_samples=3), 0)
    host.upload_scene(scene)
    host.render()
    before = host.download()
    stats = host.stats()
    probe = rt.instance_plan(*cases.root_box(arrays), cases.family("grid", arrays))
    o, d = cases.rays(probe["nodes"], 20000, seed=71)
    plain = host.trace_multihit(o, d, k=4)
    host.set_instances(cases.family("grid", arrays))
    plan = host.instances()
    first = ask(host, o, d, 1e5, 4)
    assert first["count"].any() and host.stats() == stats
    imo.assert_same(first, imo.multihit(arrays, plan, o, d, 1e5, 4), "grid of bunnies")
    for f in mo.FIELDS:
        assert imo.same_words(host.trace_multihit(o, d, k=4)[f], plain[f]).all(), ("plain, with a set", f)
    host.render()
    assert np.array_equal(bits(host.download()), bits(before))
    host.render_async()  # a frame left in flight while the queries run
    during = ask(host, o, d, 1e5, 4, sort=False)
    plain_during = host.trace_multihit(o, d, k=4)
    host.sync()
    assert np.array_equal(bits(host.download()), bits(before)) and host.stats() == stats
    imo.assert_same(during, first, "beside a frame")
    for f in mo.FIELDS:
        assert imo.same_words(plain_during[f], plain[f]).all(), ("plain, beside a frame", f)
    host.set_instances(EMPTY)
    for f in mo.FIELDS:
        assert imo.same_words(host.trace_multihit(o, d, k=4)[f], plain[f]).all(), ("plain, after", f)
    assert host.last_query_ms > 0.0
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
    host = new_host(rt)
    p = np.zeros((4, 3), np.float32)
    STATE, INVALID = api.RT_E_STATE, api.RT_E_INVALID
    W = cases.family("rotations", arrays)
    for call in (lambda: host.trace_instances_multihit(p, p), lambda: host.count_instances_hits(p, p)):
        with pytest.raises(rt.RtError) as e:  # no upload, no set
            call()
        assert e.value.code == STATE
    host.set_instances(W)
    with pytest.raises(rt.RtError) as e:  # a set, no upload
        host.trace_instances_multihit(p, p)
    assert e.value.code == STATE
    host.upload_scene(scene)
    host.set_instances(W[:0])
    with pytest.raises(rt.RtError) as e:  # an upload, no set
        host.count_instances_hits(p, p)
    assert e.value.code == STATE
    assert host.count_hits(p, p).shape == (4,)  # (the plain form needs none)
    host.set_instances(W)
    with pytest.raises(rt.RtError) as e:
        host.trace_instances_multihit(p, p, k=17)
    assert e.value.code == INVALID
    for outputs in (("count", "leaf"), ("instance",)):
        with pytest.raises(rt.RtError) as e:  # k == 0 asks for the count alone
            host.trace_instances_multihit(p, p, k=0, outputs=outputs)
        assert e.value.code == INVALID
    assert host.trace_instances_multihit(p, p, k=0, outputs=("count",))["count"].shape == (4,)
    p4 = np.zeros((4, 4), np.float32)
    at = p4.ctypes.data
    assert lib.rt_trace_instances_multihit(host._h, None, at, 4, 1.0, 2, 0, None) == INVALID
    assert lib.rt_trace_instances_multihit(host._h, at, None, 4, 1.0, 2, 0, None) == INVALID
    assert lib.rt_trace_instances_multihit_device(host._h, None, None, 4, 1.0, 2, 0, None, None) == INVALID
    assert lib.rt_trace_instances_multihit(host._h, None, None, 0, 1.0, 2, 0, None) == 0
    assert lib.rt_trace_instances_multihit(host._h, at, at, 4, 1.0, 2, 0, None) == 0  # (no outputs: nothing is written)
    assert lib.rt_trace_instances_multihit(host._h, at, at, (1 << 27) // 16 + 1, 1.0, 16, 0, None) == INVALID
    assert lib.rt_trace_instances_multihit(host._h, at, at, (1 << 27) + 1, 1.0, 0, 0, None) == INVALID
    assert lib.rt_trace_instances_multihit(None, at, at, 4, 1.0, 2, 0, None) == INVALID
    mem = _DeviceBytes(2 * 65 * 16 + 8192)
    a, b, out = mem.ptr.value, mem.ptr.value + 65 * 16, mem.ptr.value + 2 * 65 * 16

    def arrays_of(count=None, distance=None, instance=None):
        return C.byref(api._InstanceMultiHitArrays(api._MultiHitArrays(count, distance, None, None, None, None), instance))

    device = lib.rt_trace_instances_multihit_device
    assert device(host._h, a + 4, b, 64, 1.0, 2, 0, None, None) == INVALID
    assert device(host._h, a, b + 8, 64, 1.0, 2, 0, None, None) == INVALID
    assert device(host._h, a, b, 64, 1.0, 2, 0, arrays_of(count=out + 2), None) == INVALID
    assert device(host._h, a, b, 64, 1.0, 2, 0, arrays_of(distance=out + 1), None) == INVALID
    assert device(host._h, a, b, 64, 1.0, 2, 0, arrays_of(out, out + 1024, out + 2050), None) == INVALID  # `instance` off by two
    assert device(host._h, a, b, 64, 1.0, 0, 0, arrays_of(out, None, out + 2048), None) == INVALID  # k == 0 with `instance`
    assert device(host._h, a, b, 64, 1.0, 2, 0, arrays_of(out, out + 1024, out + 2048), None) == 0
    assert device(host._h, a, b, 64, 1.0, 0, 0, arrays_of(out), None) == 0
    assert host.last_query_ms >= 0.0  # (waits for the query)
    host.close()
    mem.free()
    ring = rt.FrameRing(rt.Options.defaults(width=32, height=32, ao_num_samples=3), hosts=2)
    ring.set_calibration(False)
    ring.upload_scene(scene)
    for call in (lambda: ring.host(0).trace_instances_multihit(p, p), lambda: ring.host(0).count_instances_hits(p, p)):
        with pytest.raises(rt.RtError) as e:
            call()
        assert e.value.code == STATE
    ring.close()


def test_torch_path_equals_numpy_path():
    """Device tensors in and device tensors out on a non-default stream == the numpy path
    (tests/instance_multihit_torch_driver.py, a child process that brings torch's runtime up before it loads the library)."""
    driver = os.path.join(os.path.dirname(os.path.abspath(__file__)), "instance_multihit_torch_driver.py")
    r = subprocess.run([sys.executable, driver], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "INSTANCE_MULTIHIT_TORCH_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
