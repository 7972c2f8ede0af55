"""GPU: frames in which the closest-hit walk's pruning decides pixels (tests/prune_traps.py) -- a wrong growth of the leaves'
boxes (scene_pack.h, leaf_growth) or a wrong far_limit (kernels/primary.hip.h) changes them -- against the CPU oracles,
bit for bit: one-shot hosts (no pruning), stream hosts (pruning), a ring, tiles cast in quarters, each far_limit site
alone; and, on the A/B build, the teeth: with the growth multiplied by 0 the frame DOES differ, at trap pixels only."""
import numpy as np
import pytest

import camera_oracle as co
import orc
import prune_traps as pt
import query_oracle as qo
from conftest import bits

pytestmark = pytest.mark.gpu

STREAM = 16  # frames announced before the upload: the upload then grows the boxes and the primary pass prunes
CASES = ["a", "b", "c", "ties_needle_first", "ties_ordinary_first"]

_MESH, _WANT = {}, {}


def mesh_of(rt, case):
    if case not in _MESH:
        _MESH[case] = pt.ties_mesh(case == "ties_ordinary_first") if case.startswith("ties") else pt.trap_mesh(rt, case)
    return _MESH[case]


def camera_of(rt, case):
    """None: the reference's camera."""
    if case in ("b", "c"):
        p = pt.POSES[case]
        return rt.Camera.from_vectors(p[0], p[1], p[2], p[3])
    return None


def expected(rt, oracle, case):
    """(float image, 8-bit image, counters) of the CPU oracle -- oracle.render, the posed oracle for (b) and (c) --; once."""
    if case not in _WANT:
        vertices, faces, _ = mesh_of(rt, case)
        _, arrays = pt.product_scene(rt, vertices, faces)
        opt = pt.options(rt)
        params = orc.params_from_options(opt)
        if case in ("b", "c"):
            img, counters = co.render(params, arrays, pt.POSES[case])
        else:
            img, counters, _ = oracle.render(params, arrays)
        assert counters["primary_hits"] == pt.WIDTH * pt.HEIGHT  # (every pixel sees something: the frames have no background)
        _WANT[case] = (img, oracle.resize(img, opt.width, opt.height, opt.n_super_samples), counters)
    return _WANT[case]


def differing(host, want):
    got = host.download()
    return (bits(got) != bits(want[0])) & ~(np.isnan(got) & np.isnan(want[0]))


def assert_equals(host, want, what=""):
    wrong = differing(host, want)
    assert not wrong.any(), f"{what}: {int(wrong.sum())} float words differ from the oracle, first at {np.argwhere(wrong)[:4].tolist()}"
    assert np.array_equal(host.download_u8(), want[1]), what
    st = host.stats()
    for k in ("primary_rays", "primary_hits", "ao_rays", "ao_occluded"):
        assert st[k] == want[2][k], (what, k, st[k], want[2][k])


def make_host(rt, case, scene, stream):
    host = rt.Host(pt.options(rt), 0)
    if stream:
        host.expect_frames(STREAM)
    cam = camera_of(rt, case)
    if cam is not None:
        host.set_camera(cam)
    host.upload_scene(scene)
    return host


@pytest.mark.parametrize("case", CASES)
def test_trap_and_tie_frames_equal_the_oracle(rt, oracle, case):
    """One-shot host (prune_facts: infinite margin), stream host (finite), a ring of two hosts, and the stream host with its
    tiles cast in quarters from cost class 1, from 64 and not at all: floats, bytes and the four counters are the oracle's."""
    vertices, faces, _ = mesh_of(rt, case)
    scene, _ = pt.product_scene(rt, vertices, faces)
    want = expected(rt, oracle, case)
    host = make_host(rt, case, scene, stream=False)
    try:
        assert np.isinf(host.prune_facts()["prune_margin"])
        host.render()
        assert_equals(host, want, "one-shot")
    finally:
        host.close()
    host = make_host(rt, case, scene, stream=True)
    try:
        facts = host.prune_facts()
        assert np.isfinite(facts["prune_margin"]) and 0 < facts["prune_margin"] < 1e-2 and facts["primary_bytes"] > 0
        assert (facts["unpruned_bytes"] == 2 * 32) == case.startswith("ties")  # (the root and the needle; no such face in the traps)
        for again in range(2):
            host.render()
            assert_equals(host, want, "stream")
        for above in (1, 64, 0):
            host.set_primary_split(above)
            host.render()
            assert_equals(host, want, f"stream, primary split {above}")
    finally:
        host.close()
    ring = rt.FrameRing(pt.options(rt), scene, device=0, hosts=2, camera=camera_of(rt, case))
    try:
        for _ in range(3):
            ring.submit()
            assert np.array_equal(ring.collect(), want[1])
        ring.drain()
        for k in range(2):
            assert np.isfinite(ring.host(k).prune_facts()["prune_margin"])
            assert_equals(ring.host(k), want, f"ring host {k}")
    finally:
        ring.close()


def test_camera_rays_of_the_traps_through_the_queries(rt, oracle):
    """The camera rays of placement (a) through trace_closest -- queries do not prune: a second unpruned control on the same
    device -- give the stream host's frame, and the query oracle's leaves: the front triangles hit through the slack."""
    vertices, faces, _ = mesh_of(rt, "a")
    scene, arrays = pt.product_scene(rt, vertices, faces)
    opt = pt.options(rt, enable_ao=0)
    host = rt.Host(opt, 0)
    try:
        host.expect_frames(STREAM)
        host.upload_scene(scene)
        host.render()
        img = host.download()
        o4, d4 = qo.camera_rays(orc.params_from_options(opt))
        got = host.trace_closest(o4, d4, 100000.0)
        want = qo.closest(arrays, o4, d4, 100000.0)
        for f in ("hit", "distance", "leaf", "normal"):
            assert qo.same_words(got[f], want[f]).all(), f
        value = qo.shade(got["hit"], got["normal"], d4, True).reshape(img.shape)
        assert np.array_equal(bits(value), bits(img))
    finally:
        host.close()


@pytest.mark.parametrize("knobs", [
    {"OCRT_BATCH_BELOW": "0"},        # every leaf tested on the spot: the far_limit update after a leaf's own test alone
    {"OCRT_BATCH_BELOW": "65"},       # every triangle test deferred and batched: the update after a batch alone
    {"OCRT_KEEP_CHILD_ORDER": "1"},   # the builder's child order: hits arrive in another order
    {"OCRT_NO_PRUNE": "1"},           # no limit lowered at all
    {"OCRT_PRUNE_GROWTH": "1"},       # the growth's factor, at 1
])
@pytest.mark.parametrize("case", CASES)
def test_each_pruning_site_alone_equals_the_oracle(rt_knobs, oracle, case, knobs, monkeypatch):
    for key, value in knobs.items():
        monkeypatch.setenv(key, value)
    rt = rt_knobs
    vertices, faces, _ = mesh_of(rt, case)
    scene, _ = pt.product_scene(rt, vertices, faces)
    want = expected(rt, oracle, case)
    host = make_host(rt, case, scene, stream=True)
    try:
        assert np.isfinite(host.prune_facts()["prune_margin"]) == ("OCRT_NO_PRUNE" not in knobs)
        host.render()
        assert_equals(host, want, str(knobs))
    finally:
        host.close()


def test_without_the_growth_the_trap_pixels_change(rt_knobs, oracle, tmp_path, monkeypatch):
    """The teeth, on the A/B build: OCRT_PRUNE_GROWTH=0 leaves the leaves their own boxes, and the stream host's frame of
    placement (a) then differs from the oracle in at least one trap pixel -- so the frames above do reach the kernel's
    pruning -- and in no pixel that is neither a trap nor a neighbour that shares a trap's triangles."""
    rt = rt_knobs
    vertices, faces, _ = mesh_of(rt, "a")
    o4, d4 = pt.rays(rt, "a")
    f = pt.facts(pt.sweep_program(tmp_path), tmp_path, "a", vertices, faces, o4, d4)
    trap = f["trap"].reshape(pt.HEIGHT, pt.WIDTH)
    assert trap.sum() >= 0.9 * trap.size
    of_traps = {leaf for i in np.flatnonzero(f["trap"]) for leaf, _ in f["accepted"][i]}
    allowed = np.array([bool(f["trap"][i]) or any(leaf in of_traps for leaf, _ in f["accepted"][i]) for i in range(len(o4))]).reshape(trap.shape)
    want = expected(rt, oracle, "a")
    scene, _ = pt.product_scene(rt, vertices, faces)
    monkeypatch.setenv("OCRT_PRUNE_GROWTH", "0")
    host = make_host(rt, "a", scene, stream=True)
    try:
        assert np.isfinite(host.prune_facts()["prune_margin"])
        host.render()
        wrong = differing(host, want)
    finally:
        host.close()
    print(f"OCRT_PRUNE_GROWTH=0: {int(wrong.sum())} pixels differ from the oracle, {int((wrong & trap).sum())} of them traps ({int(trap.sum())} traps)")
    assert (wrong & trap).any(), "no trap pixel changed: the frame does not reach the kernel's pruning"
    assert not (wrong & ~allowed).any()
