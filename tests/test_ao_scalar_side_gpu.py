"""GPU: the scalar side of the ambient-occlusion pass's fast walk (kernels/walk.hip.h: the any-hit form of the node loop
and the turn around it in shared_walk_any_hit), bit for bit -- the float image's sha256, ao_occluded and primary_hits
against tests/golden/golden.json, or the float image, the 8-bit image and the four counters against the CPU oracle.

What the tests are about: the block itself asks whether a packet has a live lane left and whether its place lies before
the interval's end (no loop condition outside it); it compares with the end only where a miss jump or the step off a leaf
can land there, not where it descends to a first child; its three exits -- walk over, leaf tested on the spot, list full --
are the turn's only branches; the list limit stays in a register across the walk.  So the cases want: walks that end by
the step off a leaf and by a miss jump landing exactly on the end, whole-array intervals (a one-shot host's) and narrowed
ones (an announced stream's), every exit, packets that die in a batch or at a leaf and come back to the block with no
live lane, and both look-ahead forms.

  single_32_s1_a3       one triangle: the array is one leaf and END records; the walk ends by the step off that leaf
  ties_5x3_s1_a1        duplicated triangles, fifteen rays: several accepted pairs per ray
  ties_64_s4_a3         ... across exits: with everything listed (OCRT_BATCH_BELOW=65) they fall into one batch or two
  bunny_64_s1_a3        intervals that end behind their last leaf, and intervals an inner node's miss jump lands on
  bunny_256_s1_a3       the same, full and partial tiles, more than one workgroup per queue
  bunny_101x77_s9_a2    partly filled tiles: several table directions per packet, the tile's own interval
  blob_128x96_s4_a3     sparse: packets that end with a partial list

The knobs exist in the A/B build of the library only (lib_knobs); the environment is set with monkeypatch.
"""
import hashlib

import numpy as np
import pytest

import orc
from ao_direction_cases import ALL
from conftest import bits, options_for

pytestmark = pytest.mark.gpu

STREAM = 1000
GOLDEN_CASES = ["single_32_s1_a3", "ties_5x3_s1_a1", "ties_64_s4_a3", "bunny_64_s1_a3", "bunny_256_s1_a3", "bunny_101x77_s9_a2",
                "blob_128x96_s4_a3"]
KNOBS = [
    {"OCRT_BATCH_BELOW": "0"},    # nothing is ever listed: every leaf some lane hits is a "leaf now" exit
    {"OCRT_BATCH_BELOW": "65"},   # everything is listed: the block is left by "list full" and "over" only
    {"OCRT_AO_CLAIM_MAX": "1"},   # jobs are one packet long: the limit is fetched anew for every packet
    {"OCRT_AO_BLOCKS": "3"},      # three workgroups do the whole pass
]
_REF = {}


def assert_golden(host, case, what):
    st = host.stats()
    digest = hashlib.sha256(host.download().tobytes()).hexdigest()
    print(what, "ao_occluded", st["ao_occluded"], "golden", case["counters"]["ao_occluded"], "image equal", digest == case["float_sha256"])
    assert st["ao_occluded"] == case["counters"]["ao_occluded"], what
    assert st["primary_hits"] == case["counters"]["primary_hits"], what
    assert digest == case["float_sha256"], what


def hosts_of(rt, scene, opt):
    """A one-shot host (whole-array intervals) and an announced stream (narrowed ones), each with both look-ahead forms of
    the node loop."""
    for frames in (None, STREAM):
        for lookahead in (False, True):
            host = rt.Host(opt, 0)
            host.set_ao_prefetch(lookahead)
            if frames is not None:
                host.expect_frames(frames)
            host.upload_scene(scene)
            yield host, ("frames", frames, "look-ahead", lookahead)
            host.close()


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_golden_frames(rt, golden, scene_for, name):
    case = golden["renders"][name]
    scene, _ = scene_for(case["mesh"], case["bvh"])
    for host, what in hosts_of(rt, scene, options_for(rt, case)):
        for _ in range(2):  # (the second frame finds the waves' LDS slices as the first left them)
            host.render()
            assert_golden(host, case, (name,) + what)
        ends = host.walk_interval_ends()
        print(name, what, ends)
        # every interval a packet walks ends where a subtree does (or with the array): the premise of the unchecked descend
        assert ends["intervals"] > 0 and ends["after_inner"] == 0, (name, what, ends)
        assert ends["whole_array"] + ends["after_leaf"] == ends["intervals"], (name, what, ends)
        assert ends["last_is_leaf"] + ends["last_is_inner"] == ends["after_leaf"], (name, what, ends)
        if what[1] is None:
            assert ends["whole_array"] == ends["intervals"], (name, what, ends)  # a one-shot host narrows nothing
        elif name in ("bunny_64_s1_a3", "bunny_256_s1_a3"):
            # both ways of leaving a narrowed interval occur: behind its last leaf alone, and by a miss jump onto the end
            assert ends["last_is_leaf"] > 0 and ends["last_is_inner"] > 0, (name, what, ends)
        if name == "bunny_101x77_s9_a2":
            words = host.tile_order()["words"] & 0xFF
            assert ((words > 0) & (words < 64)).sum() > 0, "no partly filled tile: the case tests nothing"


@pytest.mark.parametrize("knobs", KNOBS, ids=["_".join(f"{k[5:].lower()}{v}" for k, v in kn.items()) for kn in KNOBS])
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_golden_frames_under_the_knobs(rt_knobs, golden, scene_for_knobs, name, knobs, monkeypatch):
    for key, value in knobs.items():
        monkeypatch.setenv(key, value)
    rt = rt_knobs
    case = golden["renders"][name]
    scene, _ = scene_for_knobs(case["mesh"], case["bvh"])
    for host, what in hosts_of(rt, scene, options_for(rt, case)):
        host.render()
        assert_golden(host, case, (name, knobs) + what)


def direction_options(rt, r, width, height):
    return rt.Options.defaults(width=width, height=height, n_super_samples=1, ao_num_samples=r.rings, ao_alpha_min=r.amin,
                               ao_alpha_max=r.amax, ao_max_distance=r.aod)


def reference(oracle, arrays, opt, key):
    """The oracle's frame for `key`, rendered once per session and never written to."""
    if key not in _REF:
        img, counters, _ = oracle.render(orc.params_from_options(opt), arrays)
        img.setflags(write=False)
        u8 = oracle.resize(img, opt.width, opt.height, opt.n_super_samples)
        u8.setflags(write=False)
        _REF[key] = (img, u8, counters)
    return _REF[key]


def assert_frame(host, ref, what):
    img, u8, counters = ref
    got = host.download()
    same = (bits(got) == bits(img)) | (np.isnan(got) & np.isnan(img))
    st = host.stats()
    print(what, "differing words", int((~same).sum()), "ao_occluded", st["ao_occluded"], "oracle", counters["ao_occluded"])
    assert same.all(), (what, int((~same).sum()), st["ao_occluded"], counters["ao_occluded"])
    assert np.array_equal(host.download_u8(), u8), what
    for k in ("primary_rays", "primary_hits", "ao_rays", "ao_occluded"):
        assert st[k] == counters[k], (what, k, st[k], counters[k])


# more packets per job, and pieces dealt by the cursor: 14 directions (even: half-tile claims) and 71 (odd, above a wave's 64
# lanes) on the bunny; oracle time per frame on 8 CPU threads 0.2 s at the most
@pytest.mark.parametrize("name", ["d14", "d71"])
def test_direction_counts(rt, oracle, scene_for, name):
    r = ALL[name]
    scene, arrays = scene_for("bunny", "longest")
    opt = direction_options(rt, r, 64, 48)
    ref = reference(oracle, arrays, opt, ("bunny", 64, 48, name))
    assert ref[2]["ao_rays"] == ref[2]["primary_hits"] * r.dirs and ref[2]["ao_occluded"] > 0
    for host, what in hosts_of(rt, scene, opt):
        host.render()
        assert_frame(host, ref, ("bunny", 64, 48, name) + what)
        ends = host.walk_interval_ends()
        assert ends["after_inner"] == 0, (name, what, ends)


def test_random_frame_under_its_statistical_bar(rt, oracle, scene_for):
    """AO_RANDOM (ao_kernel<2, false>) is outside the bit-exact contract (device and host libm round differently): the bar
    of tests/test_hip_parity.py, test_random_ao_statistical_parity, on the same frame."""
    samples = 16
    opt = rt.Options.defaults(width=160, height=120, n_super_samples=1, ao_num_samples=samples, ao_method=1, ao_max_distance=0.3)
    scene, arrays = scene_for("bunny", "longest")
    host = rt.Host(opt, 0)
    host.upload_scene(scene)
    host.render()
    gpu = host.download_u8().astype(np.int32)
    st = host.stats()
    host.close()
    ref_img, counters, _ = oracle.render(orc.params_from_options(opt), arrays)
    ref = oracle.resize(ref_img, opt.width, opt.height, 1).astype(np.int32)
    assert st["primary_hits"] == counters["primary_hits"]
    assert st["ao_rays"] == counters["ao_rays"] == counters["primary_hits"] * (samples + 2)
    delta = np.abs(gpu - ref)
    print("mean |delta|", delta.mean(), "identical", (delta == 0).mean(), "max", delta.max(), "occluded", st["ao_occluded"], counters["ao_occluded"])
    assert delta.mean() <= 0.25, delta.mean()
    assert (delta == 0).mean() >= 0.97, (delta == 0).mean()
    assert delta.max() <= 3 * 255 // (samples + 1) + 1, delta.max()
    assert abs(st["ao_occluded"] - counters["ao_occluded"]) <= 0.002 * counters["ao_rays"] + 8
