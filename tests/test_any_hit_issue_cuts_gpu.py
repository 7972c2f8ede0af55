"""GPU: the slow-class vector instructions taken out of the any-hit walk's append, packet head and batch code
(kernels/walk.hip.h: OCRT_APPEND_CURSOR, lane_of_tag; kernels/ao.hip.h: the packet's interval by one scalar load), bit for
bit -- the float image, the 8-bit image and the four counters against the CPU oracle, or the float image's sha256,
ao_occluded and primary_hits against tests/golden/golden.json.

What changed and what the cases want of it:

  the append     the list is kept by its next free byte address, not by a count: a leaf every lane hits appended behind 63
                 waiting pairs (127 entries, the leftovers move to the front), lists that are never used, packets that end
                 with a partial list, duplicated triangles (several accepted pairs per ray in one batch)
  the interval   two words by a scalar load from tile * stride + which: partly filled tiles (which = 0, several directions
                 in a packet), full tiles (a direction's own interval), a one-shot host (stride 1) and an announced stream
                 (stride 1 + directions), a group with a single tile; the ends are read back and held against the records
  the lane       out of the entries' tag where a batch is run, a leaf is tested on the spot and the leftovers move -- in
                 the RANDOM kernel by another instruction sequence than in the UNIFORM ones: one RANDOM frame

The eight-instruction node test the same change considered was not built (the probe measured it slower than the nine:
profiles/any_hit_issue_cuts_notes.md), so the node test has no new form to hold against the old ones here;
tests/test_node_test_forms_gpu.py keeps comparing the walk's form with the twelve-instruction one.

Oracle time per frame on 8 CPU threads: 0.5 s at the most (bunny 256 x 192, 71 directions); one render per (frame, count),
shared by all its cases.  The knobs exist in the A/B build of the library only (lib_knobs).
"""
import hashlib

import numpy as np
import pytest

import orc
from ao_direction_cases import ALL, rung
from conftest import bits, options_for

pytestmark = pytest.mark.gpu

STREAM = 1000
COUNTS = {"d14": ALL["d14"], "d28": rung(3, 28), "d71": ALL["d71"]}
# (24 x 16: a group with a single tile; 64 x 48: groups without any; 256 x 192: more than one workgroup per queue)
FRAMES = [("bunny", 64, 48), ("bunny", 24, 16), ("bunny", 256, 192), ("interior", 100, 68)]
_REF = {}


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


def assert_golden(host, case, what):
    st = host.stats()
    digest = hashlib.sha256(host.download().tobytes()).hexdigest()
    print(what, "ao_occluded", st["ao_occluded"], "golden", case["counters"]["ao_occluded"], "image equal", digest == case["float_sha256"])
    assert st["ao_occluded"] == case["counters"]["ao_occluded"], what
    assert st["primary_hits"] == case["counters"]["primary_hits"], what
    assert digest == case["float_sha256"], what


def hosts_of(rt, scene, opt):
    """A one-shot host (the tiles' own intervals only) and an announced stream (an interval per table direction too), each
    with both look-ahead forms of the node loop."""
    for frames in (None, STREAM):
        for lookahead in (False, True):
            host = rt.Host(opt, 0)
            host.set_ao_prefetch(lookahead)
            if frames is not None:
                host.expect_frames(frames)
            host.upload_scene(scene)
            yield host, ("frames", frames, "look-ahead", lookahead)
            host.close()


def case_of(rt, oracle, scene_for, mesh, width, height, name):
    r = COUNTS[name]
    scene, arrays = scene_for(mesh, "longest")
    opt = rt.Options.defaults(width=width, height=height, n_super_samples=1, ao_num_samples=r.rings, ao_alpha_min=r.amin,
                              ao_alpha_max=r.amax, ao_max_distance=r.aod)
    ref = reference(oracle, arrays, opt, (mesh, width, height, name))
    assert ref[2]["ao_rays"] == ref[2]["primary_hits"] * r.dirs and ref[2]["ao_occluded"] > 0
    return scene, opt, ref


@pytest.mark.parametrize("name", list(COUNTS))
@pytest.mark.parametrize("mesh,width,height", FRAMES)
def test_frames_against_the_oracle(rt, oracle, scene_for, mesh, width, height, name):
    scene, opt, ref = case_of(rt, oracle, scene_for, mesh, width, height, name)
    for host, what in hosts_of(rt, scene, opt):
        for _ in range(2):  # (the second frame finds the waves' LDS slices, the lists among them, as the first left them)
            host.render()
            assert_frame(host, ref, (mesh, width, height, name) + what)
        if (width, height) != (24, 16):
            words = host.tile_order()["words"] & 0xFF
            assert ((words > 0) & (words < 64)).any(), "no partly filled tile: the tile's own interval is not used"


def test_duplicated_triangles(rt, golden, scene_for):
    case = golden["renders"]["ties_64_s4_a3"]
    scene, _ = scene_for(case["mesh"], case["bvh"])
    for host, what in hosts_of(rt, scene, options_for(rt, case)):
        for _ in range(2):
            host.render()
            assert_golden(host, case, ("ties_64_s4_a3",) + what)


# The append at its limits.  OCRT_BATCH_BELOW=65: every leaf is appended, one hit by all 64 lanes too, so the list reaches
# 63 + 64 entries and the leftovers move; 0: nothing is ever appended, the cursor never leaves the list's head.
@pytest.mark.parametrize("below", ["65", "0"])
def test_the_list_at_its_limits_duplicated_triangles(rt_knobs, golden, scene_for_knobs, below, monkeypatch):
    monkeypatch.setenv("OCRT_BATCH_BELOW", below)
    case = golden["renders"]["ties_64_s4_a3"]
    scene, _ = scene_for_knobs(case["mesh"], case["bvh"])
    for host, what in hosts_of(rt_knobs, scene, options_for(rt_knobs, case)):
        for _ in range(2):
            host.render()
            assert_golden(host, case, ("ties_64_s4_a3", "OCRT_BATCH_BELOW", below) + what)


@pytest.mark.parametrize("below", ["65", "0"])
def test_the_list_at_its_limits_bunny(rt_knobs, oracle, scene_for_knobs, below, monkeypatch):
    monkeypatch.setenv("OCRT_BATCH_BELOW", below)
    scene, opt, ref = case_of(rt_knobs, oracle, scene_for_knobs, "bunny", 64, 48, "d14")
    for host, what in hosts_of(rt_knobs, scene, opt):
        for _ in range(2):
            host.render()
            assert_frame(host, ref, ("bunny", 64, 48, "d14", "OCRT_BATCH_BELOW", below) + what)


# jobs one packet long (a tile's set-up and a partial list's flush per packet); three workgroups do the whole pass
@pytest.mark.parametrize("knob,value", [("OCRT_AO_CLAIM_MAX", "1"), ("OCRT_AO_BLOCKS", "3")])
def test_short_jobs_and_few_workgroups(rt_knobs, oracle, scene_for_knobs, knob, value, monkeypatch):
    monkeypatch.setenv(knob, value)
    scene, opt, ref = case_of(rt_knobs, oracle, scene_for_knobs, "bunny", 64, 48, "d14")
    for host, what in hosts_of(rt_knobs, scene, opt):
        host.render()
        assert_frame(host, ref, ("bunny", 64, 48, "d14", knob, value) + what)


def test_random_frame_under_its_statistical_bar(rt, oracle, scene_for):
    """AO_RANDOM (ao_kernel<2, false>) shares the block, the append and the batch code, and has the lane number by its own
    instruction sequence.  It is outside the bit-exact contract (device and host libm round differently): the bar of
    tests/test_hip_parity.py, test_random_ao_statistical_parity, on the same frame."""
    samples = 16
    opt = rt.Options.defaults(width=160, height=120, n_super_samples=1, ao_num_samples=samples, ao_method=1, ao_max_distance=0.3)
    scene, arrays = scene_for("bunny", "longest")
    host = rt.Host(opt, 0)
    host.upload_scene(scene)
    host.render()
    gpu = host.download_u8().astype(np.int32)
    st = host.stats()
    host.close()
    _, ref_u8, counters = reference(oracle, arrays, opt, ("bunny", 160, 120, "random16"))
    ref = ref_u8.astype(np.int32)
    assert st["primary_hits"] == counters["primary_hits"]
    assert st["ao_rays"] == counters["ao_rays"] == counters["primary_hits"] * (samples + 2)
    delta = np.abs(gpu - ref)
    print("mean |delta|", delta.mean(), "identical", (delta == 0).mean(), "max", delta.max(), "occluded", st["ao_occluded"], counters["ao_occluded"])
    assert delta.mean() <= 0.25, delta.mean()
    assert (delta == 0).mean() >= 0.97, (delta == 0).mean()
    assert delta.max() <= 3 * 255 // (samples + 1) + 1, delta.max()
    assert abs(st["ao_occluded"] - counters["ao_occluded"]) <= 0.002 * counters["ao_rays"] + 8


@pytest.mark.parametrize("width,height", [(64, 48), (256, 192)])
def test_interval_ends(rt, oracle, scene_for, width, height):
    """What the packets' scalar load hands the walk is what the table holds: the frames are the oracle's, and every interval
    of the table ends where a subtree does (the premise of the node loop's unchecked descend), or with the array."""
    scene, opt, ref = case_of(rt, oracle, scene_for, "bunny", width, height, "d14")
    for host, what in hosts_of(rt, scene, opt):
        host.render()
        assert_frame(host, ref, ("bunny", width, height, "d14") + what)
        ends = host.walk_interval_ends()
        print(width, height, what, ends)
        assert ends["intervals"] > 0 and ends["after_inner"] == 0, (what, ends)
        assert ends["whole_array"] + ends["after_leaf"] == ends["intervals"], (what, ends)
        assert ends["last_is_leaf"] + ends["last_is_inner"] == ends["after_leaf"], (what, ends)
        if what[1] is None:
            assert ends["whole_array"] == ends["intervals"], (what, ends)  # a one-shot host narrows nothing
        else:
            assert ends["last_is_leaf"] > 0 and ends["last_is_inner"] > 0, (what, ends)
