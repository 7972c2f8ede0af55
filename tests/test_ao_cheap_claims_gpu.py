"""GPU: the cheap suffix of the ambient-occlusion pass's claim lists (kernels/ao.hip.h, the claim step; DeviceRenderer::
orderByMeasuredCost, rule 5), bit for bit against the CPU oracle: float image, 8-bit image, the four ray counters.

Behind `GroupQueue::cheap_from` a claim is four whole tiles, one per wave, in fixed shares; in front of it a claim is one
tile shared by the four waves (or half a tile, for the split prefix).  The boundary is set with rt_debug_set_cheap_claims:

  0        no region: rt_debug_cheap_tiles reports 0 everywhere and the lists are the ones made without the rule
  0.15     the default (what a measurement installs by itself): on the headline frame, the ground-plane tiles
  0.25     the boundary below which rule 3 of the order moves a tile to the list's end anyway
  1e30     every tile that is not split: whole lists claimed a tile per wave -- group lists whose lengths are no multiples
           of four (the last claim finds fewer than four tiles, waves of it find nothing), partly filled tiles in the region

on the small frames the suite already uses: the bunny at 256 x 192 and 64 x 48, the interior stand-in at 100 x 68 and
`ties_64_s4_a3` (duplicated triangles), with 14, 28 and 71 directions.  (The 64 x 48 frame's groups hold 8, 10, 9 and 6
tiles and four hold none: its last claims are short, but no list is shorter than a claim; a 24 x 16 frame, whose second
group has two slots, is there for that.)  At 14 and 71 a
claim of 4 x ao_dirs units that follows claims of another size begins inside a tile; nothing is asserted about that, only
the image.  Which path ran is asserted from rt_debug_cheap_tiles and rt_debug_split_tiles, never from the image.

Measured costs are device-clock times and differ from run to run; the test of rt_debug_measure_tile_costs that exists
(tests/test_hip_parity.py, test_measured_tile_order_changes_nothing) has no tolerance for them.  So the case that measures
again with a region installed asserts what is exact: without `reorder` the list, its split prefix and its region come out
as they went in, every tile with work has a cost, and the frame is the oracle's; the ratio of the two measurements is
printed and not asserted.

Oracle time per frame on 8 CPU threads: 0.5 s at the most (bunny 256 x 192, 71 directions); one render per (frame, count),
shared by all its cases.
"""
import numpy as np
import pytest

import orc
from ao_direction_cases import ALL, rung
from conftest import bits, options_for

pytestmark = pytest.mark.gpu

STREAM = 1000
EVERYTHING = 1e30
COUNTS = {"d14": ALL["d14"], "d28": rung(3, 28), "d71": ALL["d71"]}
FRAMES = [("bunny", 256, 192), ("bunny", 64, 48), ("interior", 100, 68)]
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


def case_of(rt, oracle, scene_for, mesh, width, height, name):
    r = COUNTS[name]
    scene, arrays = scene_for(mesh, "longest")
    opt = rt.Options.defaults(width=width, height=height, n_super_samples=1, ao_num_samples=r.rings, ao_alpha_min=r.amin,
                              ao_alpha_max=r.amax, ao_max_distance=r.aod)
    ref = reference(oracle, arrays, opt, (mesh, width, height, name))
    assert ref[2]["ao_rays"] == ref[2]["primary_hits"] * r.dirs and ref[2]["ao_occluded"] > 0
    return scene, opt, ref


def measured_stream_host(rt, scene, opt, split_above=0.0):
    """An announced stream with measured costs.  On frames this small every tile costs more than a quarter of the pass's
    ideal length (a group's cost over its 256 workgroups), so the default policy splits them all and leaves the region
    nothing: the cases that are about the region alone turn the splitting off (`split_above` 0)."""
    host = rt.Host(opt, 0)
    host.expect_frames(STREAM)
    host.upload_scene(scene)
    assert host.cheap_tiles().sum() == 0  # (nothing measured yet: no region)
    host.measure_tile_costs(2)
    host.set_order_policy(2.0, 2.0, split_above)
    return host


def through_the_boundaries(host, ref, what):
    """The frame with the region as the measurement installed it, then off, at the default by name, at rule 3's quarter and
    over every unsplit tile; returns the tiles in the region at each."""
    host.render()
    assert_frame(host, ref, (what, "as measured"))
    info = host.tile_order()
    work = info["constants"][:, 0].astype(np.int64)
    words = info["words"] & 0xFF
    counts = {}
    for boundary in (0.0, 0.15, 0.25, EVERYTHING):
        host.set_cheap_claims(boundary)
        cheap, split = host.cheap_tiles().astype(np.int64), host.split_tiles().astype(np.int64)
        after = host.tile_order()
        print(what, "cheap_below", boundary, "tiles per group", work.tolist(), "cheap", cheap.tolist(), "split", split.tolist())
        assert np.array_equal(after["constants"], info["constants"])
        assert sorted(after["order"].tolist()) == sorted(info["order"].tolist())  # (the same entries in some order)
        assert (cheap + split <= work).all(), (what, boundary)
        if boundary == 0.0:
            assert cheap.sum() == 0, (what, cheap)
        if boundary == EVERYTHING:
            assert np.array_equal(cheap, work - split) and cheap.sum() > 0, (what, cheap, work, split)
        for _ in range(2):  # (the second frame finds the queues and the workgroups' LDS as the first left them)
            host.render()
            assert_frame(host, ref, (what, "cheap_below", boundary))
        counts[boundary] = int(cheap.sum())
    return counts, work, words


@pytest.mark.parametrize("name", list(COUNTS))
@pytest.mark.parametrize("mesh,width,height", FRAMES)
def test_region_off_default_and_everywhere(rt, oracle, scene_for, mesh, width, height, name):
    scene, opt, ref = case_of(rt, oracle, scene_for, mesh, width, height, name)
    what = (mesh, width, height, name)
    host = measured_stream_host(rt, scene, opt)
    counts, work, words = through_the_boundaries(host, ref, what)
    host.close()
    # what the frames are here for: lists that are no multiple of four long (waves of the last claim find nothing) and
    # partly filled tiles in the region; at 64 x 48 also groups without any tile
    assert (work % 4 != 0).any(), (what, work)
    assert ((words > 0) & (words < 64)).any(), what
    if (width, height) == (64, 48):
        assert (work == 0).any(), (what, work)


def test_groups_shorter_than_a_claim(rt, oracle, scene_for):
    """24 x 16: three by two tiles, so the second group's list has two slots: a claim of four tiles finds at most two."""
    scene, opt, ref = case_of(rt, oracle, scene_for, "bunny", 24, 16, "d14")
    host = measured_stream_host(rt, scene, opt)
    counts, work, words = through_the_boundaries(host, ref, ("bunny", 24, 16, "d14"))
    host.close()
    assert ((work > 0) & (work < 4)).any(), work


def test_ties_golden_frame(rt, golden, oracle, scene_for):
    """`ties_64_s4_a3`: 28 directions, four sub-pixels per pixel, duplicated triangles (an occluded ray has two accepted pairs)."""
    case = golden["renders"]["ties_64_s4_a3"]
    scene, arrays = scene_for(case["mesh"], case["bvh"])
    opt = options_for(rt, case)
    ref = reference(oracle, arrays, opt, "ties_64_s4_a3")
    assert ref[2]["ao_occluded"] == case["counters"]["ao_occluded"] and ref[2]["primary_hits"] == case["counters"]["primary_hits"]
    host = measured_stream_host(rt, scene, opt)
    through_the_boundaries(host, ref, "ties_64_s4_a3")
    host.close()


@pytest.mark.parametrize("boundary", [0.15, EVERYTHING])
def test_split_prefix_and_cheap_suffix_together(rt, oracle, scene_for, boundary):
    """Half-tile claims from their own cursor at the head of a list, whole tiles per wave at its end, in one frame: 14
    directions (even: tiles can be split; a half is 7 units, a cheap claim 56)."""
    scene, opt, ref = case_of(rt, oracle, scene_for, "bunny", 256, 192, "d14")
    host = measured_stream_host(rt, scene, opt)
    host.set_cheap_claims(boundary)
    # the threshold of the split prefix, lowered from out of reach until a list has both (the default, a quarter of the
    # pass's ideal length, splits every tile of a frame this small: see measured_stream_host)
    for split_above in (64.0, 32.0, 16.0, 8.0, 4.0, 2.0, 1.0):
        host.set_order_policy(2.0, 2.0, split_above)
        split, cheap = host.split_tiles().astype(np.int64), host.cheap_tiles().astype(np.int64)
        if ((split > 0) & (cheap > 0)).any():
            break
    work = host.tile_order()["constants"][:, 0]
    print("split_above", split_above, "split", split.tolist(), "cheap", cheap.tolist(), "tiles", work.tolist())
    assert split.sum() > 0 and cheap.sum() > 0, (split, cheap)
    assert ((split > 0) & (cheap > 0)).any() and (split + cheap <= work).all(), (split, cheap, work)
    for _ in range(2):
        host.render()
        assert_frame(host, ref, ("split and cheap", boundary))
    host.close()


def test_ring_of_two_hosts(rt, oracle, scene_for):
    """A ring measures by itself and hands list, split prefix and region to every host; the hosts share the device."""
    scene, opt, ref = case_of(rt, oracle, scene_for, "bunny", 256, 192, "d28")
    ring = rt.FrameRing(opt, None, hosts=2)
    ring.upload_scene(scene)
    assert np.array_equal(ring.host(0).cheap_tiles(), ring.host(1).cheap_tiles())
    assert np.array_equal(ring.host(0).tile_order()["order"], ring.host(1).tile_order()["order"])
    for boundary in (None, EVERYTHING):
        if boundary is not None:
            ring.drain()
            for k in range(2):
                ring.host(k).set_order_policy(2.0, 2.0, 0.0)  # (no split prefix: see measured_stream_host)
                ring.host(k).set_cheap_claims(boundary)
                assert ring.host(k).cheap_tiles().sum() > 0
        for _ in range(4):
            ring.submit()
            assert np.array_equal(ring.collect(), ref[1]), boundary
        ring.drain()
        for k in range(2):
            assert_frame(ring.host(k), ref, ("ring host", k, boundary))
    ring.close()


def test_random_frame_under_its_statistical_bar(rt, oracle, scene_for):
    """AO_RANDOM is outside the bit-exact contract (device and host libm round differently): the bar of
    tests/test_hip_parity.py, test_random_ao_statistical_parity, on the same frame, every unsplit tile in the region."""
    samples = 16
    opt = rt.Options.defaults(width=160, height=120, n_super_samples=1, ao_num_samples=samples, ao_method=1, ao_max_distance=0.3)
    scene, arrays = scene_for("bunny", "longest")
    host = measured_stream_host(rt, scene, opt)
    host.set_cheap_claims(EVERYTHING)
    assert host.cheap_tiles().sum() > 0
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


def test_one_shot_host_has_no_region(rt, oracle, scene_for):
    """No measured costs, no region -- whatever the boundary is set to."""
    scene, opt, ref = case_of(rt, oracle, scene_for, "bunny", 64, 48, "d14")
    host = rt.Host(opt, 0)
    host.upload_scene(scene)
    assert host.cheap_tiles().sum() == 0
    host.render()
    assert_frame(host, ref, "one-shot")
    host.set_cheap_claims(EVERYTHING)
    assert host.cheap_tiles().sum() == 0
    host.render()
    assert_frame(host, ref, "one-shot, boundary set")
    host.close()


def test_measuring_again_with_a_region_installed(rt, oracle, scene_for):
    """Measuring frames claim as if there were no region (a tile's cost is what ITS claims took), and a measurement without
    `reorder` leaves list, split prefix and region as they were (see the module's docstring for what is not asserted)."""
    scene, opt, ref = case_of(rt, oracle, scene_for, "bunny", 256, 192, "d14")
    host = measured_stream_host(rt, scene, opt)
    host.set_cheap_claims(0.0)
    host.measure_tile_costs(2, reorder=False)
    without = host.tile_order()
    host.set_cheap_claims(EVERYTHING)
    before, split, cheap = host.tile_order(), host.split_tiles(), host.cheap_tiles()
    assert split.sum() == 0 and cheap.sum() > 0
    host.measure_tile_costs(2, reorder=False)
    after = host.tile_order()
    assert np.array_equal(after["order"], before["order"]) and np.array_equal(after["constants"], before["constants"])
    assert np.array_equal(host.split_tiles(), split) and np.array_equal(host.cheap_tiles(), cheap)
    work = after["words"] >> 8 != 0
    assert work.any() and (after["costs"][work] > 0).all() and (after["costs"][~work] == 0).all()
    ratio = after["costs"][work] / without["costs"][work]
    print("costs with the region installed / without: median", float(np.median(ratio)), "min", float(ratio.min()), "max", float(ratio.max()))
    host.render()
    assert_frame(host, ref, "after measuring with the region installed")
    # ... and with `reorder` the region is made again from the new costs, by the boundary in force
    host.measure_tile_costs(2)
    assert np.array_equal(host.cheap_tiles().astype(np.int64), host.tile_order()["constants"][:, 0] - host.split_tiles().astype(np.int64))
    host.render()
    assert_frame(host, ref, "measured and ordered again")
    host.close()
