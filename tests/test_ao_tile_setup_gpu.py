"""GPU: the ambient-occlusion pass's tile set-up, bit for bit against the CPU oracle (float image, 8-bit image, the four
ray counters) through every way a tile's table, walk intervals and table directions reach a wave (kernels/ao.hip.h):

  cursor claims          the workgroup's four waves share one tile and deal its directions out from a cursor in LDS
  fixed-share claims     every wave has tiles of its own (forced with the A/B build's OCRT_AO_CLAIM_MAX: whole tiles per
                         wave, and a claim size that runs over the tiles' ends)
  half-tile claims       the heaviest tiles, by measured cost (set_order_policy's split_above): a cursor of their own
  a one-shot host        entry_stride == 1: only the tile's own interval exists, the whole array
  an announced stream    1 + ao_dirs intervals per tile, narrowed per direction
  a ring of two hosts    frames in turn, one table of intervals for both
  AO_RANDOM              no direction table, the tile's own interval only

with 14, 71, 79 and 262 table directions (tests/ao_direction_cases.py: even and odd, below and above a wave's 64 lanes),
on frames with full and partial tiles: 256 x 192 and 64 x 48 of the bunny, 100 x 68 of the interior stand-in.  (Written
with the attempt to set a tile up once per workgroup -- profiles/ao_tile_setup_notes.md --; the paths are the pass's own.)

Which kind of claim a case takes is reasoned from the claim rule (ao_pass: a claim that lies in one tile is dealt by the
cursor, any other in fixed shares), not observed: the kernel reports no counter for it.  With OCRT_AO_CLAIM_MAX = ao_dirs a
claim is 4 * ao_dirs units = four tiles; with 5 it is 20 units, more than a tile at 14 directions and over a tile's end every
few claims at 71 and 79.  EMPTY intervals are not among the cases: a tile's region always holds the leaf its primary rays
hit (the origins' offset along the normal, 1e-5, is below the region's margin, 1 % of AO_MAX_DISTANCE -- entry.hip.h), so
entry_kernel never writes one; what is asserted is that intervals are narrowed, per tile and per direction.

Oracle time per frame on 8 CPU threads: bunny 256 x 192 at 79 directions ~0.5 s, every other less; one render per
(frame, count), shared by all its hosts.
"""
import numpy as np
import pytest

import orc
from ao_direction_cases import ALL
from conftest import bits

pytestmark = pytest.mark.gpu

STREAM = 1000
COUNTS = ["d14", "d71", "d79_alpha"]
FRAMES = [("bunny", 256, 192), ("bunny", 64, 48), ("interior", 100, 68)]
_REF = {}


def options(rt, r, width, height, **over):
    base = dict(width=width, height=height, n_super_samples=1, ao_num_samples=r.rings, ao_alpha_min=r.amin, ao_alpha_max=r.amax,
                ao_max_distance=r.aod)
    base.update(over)
    return rt.Options.defaults(**base)


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


def new_host(rt, scene, opt, frames=None):
    host = rt.Host(opt, 0)
    if frames is not None:
        host.expect_frames(frames)
    host.upload_scene(scene)
    return host


def case_of(rt, oracle, scene_for, mesh, width, height, name):
    r = ALL[name]
    scene, arrays = scene_for(mesh, "longest")
    opt = options(rt, r, width, height)
    ref = reference(oracle, arrays, opt, (mesh, width, height, name))
    assert ref[2]["ao_rays"] == ref[2]["primary_hits"] * r.dirs and ref[2]["ao_occluded"] > 0
    return r, scene, opt, ref


@pytest.mark.parametrize("name", COUNTS)
@pytest.mark.parametrize("mesh,width,height", FRAMES)
def test_one_shot_stream_and_half_tiles(rt, oracle, scene_for, mesh, width, height, name):
    r, scene, opt, ref = case_of(rt, oracle, scene_for, mesh, width, height, name)
    what = (mesh, width, height, name)
    # a one-shot host: the tiles' own intervals only, and those the whole array
    host = new_host(rt, scene, opt)
    host.render()
    assert_frame(host, ref, (what, "one-shot"))
    words = host.tile_order()["words"] & 0xFF
    full, partial = int((words == 64).sum()), int(((words > 0) & (words < 64)).sum())
    print(what, "full tiles", full, "partial tiles", partial)
    assert full > 0 and partial > 0, (what, full, partial)  # packets of one table direction, and of several
    host.close()
    # an announced stream: intervals per tile and table direction, narrower than the tile's own
    host = new_host(rt, scene, opt, STREAM)
    e = host.walk_entries()
    print(what, "intervals", e)
    assert e["tiles_narrowed"] > 0 and e["mean_packet_share"] <= e["mean_share"] < 1.0, (what, e)
    for _ in range(2):  # (the second frame finds the workgroup's LDS as the first left it)
        host.render()
        assert_frame(host, ref, (what, "stream"))
    # ... its heaviest tiles claimed half a tile at a time (even counts only: an odd one is never split)
    host.measure_tile_costs(2)
    host.set_order_policy(2.0, 2.0, 0.01)
    split = int(host.split_tiles().sum())
    assert (split >= 1) == (r.dirs % 2 == 0), (what, split)
    host.render()
    assert_frame(host, ref, (what, "split tiles", split))
    host.close()


def test_half_tiles_of_a_large_table(rt, oracle, scene_for):
    """262 directions, even: half-tile claims of 131, four packets' worth of intervals per lane."""
    r, scene, opt, ref = case_of(rt, oracle, scene_for, "bunny", 64, 48, "d262")
    host = new_host(rt, scene, opt, STREAM)
    host.render()
    assert_frame(host, ref, ("d262", "stream"))
    host.measure_tile_costs(2)
    host.set_order_policy(2.0, 2.0, 0.01)
    assert host.split_tiles().sum() >= 1
    host.render()
    assert_frame(host, ref, ("d262", "split"))
    host.close()


@pytest.mark.parametrize("name", COUNTS)
@pytest.mark.parametrize("claim", ["whole_tiles", "straddling", "single"])
def test_fixed_share_claims(rt_knobs, oracle, scene_for_knobs, name, claim, monkeypatch):
    """The A/B build's claim knob (the product library reads none).  OCRT_AO_CLAIM_MAX = ao_dirs: a claim of four whole
    tiles, one per wave -- fixed shares.  = 5: claims of 20 units, which lie in one tile (cursor) or run over its end (fixed
    shares, a wave's share going on in the next tile) by turns.  = 1: four units per claim, cursor claims but where ao_dirs
    is no multiple of four."""
    rt = rt_knobs
    r = ALL[name]
    monkeypatch.setenv("OCRT_AO_CLAIM_MAX", {"whole_tiles": str(r.dirs), "straddling": "5", "single": "1"}[claim])
    for mesh, width, height in (("bunny", 64, 48), ("interior", 100, 68)):
        _, scene, opt, ref = case_of(rt, oracle, scene_for_knobs, mesh, width, height, name)
        for frames in (None, STREAM):
            host = new_host(rt, scene, opt, frames)
            host.render()
            assert_frame(host, ref, (mesh, name, claim, "frames", frames))
            host.close()


@pytest.mark.parametrize("name", COUNTS)
def test_ring_of_two_hosts(rt, oracle, scene_for, name):
    """Two hosts taking frames in turn on one table of intervals (a ring measures the tiles' costs and splits by itself)."""
    r, scene, opt, ref = case_of(rt, oracle, scene_for, "bunny", 256, 192, name)
    ring = rt.FrameRing(opt, None, hosts=2)
    ring.upload_scene(scene)
    for _ in range(4):
        ring.submit()
        assert np.array_equal(ring.collect(), ref[1]), name
    ring.drain()
    img, _, counters = ref
    for k in range(2):
        host = ring.host(k)
        got = host.download()
        assert ((bits(got) == bits(img)) | (np.isnan(got) & np.isnan(img))).all(), (name, "ring host", k)
        st = host.stats()
        for key in ("primary_rays", "primary_hits", "ao_rays", "ao_occluded"):
            assert st[key] == counters[key], (name, "ring host", k, key, st[key], counters[key])
    ring.close()


@pytest.mark.parametrize("mesh,width,height", FRAMES[1:])
def test_random_sampler(rt, scene_for, mesh, width, height):
    """AO_RANDOM: the device's libm is outside the bit-exact contract with the CPU, so the frame is compared with itself
    across the kinds of claims (one-shot, stream, split tiles)."""
    scene, _ = scene_for(mesh, "longest")
    opt = rt.Options.defaults(width=width, height=height, n_super_samples=1, ao_num_samples=16, ao_method=1)
    host = new_host(rt, scene, opt)
    host.render()
    plain, st = host.download(), host.stats()
    assert st["primary_hits"] > 0 and st["ao_rays"] == st["primary_hits"] * (16 + 2) and st["ao_occluded"] > 0
    host.close()
    host = new_host(rt, scene, opt, STREAM)
    host.render()
    assert np.array_equal(bits(host.download()), bits(plain)) and host.stats()["ao_occluded"] == st["ao_occluded"]
    host.measure_tile_costs(2)
    host.set_order_policy(2.0, 2.0, 0.01)
    host.render()
    assert np.array_equal(bits(host.download()), bits(plain)) and host.stats()["ao_occluded"] == st["ao_occluded"]
    host.close()
