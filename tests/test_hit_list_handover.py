"""GPU tests of the hand-over between the two ray passes: the hit list the primary pass writes and the ambient-occlusion
pass and the finishing kernel read, and the per-hit occlusion counts.  Frames of one scene are identical, so a frame that
leaned on what the one before it left in either could not be told from one that wrote them itself -- unless what it finds
there is garbage: every frame here starts from a POISONED hit list (rt_debug_poison_hit_list).  Bar: the golden bits,
which are the oracle's (tests/test_hip_parity.py)."""
import hashlib

import numpy as np
import pytest

from conftest import bits, options_for

pytestmark = pytest.mark.gpu

# a partial tile; one triangle; the supersampled finishing path; odd sizes with finish_wide_kernel; whole tiles
CASES = ["ties_5x3_s1_a1", "single_32_s1_a3", "blob_128x96_s4_a3", "bunny_101x77_s9_a2", "bunny_256_s1_a3"]


def poisoned_turns(rt, golden, scene_for, name, device_share=None):
    c = golden["renders"][name]
    opt = options_for(rt, c)
    scene, _ = scene_for(c["mesh"], c["bvh"])
    host = rt.Host(opt, 0)
    host.expect_frames(1000)
    host.upload_scene(scene)
    if device_share:
        host.set_device_share(device_share)
    host.render()
    for _ in range(4):
        host.poison_hit_list()
        host.render()
        assert hashlib.sha256(host.download().tobytes()).hexdigest() == c["float_sha256"]
        assert hashlib.md5(rt.pgm_bytes(host.download_u8())).hexdigest() == c["pgm_md5"]
    st = host.stats()
    assert st["primary_hits"] == c["counters"]["primary_hits"] and st["ao_occluded"] == c["counters"]["ao_occluded"]
    host.close()


@pytest.mark.parametrize("name", CASES)
def test_frames_after_a_poisoned_hit_list(rt, golden, scene_for, name):
    poisoned_turns(rt, golden, scene_for, name)


def test_frames_after_a_poisoned_hit_list_on_a_shared_device(rt, golden, scene_for):
    """(the smaller grid of the ambient-occlusion pass of a host that shares its GPU with two others)"""
    poisoned_turns(rt, golden, scene_for, "bunny_256_s1_a3", device_share=3)


def test_poisoned_frames_through_a_replayed_graph(rt, golden, scene_for):
    """A ring of one host replays ONE captured graph: nothing about the hit list can come in as an argument."""
    c = golden["renders"]["bunny_600_defaults"]
    opt = options_for(rt, c)
    scene, _ = scene_for(c["mesh"], c["bvh"])
    ring = rt.FrameRing(opt, scene, hosts=1)
    host = ring.host(0)
    for _ in range(3):
        host.poison_hit_list()
        ring.run(3)
        ring.drain()
        assert hashlib.md5(rt.pgm_bytes(ring.download_last())).hexdigest() == c["pgm_md5"]
        assert hashlib.sha256(host.download().tobytes()).hexdigest() == c["float_sha256"]
    ring.close()


def test_random_mode_frames_after_a_poisoned_hit_list(rt, scene_for):
    """The RANDOM sampler reads hit records a second time (the un-normalised normal of ray 0); its generator is seeded by
    pixel, so two frames of one host are the same bits -- also when the second starts from garbage."""
    scene, _ = scene_for("bunny", "longest")
    opt = rt.Options.defaults(width=64, height=64, n_super_samples=1, ao_method=1)
    host = rt.Host(opt, 0)
    host.upload_scene(scene)
    host.render()
    first, first_u8 = host.download().copy(), host.download_u8().copy()
    host.poison_hit_list()
    host.render()
    assert np.array_equal(bits(host.download()), bits(first))
    assert np.array_equal(host.download_u8(), first_u8)
    host.close()
