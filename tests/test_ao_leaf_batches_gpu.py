"""GPU: the leaf tests of the ambient-occlusion pass's fast walk (kernels/walk.hip.h: run_batch and the leaf tested on
the spot), bit for bit -- the float image's sha256 and ao_occluded against tests/golden/golden.json, or the float image,
the 8-bit image and the four counters against the CPU oracle.

What the tests are about: a ray is occluded by a candidate pair iff the leaf's OWN box passes and the triangle is
accepted.  The pass runs the triangle test first and looks at the box only in a batch (or at a leaf) where some lane
accepted; whatever follows a batch -- the occluded bits, the counts, the live mask -- is skipped where none did.  So the
cases want: batches with and without accepted pairs, full and partial (the flush at a packet's end), leaves tested on
the spot, rays with MORE than one accepted pair (counted once), and partly filled tiles.

  bunny_256_s1_a3       full and partial tiles, the usual mix of batches and leaves tested on the spot
  blob_128x96_s4_a3     sparse: most packets end with fewer than 64 pairs waiting
  ties_64_s4_a3         duplicated triangles: an occluded ray has two accepted pairs, which with everything listed
                        (OCRT_BATCH_BELOW=65) fall into one batch or into two -- the trap for double counting
  bunny_101x77_s9_a2    partly filled tiles: packets of several table directions

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
GOLDEN_CASES = ["bunny_256_s1_a3", "blob_128x96_s4_a3", "ties_64_s4_a3", "bunny_101x77_s9_a2"]
KNOBS = [
    {"OCRT_BATCH_BELOW": "0"},    # nothing is ever listed: every leaf is tested on the spot
    {"OCRT_BATCH_BELOW": "65"},   # everything is listed: batches only, and on the sparse blob mostly partial ones
    {"OCRT_AO_CLAIM_MAX": "1"},   # jobs are one packet long: every packet flushes, every job starts from cleared bits
    {"OCRT_AO_BLOCKS": "3"},      # three workgroups do the whole pass: the same LDS slices serve every tile in turn
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
    """A one-shot host and an announced stream, each with both look-ahead forms of the node loop."""
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
# lanes), on frames with full and partly filled tiles; oracle time per frame on 8 CPU threads 0.2 s at the most
@pytest.mark.parametrize("name", ["d14", "d71"])
@pytest.mark.parametrize("mesh,width,height", [("bunny", 64, 48), ("ties", 33, 21)])
def test_direction_counts(rt, oracle, scene_for, mesh, width, height, name):
    r = ALL[name]
    scene, arrays = scene_for(mesh, "longest")
    opt = direction_options(rt, r, width, height)
    ref = reference(oracle, arrays, opt, (mesh, width, height, name))
    assert ref[2]["ao_rays"] == ref[2]["primary_hits"] * r.dirs and ref[2]["ao_occluded"] > 0
    for host, what in hosts_of(rt, scene, opt):
        host.render()
        assert_frame(host, ref, (mesh, width, height, name) + what)


@pytest.mark.parametrize("knobs", KNOBS[:2], ids=["batch_below0", "batch_below65"])
@pytest.mark.parametrize("name", ["d14", "d71"])
def test_direction_counts_listed_and_unlisted(rt_knobs, oracle, scene_for_knobs, name, knobs, monkeypatch):
    for key, value in knobs.items():
        monkeypatch.setenv(key, value)
    rt = rt_knobs
    r = ALL[name]
    scene, arrays = scene_for_knobs("ties", "longest")
    opt = direction_options(rt, r, 33, 21)
    ref = reference(oracle, arrays, opt, ("ties", 33, 21, name))
    for host, what in hosts_of(rt, scene, opt):
        host.render()
        assert_frame(host, ref, ("ties", name, knobs) + what)


def test_random_frame_under_its_statistical_bar(rt, oracle, scene_for):
    """AO_RANDOM is outside the bit-exact contract (device and host libm round differently): the bar of
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
