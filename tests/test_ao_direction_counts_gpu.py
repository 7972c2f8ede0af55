"""GPU: the ambient-occlusion pass across direction counts -- 4 to 34986 table directions per hit -- bit for bit against
the CPU oracle: float image (a NaN on both sides is equal), 8-bit image and the four ray counters, through every kind of
host.  Which counts and why: tests/ao_direction_cases.py (tests/test_ao_direction_counts_cpu.py pins them).

Oracle time per case, measured on 8 CPU threads (one render per rung, shared by all the hosts of the rung):
blob 25 x 17 (237 hits) d32168 0.61 s, d32526_alpha 0.60 s, d32719 0.59 s, d33283 0.58 s, d34986 0.66 s (8.3 M rays); every
small rung 0.05 s or less, on ties too; the claim-size frames: beside their cases below; the AO queries' 65 points at 34986 rays each: below 0.3 s.
"""
import numpy as np
import pytest

import ao_oracle as aoo
import orc
from ao_direction_cases import ALL, LARGE, LIMIT, SMALL
from conftest import bits

pytestmark = pytest.mark.gpu

STREAM = 1000
# blob at 25 x 17: 4 x 3 tiles of 8 x 8 sub-pixels, among them a full one (64 hits), tiles with 4, 5, 8 and 11 hits and one
# with exactly 1 -- the cursor's piece is 64 >> floor(log2(hit count)) directions: 1, 16, 8, 64; asserted in frame_of().
# ties at 33 x 21: two full tiles and tiles of 7 .. 30 hits.
FRAMES = {"blob": (25, 17), "ties": (33, 21)}
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


def new_host(rt, scene, opt, frames=None, rank=0, nranks=1, before_upload=None):
    host = rt.Host(opt, 0, rank, nranks)
    if frames is not None:
        host.expect_frames(frames)
    if before_upload:
        before_upload(host)
    host.upload_scene(scene)
    return host


def every_host(rt, scene, opt, r, ref, what):
    # one-shot, and a stream announced
    for frames in (None, STREAM):
        host = new_host(rt, scene, opt, frames)
        host.render()
        assert_frame(host, ref, (what, "frames", frames))
        if frames is None:
            words = host.tile_order()["words"] & 0xFF
        host.close()
    # measured costs, and the heaviest tiles claimed half a tile at a time from a threshold down
    host = new_host(rt, scene, opt, STREAM)
    host.render()
    host.measure_tile_costs(2)
    assert host.tile_order()["costs"].max() > 0
    for split_above in (0.01, 0.25, 1e9, 0.0):
        host.set_order_policy(2.0, 2.0, split_above)
        split = int(host.split_tiles().sum())
        if split_above == 0.01 and r.dirs % 2 == 0 and r.dirs < LIMIT:
            assert split >= 1, (what, "no tile is split: the case tests nothing")
        if split_above in (1e9, 0.0) or r.dirs % 2 == 1:
            assert split == 0, (what, split_above, split)
        if r.dirs >= LIMIT:
            # from 0x8000 directions on the pass has no cursor to end a half-tile claim with (its word holds 15 bits), and
            # fixed shares overran the half where it is no multiple of 4: no tile is split there (tile_order.cc)
            assert split == 0, (what, split_above, split)
        host.render()
        assert_frame(host, ref, (what, "split_above", split_above, "split tiles", split))
    host.close()
    # beside other hosts' frames (smaller grid, another claim rule); primary tiles in quarters
    host = new_host(rt, scene, opt, STREAM, before_upload=lambda h: h.set_device_share(3))
    host.render()
    assert_frame(host, ref, (what, "device share 3"))
    host.close()
    host = new_host(rt, scene, opt)
    host.set_primary_split(1)
    host.render()
    assert_frame(host, ref, (what, "primary split 1"))
    host.close()
    # the bands of three ranks, reassembled
    img, u8, counters = ref
    seen = np.zeros(opt.height, dtype=bool)
    sums = dict.fromkeys(("primary_hits", "ao_rays", "ao_occluded"), 0)
    for rank in range(3):
        part = new_host(rt, scene, opt, rank=rank, nranks=3)
        part.render()
        rows = part.local_to_global_rows()
        keep = rows < opt.height
        assert np.array_equal(part.download_u8_local()[keep], u8[rows[keep]]), (what, "rank", rank)
        got = part.download()[rows[keep]]
        want = img[rows[keep]]
        assert ((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all(), (what, "rank", rank)
        seen[rows[keep]] = True
        st = part.stats()
        for k in sums:
            sums[k] += st[k]
        part.close()
    assert seen.all()
    for k in sums:
        assert sums[k] == counters[k], (what, "ranks", k)
    return words


def frame_of(rt, oracle, scene_for, mesh, name):
    r = ALL[name]
    scene, arrays = scene_for(mesh, "longest")
    w, h = FRAMES[mesh]
    opt = options(rt, r, w, h)
    return r, scene, opt, reference(oracle, arrays, opt, (mesh, name, w, h))


@pytest.mark.parametrize("name", list(SMALL) + list(LARGE))
def test_ladder_on_blob(rt, oracle, scene_for, name):
    r, scene, opt, ref = frame_of(rt, oracle, scene_for, "blob", name)
    assert ref[2]["ao_rays"] == ref[2]["primary_hits"] * r.dirs
    words = every_host(rt, scene, opt, r, ref, name)
    # tiles of more than one hit count: a full one, a handful, exactly one
    counts = set(words.tolist())
    assert 64 in counts and 1 in counts and counts & {3, 4, 5, 6, 7}, sorted(counts)


@pytest.mark.parametrize("name", list(SMALL))
def test_small_rungs_on_ties(rt, oracle, scene_for, name):
    r, scene, opt, ref = frame_of(rt, oracle, scene_for, "ties", name)
    every_host(rt, scene, opt, r, ref, ("ties", name))


def claim_rule(constants, tiles, dirs, workgroups):
    """ao_kernel's claim size per group, restated: which branch of its rule each group with work takes.  launch_ao starts
    min(workgroups, ceil(tiles * dirs / 4)) workgroups of 4 waves; a group's waves = ceil(4 * that / 8) (`claim_div`); the
    group's units = its tiles with hits * dirs; per wave = units / claim_div; a whole tile per wave where the group's mean
    cost class is below 8 and units >= 512 * claim_div, else a third of a quarter below 12 per wave, half a quarter below
    24, a quarter from there."""
    blocks = min(workgroups, -(-tiles * dirs // 4))
    div = max(1, -(-4 * blocks // 8))
    taken = {}
    for g in range(8):
        work, cost = int(constants[g][0]), int(constants[g][1])
        if work == 0:
            continue
        units = work * dirs
        per_wave = units // div
        branch = ("whole_tile" if cost < 8 * work and units >= 512 * div else "third" if per_wave < 12 else
                  "half" if per_wave < 24 else "quarter")
        taken.setdefault(branch, []).append((g, work, per_wave))
    return taken


# An MI355X has 256 compute units and a host alone launches 8 workgroups on each: 2048, so claim_div = 4 * 2048 / 8 = 1024
# as soon as tiles * dirs >= 8192.  Per wave = (group's tiles with hits, W) * dirs / 1024.  A group is every eighth pair
# of tile columns; W below is counted from the oracle's hit image.
#   371 directions: a third below 12 per wave = W <= 33 (33 * 371 = 12243 -> 11), half a quarter up to W = 66 (24486 -> 23),
#     a quarter from W = 67 (24857 -> 24).  blob 192 x 144: W = 24 .. 41 -> 8, 11 and 14 per wave, a third and a half; blob
#     288 x 216: W = 66 .. 84 -> 23 .. 30, a half and a quarter.
#   2206 directions: a third up to W = 5 (11030 -> 10), half a quarter for W = 6 .. 11 (13236 -> 12, 24266 -> 23), a
#     quarter from W = 12 (26472 -> 25).  blob 72 x 48: W = 4, 12, 12, 8, 2 -> 8, 25, 25, 17, 4: all three; blob 80 x 48:
#     W = 4, 11, 12, 11, 4 -> 8, 23, 25, 23, 8: both sides of 24; blob 48 x 32: W = 6, 8, 6 -> 12, 17, 12: 12 itself.
#   a whole tile per wave: 512 * 1024 units = 238 tiles of 2206 directions in one group, of mean cost class below 8: the
#     one triangle of `single` at 512 x 384, focal length 3: W = 282 .. 292; at focal length 1 W = 68 and it is a quarter.
#   (25 x 17, the ladder's frame: 12 tiles * 371 / 4 = 1113 workgroups, claim_div 557, W <= 6: at most 3 per wave, a third.)
# What each group takes is computed from the host's own constants and asserted -- nothing in the kernel reports its branch.
@pytest.mark.parametrize("mesh,name,width,height,focal,expect", [
    ("blob", "d371", 192, 144, 1.0, {"third", "half"}),             # oracle 0.60 s
    ("blob", "d371", 288, 216, 1.0, {"half", "quarter"}),           # oracle 1.22 s (13 M rays)
    ("blob", "d2206", 72, 48, 1.0, {"third", "half", "quarter"}),   # oracle 0.38 s
    ("blob", "d2206", 80, 48, 1.0, {"third", "half", "quarter"}),   # oracle 0.44 s
    ("blob", "d2206", 48, 32, 1.0, {"half"}),                       # oracle 0.18 s
    ("single", "d2206", 512, 384, 1.0, {"quarter"}),                # oracle 0.32 s
    ("single", "d2206", 512, 384, 3.0, {"whole_tile"}),             # oracle 1.46 s (320 M rays at one triangle)
])
def test_claim_sizes_scarce_and_plentiful(rt, oracle, scene_for, mesh, name, width, height, focal, expect):
    r = ALL[name]
    scene, arrays = scene_for(mesh, "longest")
    opt = options(rt, r, width, height, focal_length=focal)
    ref = reference(oracle, arrays, opt, (mesh, name, width, height, focal))
    host = new_host(rt, scene, opt, STREAM)
    host.render()
    order = host.tile_order()
    taken = claim_rule(order["constants"], len(order["words"]), r.dirs, 2048)
    print(mesh, name, width, height, taken)
    assert_frame(host, ref, (mesh, name, width, height))
    assert expect <= set(taken), (sorted(taken), taken)
    host.measure_tile_costs(2)
    host.set_order_policy(2.0, 2.0, 0.01)
    assert (host.split_tiles().sum() >= 1) == (r.dirs % 2 == 0)  # (an odd count is never split)
    host.render()
    assert_frame(host, ref, (mesh, name, width, height, "split"))
    host.close()


@pytest.mark.parametrize("calibrate", [True, False], ids=["calibrated", "uncalibrated"])
@pytest.mark.parametrize("name", ["d14", "d2206", "d32719", "d33283", "d34986"])
def test_frame_ring(rt, oracle, scene_for, name, calibrate):
    """Two hosts taking frames in turn (a ring measures the tiles' costs and splits by itself), three frames."""
    r, scene, opt, ref = frame_of(rt, oracle, scene_for, "blob", name)
    ring = rt.FrameRing(opt, None, hosts=2)
    ring.set_calibration(calibrate)
    ring.upload_scene(scene)
    for _ in range(3):
        ring.submit()
        assert np.array_equal(ring.collect(), ref[1]), name
    ring.drain()
    img, _, counters = ref
    for k in range(2):  # (both have rendered: their last frames' floats and counters; the bytes came through collect())
        host = ring.host(k)
        got = host.download()
        assert ((bits(got) == bits(img)) | (np.isnan(got) & np.isnan(img))).all(), (name, "ring host", k)
        st = host.stats()
        for key in ("primary_rays", "primary_hits", "ao_rays", "ao_occluded"):
            assert st[key] == counters[key], (name, "ring host", k, key, st[key], counters[key])
        if r.dirs % 2 == 1 or r.dirs >= LIMIT:
            assert host.split_tiles().sum() == 0
    ring.close()


def test_random_sampler_above_the_limit(rt, scene_for):
    """RANDOM with 32768 samples: 32770 rays per hit -- even, half 16385 = 1 mod 4, above 0x8000.  The mode is outside the
    bit-exact contract with the CPU, so the frame is compared with itself: with the split threshold at a hundredth of the
    pass's ideal length against with no splitting, on one host.  (Above the limit no tile is split any more -- tile_order.cc
    --, which is asserted; before that rule the two frames differed.)"""
    scene, _ = scene_for("blob", "longest")
    opt = rt.Options.defaults(width=13, height=11, n_super_samples=1, ao_num_samples=32768, ao_method=1)
    host = new_host(rt, scene, opt, STREAM)
    host.render()
    st = host.stats()
    assert st["primary_hits"] > 0 and st["ao_rays"] == st["primary_hits"] * (32768 + 2)
    host.measure_tile_costs(2)
    host.set_order_policy(2.0, 2.0, 0.0)
    host.render()
    plain, plain_occluded = host.download(), host.stats()["ao_occluded"]
    host.set_order_policy(2.0, 2.0, 0.01)
    assert host.split_tiles().sum() == 0
    host.render()
    assert np.array_equal(bits(host.download()), bits(plain))
    assert host.stats()["ao_occluded"] == plain_occluded and host.stats()["ao_rays"] == st["ao_rays"]
    host.close()


@pytest.mark.parametrize("name,most", [("d371", 300), ("d2206", 300), ("d34986", 65)])
def test_ao_queries_with_long_runs(rt, scene_for, name, most):
    """Host.ambient_occlusion with hundreds to tens of thousands of rays per point: a point's run of lanes spans up to 547
    packets (ao_query_kernel's first / end / below_end), sorted and unsorted, for 1, 2, 63, 64, 65 and `most` points."""
    import query_oracle as qo

    r = ALL[name]
    scene, arrays = scene_for("blob", "longest")
    opt = options(rt, r, 64, 48)
    host = new_host(rt, scene, opt)
    assert host.ao_rays_per_point == (r.dirs, r.dirs)
    p = orc.params_from_options(rt.Options.defaults(width=64, height=48, n_super_samples=1))
    o4, d4 = qo.camera_rays(p)
    cam = host.trace_closest(o4, d4)
    hit = cam["hit"].astype(bool)
    step = max(1, int(hit.sum()) // most)
    points, normals = cam["position"][hit][::step][:most], cam["normal"][hit][::step][:most]
    assert len(points) == most
    want = aoo.ambient_occlusion(orc.params_from_options(opt), arrays, points, normals)
    assert want["rays"] == r.dirs and want["occluded"].max() > 0
    for n in sorted({1, 2, 63, 64, 65, most}):
        for sort in (True, False):
            got = host.ambient_occlusion(points[:n], normals[:n], sort=sort)
            for f in ("ao", "occluded"):
                same = qo.same_words(got[f], want[f][:n])
                assert same.all(), (name, n, sort, f, int((~same).sum()))
    host.close()
