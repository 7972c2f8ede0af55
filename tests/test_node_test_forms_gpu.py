"""GPU: the any-hit walk's node test with near and far of an axis from ONE packed fma (kernels/walk.hip.h,
OCRT_TEST_CE_SCALED: 3 v_fma_f32 + 3 v_pk_fma_f32 + max3 + min3 + cmp) against the twelve-instruction form it replaced.

The arithmetic test runs both forms on the device over the same centre / half-extent records and walk rays
(include/rt_hip_debug.h, rt_debug_node_test_forms; the old form lives on in that test kernel alone) and asserts equal BITS of
near and far and equal decisions, lane by lane, for the packed form in the registers of the loop's node `a` and of its node
`b`.  That is what the proofs at ce_record / padded_bound (scene_pack.cc) and tests/walk_margin_check.cc rest on: each half
of the packed instruction is the fused multiply-add v_fma_f32 is, on the same operands -- that op_sel picks the high dword of
an SGPR pair, that neg_lo negates the low half alone and that the clamp reaches both halves is decided here, on the part, not
from the manual.  64 rays x 512 records: random finite values and the edge values the loop meets.

The frame tests render through the loop the way tests/test_ao_tile_setup_gpu.py does (whose helpers and oracle frames they
share), bit for bit against the CPU oracle: 64 x 48 and 256 x 192 of the bunny, 100 x 68 of the interior stand-in, 28 and 71
table directions, one-shot and stream hosts, with and without the look-ahead loads (setAoPrefetch); and one AO_RANDOM frame
under that mode's statistical bar (tests/test_hip_parity.py, test_random_ao_statistical_parity).
"""
import numpy as np
import pytest

import orc
from ao_direction_cases import ALL, rung
from test_ao_tile_setup_gpu import FRAMES, STREAM, assert_frame, options, reference

pytestmark = pytest.mark.gpu

RAYS, BOXES = 64, 512
F = np.float32
COUNTS = {"d28": rung(3, 28), "d71": ALL["d71"]}


def f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def walk_rays():
    """(64, 6) walk rays as make_walk_ray leaves them: i = reciprocal * walk_scale, oi = -(o * i) rounded once."""
    rng = np.random.default_rng(20260)
    scale = F(1.0) / F(0.2)  # ~ 1 / AO_MAX_DISTANCE
    d = rng.normal(size=(RAYS, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = rng.uniform(-1.0, 1.0, size=(RAYS, 3)).astype(F)
    inv = (F(1.0) / d.astype(F)).astype(F)
    # a zero direction component: walk_reciprocal's +-2^100 for the infinite reciprocal, on each axis and both signs
    for k, (ray, axis) in enumerate([(40, 0), (41, 1), (42, 2), (43, 0), (44, 1), (45, 2)]):
        inv[ray, axis] = F(2.0 ** 100) if k < 3 else F(-(2.0 ** 100))
    inv[46] = [F(2.0 ** 100), F(-(2.0 ** 100)), inv[46, 2]]
    i = (inv * scale).astype(F)
    o[47] = [0.0, -0.0, 0.0]  # oi = -0.0 / +0.0 by the sign of i
    o[48, 2] = 0.0
    oi = (-(o * i)).astype(F)
    oi[49, 0] = np.nan  # a NaN oi: v_max3 / v_min3 drop the axis (x, y), the clamp makes 0 of it (z)
    oi[50, 1] = np.nan
    oi[51, 2] = np.nan
    oi[52] = np.nan
    oi[53, 2], oi[54, 2] = F(1.0e6), F(-1.0e6)  # t_c far outside [0, 1] on z: both clamps bite
    oi[55, 2], oi[56, 2] = F(3.0e38), F(-3.0e38)
    oi[57, 0], oi[58, 1] = f32(0x00000001), f32(0x80000001)  # denormal oi
    i[59] = [-0.0, 0.0, -0.0]  # (never met: |i| >= 0.5 * scale; the sign handling of a zero all the same)
    i[60, 0], i[61, 2] = F(-2.5), F(-2.5)
    oi[62, 2], oi[63, 2] = F(0.5), F(1.0)  # t_c on the limits of the clamp
    return np.concatenate([i, oi], axis=1).astype(F)


def records():
    """(512, 8) centre / half-extent records: c.xyz, skip | e.xyz, leaf (scene_pack.cc, ce_record)."""
    rng = np.random.default_rng(20261)
    c = rng.uniform(-1.0, 1.0, size=(BOXES, 3)).astype(F)
    e = rng.uniform(0.0, 0.5, size=(BOXES, 3)).astype(F)
    e[400:420] = 0.0  # zero half-extents (a flat box's axis), on one axis and on all
    e[420:440, 0] = 0.0
    e[440:460, 2] = 0.0
    e[460:470] = f32(0x00000001)  # denormal half-extents
    e[470:480, 1] = f32(0x007FFFFF)
    e[480:484] = -0.0  # (not made by ce_record; the sign of a zero product)
    c[484:490] = -0.0
    c[490:494, 2] = 0.0
    c[494:500] = rng.uniform(-1.0e6, 1.0e6, size=(6, 3)).astype(F)  # the origin limit's magnitude
    e[500:506] = rng.uniform(0.0, 1.0e6, size=(6, 3)).astype(F)
    e[506:512] = np.inf  # the END records' infinite box
    c[506:512] = 0.0
    rec = np.zeros((BOXES, 8), dtype=F)
    rec[:, 0:3], rec[:, 4:7] = c, e
    words = rec.view(np.uint32)
    words[:, 3] = 32 * rng.integers(1, 1000, size=BOXES)  # skip bytes: small integers, denormal patterns
    words[:, 7] = np.where(np.arange(BOXES) % 2 == 0, 0xFFFFFFFF, rng.integers(0, 1 << 26, size=BOXES))  # leaf: NONE (a NaN pattern) or a number
    words[7::16, 7] = 0xFFFFFFFE  # WALK_END
    return rec


def test_packed_form_has_the_bits_of_the_twelve_instruction_form(rt):
    rays, rec = walk_rays(), records()
    out = rt.node_test_forms(rec, rays)
    assert out.shape == (RAYS, BOXES, 9)
    old, new_a, new_b = out[:, :, 0:3], out[:, :, 3:6], out[:, :, 6:9]
    near, far = old[:, :, 0].view(np.float32), old[:, :, 1].view(np.float32)
    hits = int(old[:, :, 2].sum())
    print("pairs", RAYS * BOXES, "hits (old form)", hits, "near clamped to 1", int((near == 1.0).sum()), "far clamped to 0", int((far == 0.0).sum()),
          "NaN near", int(np.isnan(near).sum()))
    for name, new in (("node a", new_a), ("node b", new_b)):
        diff = new != old
        print(name, "differing near", int(diff[:, :, 0].sum()), "far", int(diff[:, :, 1].sum()), "decision", int(diff[:, :, 2].sum()))
    # the cases are not vacuous: both decisions occur, and both clamps bite
    # (rays 53 / 54 against the plain random records: z clamped to 1 on both sides -> near >= 1 >= far; to 0 -> far <= 0 <= near)
    assert set(np.unique(old[:, :, 2]).tolist()) == {0, 1} and 0.01 * RAYS * BOXES < hits < 0.99 * RAYS * BOXES
    assert (near[53, :400] >= 1.0).all() and (far[53, :400] <= 1.0).all() and not old[53, :400, 2].any()
    assert (near[54, :400] >= 0.0).all() and (far[54, :400] <= 0.0).all() and not old[54, :400, 2].any()
    # ... the decision is the strict comparison of the two values (NaN: false)
    assert np.array_equal(old[:, :, 2] == 1, near < far)
    for name, new in (("node a", new_a), ("node b", new_b)):
        for k, what in enumerate(("near", "far", "decision")):
            bad = np.argwhere(new[:, :, k] != old[:, :, k])
            assert bad.size == 0, (name, what, len(bad), "first (ray, record)", bad[0].tolist(),
                                   hex(int(old[tuple(bad[0])][k])), hex(int(new[tuple(bad[0])][k])), rays[bad[0][0]].tolist(),
                                   rec[bad[0][1]].tolist())


def test_bad_arguments_are_refused(rt):
    with pytest.raises(rt.RtError):
        rt.node_test_forms(records(), walk_rays()[:63])  # not a multiple of 64
    with pytest.raises(ValueError):
        rt.node_test_forms(records()[:, :7], walk_rays())


@pytest.mark.parametrize("name", list(COUNTS))
@pytest.mark.parametrize("mesh,width,height", FRAMES)
def test_frames_through_the_packed_test(rt, oracle, scene_for, mesh, width, height, name):
    r = COUNTS[name]
    scene, arrays = scene_for(mesh, "longest")
    opt = options(rt, r, width, height)
    ref = reference(oracle, arrays, opt, (mesh, width, height, name))
    assert ref[2]["ao_rays"] == ref[2]["primary_hits"] * r.dirs and ref[2]["ao_occluded"] > 0
    for frames in (None, STREAM):  # a one-shot host, an announced stream (walk intervals per tile and direction)
        for lookahead in (False, True):
            host = rt.Host(opt, 0)
            host.set_ao_prefetch(lookahead)
            if frames is not None:
                host.expect_frames(frames)
            host.upload_scene(scene)
            host.render()
            assert_frame(host, ref, (mesh, width, height, name, "frames", frames, "look-ahead", lookahead))
            host.close()


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
