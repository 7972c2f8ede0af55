"""The frame layers and multi-view rendering on one kernel and one tail (kernels/layers.hip.h, kernels/views.hip.h): what
the fold could have moved, compared as BIT PATTERNS -- np.array_equal on floats cannot tell -0 from +0, and a layers
call's `value` of a missed sub-pixel is 0 * 1 out of the tail's arithmetic, no longer a constant out of a select.

The sizes: 5 x 3 is one partial tile; 11 x 6 at 9 supersamples is 33 x 18 sub-pixels, 5 x 3 tiles, partial on both edges
and no multiple of the four waves of a workgroup."""
import numpy as np
import pytest

import layers_cases as lc
import layers_oracle as lo
import orc
from conftest import bits
from test_camera_gpu import poses_for

SIZES = [(5, 3, 1), (11, 6, 9)]
METHODS = [(0, "uniform"), (1, "random")]
HOSTS = ["unposed", "default_pose", "infinite"]  # a host without a pose, one posed at the default pose, one that sees nothing
ONE, ZERO = 0x3F800000, 0x00000000
MISS = ("hit", "ao", "value")

_WANT = {}


def case_of(size):
    return ("blob", "longest", *size, None, 1, 2)


def camera_of(rt, scene_for, kind):
    if kind == "unposed":
        return None
    return rt.Camera.default() if kind == "default_pose" else poses_for(rt, scene_for("bunny", "longest")[1])[kind]


def oracle_of(rt, scene_for, size, method, kind) -> dict:
    """The CPU oracle's layers (tests/layers_oracle.c), computed once per case and shared."""
    key = (size, method, kind)
    if key not in _WANT:
        opt = lc.options_of(rt, case_of(size), ao_method=method)
        _WANT[key] = lo.render(orc.params_from_options(opt), scene_for("blob", "longest")[1], camera_of(rt, scene_for, kind))
    return _WANT[key]


def upload(rt, scene_for, size, method, cam):
    opt = lc.options_of(rt, case_of(size), ao_method=method)
    host = rt.Host(opt, 0)
    if cam is not None:
        host.set_camera(cam)
    host.upload_scene(scene_for("blob", "longest")[0])
    return host


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}_s{s[2]}")
def test_the_oracle_sees_hit_and_missed_sub_pixels(rt, scene_for, size):
    """(no GPU) What test_missed_sub_pixels compares is there: both kinds of sub-pixel at both sizes, none hit from the blind pose."""
    for kind in ("unposed", "default_pose"):
        hit = oracle_of(rt, scene_for, size, 0, kind)["hit"].astype(bool)
        assert hit.any() and (~hit).any(), (size, kind, int(hit.sum()), hit.size)
    assert not oracle_of(rt, scene_for, size, 0, "infinite")["hit"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", HOSTS)
@pytest.mark.parametrize("method", METHODS, ids=lambda m: m[1])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}_s{s[2]}")
def test_missed_sub_pixels(rt, scene_for, size, method, kind):
    """A layers call with the ambient-occlusion step: a missed sub-pixel's `ao` is 1.0f and its `value` +0.0f, word for
    word; a hit one's are the oracle's."""
    want = oracle_of(rt, scene_for, size, method[0], kind)
    host = upload(rt, scene_for, size, method[0], camera_of(rt, scene_for, kind))
    try:
        got = host.render_layers(MISS)
    finally:
        host.close()
    hit = got["hit"].astype(bool)
    assert np.array_equal(got["hit"], want["hit"])
    if kind == "infinite":
        assert not hit.any()
    else:
        assert hit.any() and (~hit).any()
    ao, value = bits(got["ao"]), bits(got["value"])
    print(f"FOLD_MISSED size={size} method={method[1]} host={kind} hit={int(hit.sum())} missed={int((~hit).sum())} "
          f"ao_missed_not_one={int((ao[~hit] != ONE).sum())} value_missed_not_zero={int((value[~hit] != ZERO).sum())} "
          f"ao_hit_differs={int((ao[hit] != bits(want['ao'])[hit]).sum())} value_hit_differs={int((value[hit] != bits(want['value'])[hit]).sum())}")
    assert (ao[~hit] == ONE).all() and (value[~hit] == ZERO).all()
    assert np.array_equal(ao[hit], bits(want["ao"])[hit]) and np.array_equal(value[hit], bits(want["value"])[hit])


def same_bits(a, b) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a) if a.dtype == np.float32 else a, bits(b) if b.dtype == np.float32 else b)


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS, ids=lambda m: m[1])
def test_the_two_routes_of_the_posed_kernel_agree(rt, scene_for, method):
    """render_layers on a host uploaded with pose P == block 0 of render_views([P]) on that host == block 1 of
    render_views([Q, P]) on a host without a pose: the pose from the kernel arguments against the pose from the array,
    every sub-pixel an entry of the ambient-occlusion step against the hit ones listed."""
    named = poses_for(rt, scene_for("bunny", "longest")[1])
    P, Q = named["orbit_135"], named["roll"]
    posed, plain = upload(rt, scene_for, (11, 6, 9), method[0], P), upload(rt, scene_for, (11, 6, 9), method[0], None)
    try:
        layers = posed.render_layers(rt.LAYER_OUTPUTS)
        own = posed.render_views([P], rt.LAYER_OUTPUTS)
        other = plain.render_views([Q, P], rt.LAYER_OUTPUTS)
    finally:
        posed.close()
        plain.close()
    hit = layers["hit"].astype(bool)
    assert hit.any() and (~hit).any()
    for name in rt.LAYER_OUTPUTS:
        assert same_bits(layers[name], own[name][0]), (name, "block 0 of the host's own pose")
        assert same_bits(layers[name], other[name][1]), (name, "block 1 on a host without a pose")
    assert not same_bits(other["hit"][0], other["hit"][1])  # (Q is another view)


@pytest.mark.gpu
def test_a_layers_call_leaves_the_views_books_alone(rt, scene_for):
    """rt_debug_last_views reports views calls only (the stream-ordered half: tests/views_torch_driver.py)."""
    host = upload(rt, scene_for, (11, 6, 9), 0, None)
    try:
        before = host.render_layers(("ao", "value"))
        host.render_views([rt.Camera.default(), poses_for(rt, scene_for("bunny", "longest")[1])["roll"]], ("ao",))
        done = host.last_views()
        assert done["views"] == 2 and done["chunks"] == 1 and done["ao_points"] > 0
        after = host.render_layers(("ao", "value"))
        assert host.last_views() == done
        assert same_bits(after["ao"], before["ao"]) and same_bits(after["value"], before["value"])
    finally:
        host.close()
