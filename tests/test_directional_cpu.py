"""CPU: the directional occlusion queries' oracle (tests/directional_oracle.c) against the reference's own function, and the
library's exported entry points and binding (include/rt_hip_directional.h)."""
import os
import subprocess

import numpy as np
import pytest

import ao_oracle as aoo
import directional_oracle as dro
import orc
import query_oracle as qo
from conftest import bits, options_for

SYMBOLS = ("rt_ao_mask_words", "rt_trace_ao_directional", "rt_trace_ao_directional_device", "rt_ao_rays", "rt_ao_rays_device")
STRUCT = "rt_ao_directional_arrays"
# golden case -> (counters["ao_occluded"], counters["ao_rays"]) of tests/golden/golden.json
CASES = {"bunny_64_s1_a3": (6127, 60592), "ties_33_s1_a3": (1770, 7560), "blob_40x24_s4_a2_d03_f08": (7520, 28000),
         "blob_80_s1_a5_noshade": (65048, 250062)}


def test_library_exports_the_directional_entry_points(rt):
    header = os.path.join(os.path.dirname(__file__), "..", "include", "rt_hip_directional.h")
    assert os.path.exists(header), "include/rt_hip_directional.h is missing"
    text = open(header).read()
    assert '#include "rt_hip_ao.h"' in text and STRUCT in text
    out = subprocess.run(["nm", "-D", "--defined-only", rt.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    missing = [s for s in SYMBOLS if s not in exported]
    assert not missing, missing
    for s in SYMBOLS:
        assert s + "(" in text, s
        assert s in rt.api._SIGNATURES, s
    for method in ("ao_mask_words", "directional_occlusion", "ao_rays", "vertex_bent_normals"):
        assert hasattr(rt.Host, method), method
    assert callable(rt.unpack_ao_mask) and rt.api.unpack_ao_mask is rt.unpack_ao_mask
    assert rt.api.DIRECTIONAL_OUTPUTS == ("ao", "occluded", "mask", "bent")
    assert rt.api.AO_OUTPUTS == ("ao", "occluded")
    assert [name for name, _ in rt.api._DirectionalArrays._fields_] == ["ao", "occluded", "mask", "bent"]


class _NoLibraryHost:
    """A Host that was never created: every library call through it would fail on the missing handle."""

    def __getattr__(self, name):
        raise AssertionError(f"the binding reached for {name}: a library call before the inputs were checked")


def test_binding_refuses_before_any_library_call(rt):
    host = _NoLibraryHost()
    pts = np.zeros((4, 3), np.float32)
    directional, rays = rt.Host.directional_occlusion, rt.Host.ao_rays
    with pytest.raises(ValueError):
        directional(host, pts, pts, outputs=("hit",))
    with pytest.raises(ValueError):
        directional(host, pts, pts, outputs=("mask", "distance"))
    for call in (directional, rays):
        with pytest.raises(ValueError):
            call(host, pts.astype(np.float64), pts)
        with pytest.raises(ValueError):
            call(host, pts, pts[:3])
        with pytest.raises(ValueError):
            call(host, pts, np.zeros((4, 2), np.float32))
        with pytest.raises(ValueError):
            call(host, pts, pts, seeds=np.zeros(3, np.uint32))
        with pytest.raises(ValueError):
            call(host, pts, pts, seeds=np.zeros(4, np.int64))


def test_unpack_ao_mask():
    import opencl_raytracer_amd as rt

    mask = np.array([[0x80000001, 0x2], [0, 0], [0xFFFFFFFF, 0x3]], np.uint32)
    got = rt.unpack_ao_mask(mask, 34)
    assert got.shape == (3, 34) and got.dtype == bool
    assert np.flatnonzero(got[0]).tolist() == [0, 31, 33] and not got[1].any() and got[2].all()
    assert rt.unpack_ao_mask(mask, 28).shape == (3, 28) and rt.unpack_ao_mask(mask[:0], 64).shape == (0, 64)
    with pytest.raises(ValueError):
        rt.unpack_ao_mask(mask, 65)
    with pytest.raises(ValueError):
        rt.unpack_ao_mask(mask.astype(np.int64), 34)


def camera_points(rt, golden, scene_for, name):
    c = golden["renders"][name]
    opt = options_for(rt, c)
    _, arrays = scene_for(c["mesh"], c["bvh"])
    p = orc.params_from_options(opt)
    o4, d4 = qo.camera_rays(p)
    res = qo.closest(arrays, o4, d4, 100000.0)
    hit = res["hit"].astype(bool)
    return c, p, arrays, res["position"][hit], res["normal"][hit], np.flatnonzero(hit).astype(np.uint32)


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_is_the_reference_function(rt, golden, scene_for, name):
    """Per point the popcount of the restated loop's flags is ambient_occlusion's `hits` and the value made of it its
    result, bit for bit; over the camera's closest hits they add up to the golden frame's counters."""
    c, p, arrays, points, normals, index = camera_points(rt, golden, scene_for, name)
    occluded_total, rays_total = CASES[name]
    assert (c["counters"]["ao_occluded"], c["counters"]["ao_rays"]) == (occluded_total, rays_total)
    got = dro.directional(p, arrays, points, normals, seeds=index)
    want = aoo.ambient_occlusion(p, arrays, points, normals, seeds=index)
    R = got["rays"]
    assert R == want["rays"] and R * len(index) == rays_total
    assert got["mask"].shape == (len(index), (R + 31) // 32)
    assert np.array_equal(got["occluded"], want["occluded"])
    assert np.array_equal(bits(got["ao"]), bits(want["ao"]))
    assert int(got["occluded"].sum(dtype=np.uint64)) == occluded_total
    assert ((got["occluded"] > 0) & (got["occluded"] < R)).any()
    # the bits from R upwards are 0, and the flags unpack to the popcount
    flags = rt.unpack_ao_mask(got["mask"], R)
    assert np.array_equal(flags.sum(axis=1, dtype=np.uint32), got["occluded"])
    # the origin and the sum are what the contract says of the emitted directions
    eps = np.float32(1.0) / np.float32(100000.0)
    assert np.array_equal(bits(got["origins"]), bits(points + normals * eps))
    assert qo.same_words(got["bent"], dro.ordered_sum(got["directions"], ~flags)).all()


def test_open_scene_has_empty_masks(rt, golden, scene_for):
    c, p, arrays, points, normals, index = camera_points(rt, golden, scene_for, "single_32_s1_a3")
    assert len(index) > 0 and c["counters"]["ao_occluded"] == 0
    got = dro.directional(p, arrays, points, normals, seeds=index)
    assert not got["mask"].any() and not got["occluded"].any() and (got["ao"] == 1.0).all()
    everything = np.ones((len(index), got["rays"]), bool)
    assert qo.same_words(got["bent"], dro.ordered_sum(got["directions"], everything)).all()
    assert np.isfinite(got["bent"]).all() and (np.abs(got["bent"]).max(axis=1) > 1.0).all()
