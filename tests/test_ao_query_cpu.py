"""CPU: the ambient-occlusion queries' oracle (tests/ao_oracle.c) and the library's exported AO entry points."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import ao_oracle as aoo
import orc
import query_oracle as qo
from conftest import GOLDEN_DIR, bits, options_for

AO_SYMBOLS = ("rt_ao_rays_per_point", "rt_trace_ao", "rt_trace_ao_device")
CASES = ["bunny_64_s1_a3", "ties_33_s1_a3", "blob_40x24_s4_a2_d03_f08", "blob_80_s1_a5_noshade"]


@pytest.mark.parametrize("name", CASES)
def test_ao_oracle_rebuilds_the_oracle_image(rt, oracle, golden, scene_for, name):
    """The wrapper is the reference's function: shade x ambient_occlusion(position, normal, index = y W + x) at the closest
    hits of the reference camera, 0 elsewhere, is the oracle's frame -- and the reference kernel's own float image."""
    c = golden["renders"][name]
    opt = options_for(rt, c)
    _, arrays = scene_for(c["mesh"], c["bvh"])
    p = orc.params_from_options(opt)
    ref_img, counters, _ = oracle.render(p, arrays)
    o4, d4 = qo.camera_rays(p)
    res = qo.closest(arrays, o4, d4, 100000.0)
    value = qo.shade(res["hit"], res["normal"], d4, bool(opt.enable_shading))
    hit = res["hit"].astype(bool)
    index = np.flatnonzero(hit).astype(np.uint32)  # y * W + x of the sub-pixel
    got = aoo.ambient_occlusion(p, arrays, res["position"][hit], res["normal"][hit], seeds=index)
    assert got["rays"] * len(index) == counters["ao_rays"] == c["counters"]["ao_rays"]
    assert int(got["occluded"].sum(dtype=np.uint64)) == c["counters"]["ao_occluded"]
    value[hit] = value[hit] * got["ao"]
    value = value.reshape(ref_img.shape)
    assert np.array_equal(bits(value), bits(ref_img))
    assert hashlib.sha256(value.tobytes()).hexdigest() == c["float_sha256"]
    dump = os.path.join(GOLDEN_DIR, f"render_{name}.npz")
    assert os.path.exists(dump) == bool(c["dump"])
    if c["dump"]:  # the reference kernel's own float image
        with np.load(dump) as z:
            assert np.array_equal(bits(z["image"]), bits(value))
    # UNIFORM ignores the index: defaulted seeds give the same words
    again = aoo.ambient_occlusion(p, arrays, res["position"][hit], res["normal"][hit])
    assert np.array_equal(bits(again["ao"]), bits(got["ao"])) and np.array_equal(again["occluded"], got["occluded"])


def test_library_exports_the_ao_entry_points(rt):
    out = subprocess.run(["nm", "-D", "--defined-only", rt.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    missing = [s for s in AO_SYMBOLS if s not in exported]
    assert not missing, missing
    header = os.path.join(os.path.dirname(__file__), "..", "include", "rt_hip_ao.h")
    assert os.path.exists(header), "include/rt_hip_ao.h is missing"
    text = open(header).read()
    for s in AO_SYMBOLS:
        assert s + "(" in text, s
        assert s in rt.api._SIGNATURES, s
    for method in ("ao_rays_per_point", "ambient_occlusion", "vertex_ao"):
        assert hasattr(rt.Host, method), method
