"""CPU: the ray queries' oracle (tests/query_oracle.c) and the library's exported query entry points."""
import hashlib
import os
import subprocess

import numpy as np

import orc
import query_oracle as qo
from conftest import bits, options_for

QUERY_SYMBOLS = ("rt_trace_closest", "rt_trace_occluded", "rt_trace_closest_device", "rt_trace_occluded_device",
                 "rt_last_query_ms")


def _rebuild(rt, oracle, golden, scene_for, name):
    c = golden["renders"][name]
    opt = options_for(rt, c)
    opt.enable_ao = 0  # the primary rays' term alone: what the closest hit decides
    _, arrays = scene_for(c["mesh"], c["bvh"])
    p = orc.params_from_options(opt)
    ref_img, _, _ = oracle.render(p, arrays)
    o4, d4 = qo.camera_rays(p)
    res = qo.closest(arrays, o4, d4, 100000.0)
    value = qo.shade(res["hit"], res["normal"], d4, bool(opt.enable_shading)).reshape(ref_img.shape)
    assert np.array_equal(bits(value), bits(ref_img))
    assert np.array_equal(qo.occluded(arrays, o4, d4, 100000.0), res["hit"])
    return c, value


def test_closest_hits_rebuild_the_oracle_image_bunny(rt, oracle, golden, scene_for):
    c, value = _rebuild(rt, oracle, golden, scene_for, "bunny_256_s1_a0")
    assert hashlib.sha256(value.tobytes()).hexdigest() == c["float_sha256"]  # the reference kernel's own image


def test_closest_hits_rebuild_the_oracle_image_blob_noshade(rt, oracle, golden, scene_for):
    _rebuild(rt, oracle, golden, scene_for, "blob_80_s1_a5_noshade")


def test_library_exports_the_query_entry_points(rt):
    out = subprocess.run(["nm", "-D", "--defined-only", rt.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    missing = [s for s in QUERY_SYMBOLS if s not in exported]
    assert not missing, missing


def test_query_header_declares_the_entry_points():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "rt_hip_query.h")).read()
    for s in QUERY_SYMBOLS:
        assert s + "(" in header, s
