"""Child process of tests/test_build_gpu.py::test_device_memory_form: torch's HIP runtime comes up first, then the library; a
build from device tensors must leave the records, the leaf order and the answers a build from numpy arrays leaves, on every
mesh of tests/build_cases.py; and a face index out of range is found ON the device: refused, the previous scene still answers."""
import os
import sys

import torch

torch.zeros(1, device="cuda:0")  # (before the library is loaded)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np  # noqa: E402

import opencl_raytracer_amd as rt  # noqa: E402
import build_cases as bc  # noqa: E402
import multihit_oracle as mo  # noqa: E402
import orc  # noqa: E402
import query_oracle as qo  # noqa: E402


def same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("nodes", "tris", "shade"))


def main():
    opt = rt.Options.defaults(width=64, height=48, n_super_samples=1, ao_num_samples=3, ao_max_distance=0.2)
    by_numpy, by_torch = rt.Host(opt, 0), rt.Host(opt, 0)
    side = torch.cuda.Stream(device="cuda:0")
    for name in bc.MESHES:
        v, f = bc.mesh(name)
        scene = rt.Scene.from_arrays(v, f)
        by_numpy.build_scene(v, f, scene.vnormals)
        want = by_numpy.records()
        with torch.cuda.stream(side):
            tv, tn = torch.from_numpy(v.copy()).to("cuda:0"), torch.from_numpy(scene.vnormals.copy()).to("cuda:0")
            tf = torch.from_numpy(f.astype(np.int32)).to("cuda:0")
            by_torch.build_scene(tv, tf, tn)
        assert same(by_torch.records(), want), name
        assert np.array_equal(by_torch.face_of_leaf(), by_numpy.face_of_leaf()), name
        assert np.array_equal(by_torch.face_of_leaf(), bc.restated(name)["triangles"]), name
        assert by_torch.last_build_ms > 0.0
    # blob is next: (V, 3) vertices and int64 faces; a query right behind the build, on the same stream
    v, f = bc.mesh("blob")
    built = bc.lbvh_scene(rt, "blob")
    arrays = orc.SceneArrays.from_scene(built)
    ro, rd = mo.random_rays(arrays, 20000, 7)  # (enough for the sort, whose box the build must have dropped)
    want_hits = qo.closest(arrays, ro, rd, 100000.0)
    with torch.cuda.stream(side):
        tv3 = torch.from_numpy(np.ascontiguousarray(v[:, :3])).to("cuda:0")
        tn = torch.from_numpy(built.vnormals.copy()).to("cuda:0")
        by_torch.build_scene(tv3, torch.from_numpy(f.astype(np.int64)).to("cuda:0"), tn)
        behind = by_torch.trace_closest(torch.from_numpy(ro).to("cuda:0"), torch.from_numpy(rd).to("cuda:0"))
    side.synchronize()
    for name in rt.api.QUERY_OUTPUTS:
        assert qo.same_words(behind[name].cpu().numpy(), want_hits[name]).all(), name
    good = by_torch.records()
    # one face index == num_vertices.  The vertex tensor is a slice of a larger one: even a read through the bad index would stay
    # inside its allocation -- this is about the flag the first kernel raises, not about a fault.
    larger = torch.zeros((len(v) + 64, 4), dtype=torch.float32, device="cuda:0")
    larger[:len(v)] = torch.from_numpy(v.copy()).to("cuda:0")
    tv = larger[:len(v)]
    bad = f.astype(np.int32).copy()
    bad[len(bad) // 2, 1] = len(v)
    try:
        by_torch.build_scene(tv, torch.from_numpy(bad).to("cuda:0"), tn)
    except rt.RtError as e:
        assert e.code == rt.api.RT_E_INVALID and "out of range" in e.message, e
    else:
        raise AssertionError("a build with a face index out of range went through")
    assert same(by_torch.records(), good)
    again = by_torch.trace_closest(ro, rd)
    for name in rt.api.QUERY_OUTPUTS:
        assert qo.same_words(again[name], want_hits[name]).all(), name
    # refusals of the device form and of the binding
    tf = torch.from_numpy(f.astype(np.int32)).to("cuda:0")
    for call, kind in ((lambda: by_torch.build_scene(tv, tf), rt.RtError), (lambda: by_torch.build_scene(tv, tf, built.vnormals), ValueError),
                       (lambda: by_torch.build_scene(tv, tf.float(), tn), ValueError), (lambda: by_torch.build_scene(tv, tf[:0], tn), rt.RtError)):
        try:
            call()
        except kind as e:
            assert kind is not rt.RtError or e.code == rt.api.RT_E_INVALID
        else:
            raise AssertionError("a build that must be refused went through")
    lib = rt.load_library()
    assert lib.rt_build_scene_device(by_torch._h, tv.data_ptr() + 4, tn.data_ptr(), len(v), tf.data_ptr(), len(f), None) == rt.api.RT_E_INVALID
    assert same(by_torch.records(), good)
    by_numpy.close()
    by_torch.close()
    print("BUILD_TORCH_OK", int(want_hits["hit"].sum()), "of", len(ro), "rays hit")


if __name__ == "__main__":
    main()
