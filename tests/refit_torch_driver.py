"""Child process of tests/test_refit_gpu.py::test_device_memory_form_equals_host_memory_form: torch's HIP runtime comes up
first, then the library; an update from device tensors on a non-default stream must leave the records a numpy update leaves,
and a query enqueued right behind it -- on that stream or on the host's own -- must see the whole of it."""
import os
import sys

import torch

torch.zeros(1, device="cuda:0")  # (before the library is loaded)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np  # noqa: E402

import opencl_raytracer_amd as rt  # noqa: E402
import multihit_oracle as mo  # noqa: E402
import orc  # noqa: E402
import query_oracle as qo  # noqa: E402
import refit_cases as rc  # noqa: E402


def same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("nodes", "tris", "shade"))


def main():
    opt = rt.Options.defaults(width=64, height=48, n_super_samples=1, ao_num_samples=3, ao_max_distance=0.2)
    scene = rc.fresh_scene(rt, "blob", "sah")
    original = scene.vertices
    new = rc.deformed("twist", original)
    by_numpy, by_torch = rt.Host(opt, 0), rt.Host(opt, 0)
    by_numpy.upload_scene(scene)
    by_torch.upload_scene(scene)
    uploaded = by_torch.records()
    scene.refit(new)
    arrays = orc.SceneArrays.from_scene(scene)
    ro, rd = mo.random_rays(arrays, 20000, 7)  # (enough for the sort, whose box the update must have dropped)
    want_hits = qo.closest(arrays, ro, rd, 100000.0)
    by_numpy.update_vertices(new, scene.vnormals)
    want = by_numpy.records()
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):
        tv = torch.from_numpy(new).to("cuda:0")
        tn = torch.from_numpy(scene.vnormals).to("cuda:0")
        by_torch.update_vertices(tv, tn)
        behind = by_torch.trace_closest(torch.from_numpy(ro).to("cuda:0"), torch.from_numpy(rd).to("cuda:0"))  # same stream, no wait between
    on_own_stream = by_torch.trace_closest(ro, rd)  # the host-memory form, on the host's own stream: ordered by the queries' event
    side.synchronize()
    assert same(by_torch.records(), want)
    for f in rt.api.QUERY_OUTPUTS:
        assert qo.same_words(behind[f].cpu().numpy(), want_hits[f]).all(), f
        assert qo.same_words(on_own_stream[f], want_hits[f]).all(), f
    assert by_torch.last_update_ms > 0.0
    # (V, 3) tensors, no normals: the padded copy is the binding's; the shading records stay
    with torch.cuda.stream(side):
        by_torch.update_vertices(torch.from_numpy(np.ascontiguousarray(original[:, :3])).to("cuda:0"))
    side.synchronize()
    back = by_torch.records()
    assert back["shade"].tobytes() == want["shade"].tobytes() and back["tris"].tobytes() == uploaded["tris"].tobytes()
    assert np.array_equal(back["nodes"]["lo"], uploaded["nodes"]["lo"]) and np.array_equal(back["nodes"]["hi"], uploaded["nodes"]["hi"])  # (as values)
    # refusals of the device form and of the binding
    for call, kind in ((lambda: by_torch.update_vertices(tv[:-1]), rt.RtError), (lambda: by_torch.update_vertices(tv, scene.vnormals), ValueError),
                       (lambda: by_torch.update_vertices(tv.cpu()), ValueError), (lambda: by_torch.update_vertices(tv.double()), ValueError)):
        try:
            call()
        except kind as e:
            assert kind is not rt.RtError or e.code == rt.api.RT_E_INVALID
        else:
            raise AssertionError("an update that must be refused went through")
    lib = rt.load_library()
    assert lib.rt_update_vertices_device(by_torch._h, tv.data_ptr() + 4, None, len(new), None) == rt.api.RT_E_INVALID
    assert same(by_torch.records(), back)
    by_numpy.close()
    by_torch.close()
    print("REFIT_TORCH_OK", int(want_hits["hit"].sum()), "of", len(ro), "rays hit")


if __name__ == "__main__":
    main()
