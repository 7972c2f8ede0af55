"""Child process of tests/test_instances_gpu.py::test_torch_path_equals_numpy_path: torch's HIP runtime comes up first, then
the library; device tensors in and device tensors out on a non-default stream must equal the numpy path -- both forms, sorted
and not, (N, 3) and (N, 4) inputs, a subset of the outputs."""
import os
import sys

import torch

torch.zeros(1, device="cuda:0")  # (before the library is loaded)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np  # noqa: E402

import instance_cases as cases  # noqa: E402
import instance_oracle as io  # noqa: E402
import opencl_raytracer_amd as rt  # noqa: E402
import orc  # noqa: E402


def same(got, want, what):
    for f in got:
        assert io.same_words(got[f].cpu().numpy(), want[f]).all(), (what, f)


def main():
    scene = rt.Scene.load_off(os.path.join(HERE, "golden", "meshes", "blob.off")).build_bvh(1)
    arrays = orc.SceneArrays.from_scene(scene)
    host = rt.Host(rt.Options.defaults(width=64, height=48), 0)
    host.upload_scene(scene)
    host.set_instances(cases.many(arrays, 65, seed=3))
    plan = host.instances()
    o, d = cases.rays(plan["nodes"], 20000, seed=83)
    oo, od = cases.odd_rays(plan["nodes"])
    o, d = np.concatenate([o, oo]), np.concatenate([d, od])
    want = host.trace_instances_closest(o, d)
    want_near = host.trace_instances_closest(o, d, 0.3)
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):
        to, td = torch.from_numpy(o).to("cuda:0"), torch.from_numpy(d).to("cuda:0")
        got = host.trace_instances_closest(to, td)
        occ = host.trace_instances_occluded(to, td, sort=False)
        got_near = host.trace_instances_closest(torch.nn.functional.pad(to, (0, 1)), torch.nn.functional.pad(td, (0, 1)), 0.3, sort=False)
        part = host.trace_instances_closest(to, td, outputs=("instance", "normal"))
    side.synchronize()
    same(got, want, "closest")
    same(got_near, want_near, "closest, max_distance 0.3")
    assert np.array_equal(occ.cpu().numpy(), want["hit"])
    assert set(part) == {"instance", "normal"}
    same(part, want, "subset")
    assert got["instance"].dtype == torch.uint32 and got["hit"].device.type == "cuda" and occ.dtype == torch.uint8
    io.assert_same(want, io.closest(arrays, plan, o, d, 1e5), "numpy path")
    host.close()
    print("INSTANCES_TORCH_OK", int(want["hit"].sum()), "hit of", len(o))


if __name__ == "__main__":
    main()
