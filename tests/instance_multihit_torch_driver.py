"""Child process of tests/test_instance_multihit_gpu.py::test_torch_path_equals_numpy_path: torch's HIP runtime comes up
first, then the library; device tensors in and device tensors out on a non-default stream must equal the numpy path -- k = 16,
3 and the count alone, sorted and not, (N, 3) and (N, 4) inputs, a subset of the outputs."""
import os
import sys

import torch

torch.zeros(1, device="cuda:0")  # (before the library is loaded)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np  # noqa: E402

import instance_cases as cases  # noqa: E402
import instance_multihit_oracle as imo  # noqa: E402
import opencl_raytracer_amd as rt  # noqa: E402
import orc  # noqa: E402


def same(got, want, what):
    for f in got:
        assert tuple(got[f].shape) == want[f].shape, (what, f, tuple(got[f].shape), want[f].shape)
        assert imo.same_words(got[f].cpu().numpy(), want[f]).all(), (what, f)


def main():
    scene = rt.Scene.load_off(os.path.join(HERE, "golden", "meshes", "blob.off")).build_bvh(1)
    arrays = orc.SceneArrays.from_scene(scene)
    host = rt.Host(rt.Options.defaults(width=64, height=48), 0)
    host.upload_scene(scene)
    host.set_instances(cases.family("grid", arrays))
    plan = host.instances()
    o, d = cases.rays(plan["nodes"], 20000, seed=83)
    oo, od = cases.odd_rays(plan["nodes"])
    o, d = np.concatenate([o, oo]), np.concatenate([d, od])
    want = host.trace_instances_multihit(o, d, k=16)
    want_near = host.trace_instances_multihit(o, d, 0.3, k=3)
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):
        to, td = torch.from_numpy(o).to("cuda:0"), torch.from_numpy(d).to("cuda:0")
        got = host.trace_instances_multihit(to, td, k=16)
        count = host.count_instances_hits(to, td, sort=False)
        got_near = host.trace_instances_multihit(torch.nn.functional.pad(to, (0, 1)), torch.nn.functional.pad(td, (0, 1)), 0.3, k=3, sort=False)
        part = host.trace_instances_multihit(to, td, k=16, outputs=("instance", "normal"))
    side.synchronize()
    same(got, want, "k = 16")
    same(got_near, want_near, "k = 3, max_distance 0.3")
    assert np.array_equal(count.cpu().numpy(), want["count"])
    assert set(part) == {"instance", "normal"}
    same(part, want, "subset")
    assert got["instance"].dtype == torch.uint32 and got["count"].device.type == "cuda" and tuple(got["instance"].shape) == (len(o), 16)
    imo.assert_same(want, imo.multihit(arrays, plan, o, d, 1e5, 16), "numpy path")
    host.close()
    print("INSTANCE_MULTIHIT_TORCH_OK", int(want["count"].sum()), "members on", len(o), "rays")


if __name__ == "__main__":
    main()
