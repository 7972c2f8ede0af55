"""Child process of tests/test_instance_directional_gpu.py::test_torch_path_equals_numpy_path: torch's HIP runtime comes up
first, then the library; device tensors in and device tensors out on a non-default stream must equal the numpy path -- sorted
and not, (N, 3) and (N, 4) inputs, seeds, subsets of the outputs."""
import os
import sys

import torch

torch.zeros(1, device="cuda:0")  # (before the library is loaded)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np  # noqa: E402

import instance_cases as cases  # noqa: E402
import instance_directional_oracle as ido  # noqa: E402
import opencl_raytracer_amd as rt  # noqa: E402
import orc  # noqa: E402


def same(got, want, what):
    for f in got:
        assert tuple(got[f].shape) == want[f].shape, (what, f)
        assert ido.same_words(got[f].cpu().numpy(), want[f]).all(), (what, f)


def main():
    scene = rt.Scene.load_off(os.path.join(HERE, "golden", "meshes", "blob.off")).build_bvh(1)
    arrays = orc.SceneArrays.from_scene(scene)
    opt = rt.Options.defaults(width=64, height=48, ao_num_samples=5, ao_max_distance=0.5)
    host = rt.Host(opt, 0)
    host.upload_scene(scene)
    host.set_instances(cases.many(arrays, 65, seed=3))
    plan = host.instances()
    o, d = cases.rays(plan["nodes"], 6000, seed=83)
    near = host.trace_instances_closest(o, d, outputs=("distance", "position", "normal"))
    at = near["distance"] < np.inf
    points, normals = np.ascontiguousarray(near["position"][at][:700]), np.ascontiguousarray(near["normal"][at][:700])
    n = len(points)
    assert n > 300 and n * host.ao_rays_per_point[0] >= 16384  # (sorted where the call allows it)
    seeds = np.arange(n, dtype=np.uint32)[::-1].copy()
    want = host.instances_directional_occlusion(points, normals, seeds)
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):
        tp, tn, ts = torch.from_numpy(points).to("cuda:0"), torch.from_numpy(normals).to("cuda:0"), torch.from_numpy(seeds).to("cuda:0")
        got = host.instances_directional_occlusion(tp, tn, ts)
        loose = host.instances_directional_occlusion(torch.nn.functional.pad(tp, (0, 1)), torch.nn.functional.pad(tn, (0, 1)), sort=False)
        part = host.instances_directional_occlusion(tp, tn, ts, outputs=("bent",))
        mask = host.instances_directional_occlusion(tp, tn, outputs=("mask",), sort=False)
    side.synchronize()
    same(got, want, "all four")
    same(loose, want, "(N, 4) inputs, unsorted, no seeds")
    assert set(part) == {"bent"} and set(mask) == {"mask"}
    same(part, want, "bent alone")
    same(mask, want, "mask alone")
    assert got["mask"].dtype == torch.uint32 and got["bent"].device.type == "cuda" and tuple(got["mask"].shape) == (n, host.ao_mask_words)
    expect = ido.directional(orc.params_from_options(opt), arrays, plan, points, normals, seeds)
    for f in ido.OUTPUTS:
        assert ido.same_words(want[f], expect[f]).all(), ("numpy path", f)
    assert want["occluded"].any()
    host.close()
    print("INSTANCE_DIRECTIONAL_TORCH_OK", int(want["occluded"].sum()), "blocked rays at", n, "points")


if __name__ == "__main__":
    main()
