"""Child process of tests/test_ao_query_gpu.py::test_torch_path_equals_numpy_path: torch's HIP runtime comes up first,
then the library; device tensors in and out on a non-default stream must equal the numpy path."""
import os
import sys

import torch

torch.zeros(1, device="cuda:0")  # (before the library is loaded)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np  # noqa: E402

import opencl_raytracer_amd as rt  # noqa: E402
import orc  # noqa: E402
import query_oracle as qo  # noqa: E402
from tools.meshes import bunny_path  # noqa: E402


def main():
    scene = rt.Scene.load_off(bunny_path()).build_bvh(1)
    host = rt.Host(rt.Options.defaults(width=64, height=48, ao_num_samples=3), 0)
    host.upload_scene(scene)
    o4, d4 = qo.camera_rays(orc.params_from_options(rt.Options.defaults(width=96, height=72, n_super_samples=1)))
    cam = host.trace_closest(o4, d4)
    hit = cam["hit"].astype(bool)
    points, normals = cam["position"][hit], cam["normal"][hit]
    n = len(points)
    seeds = np.flatnonzero(hit).astype(np.uint32)
    want = host.ambient_occlusion(points, normals, seeds=seeds)
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):
        tp = torch.from_numpy(points).to("cuda:0")
        tn = torch.from_numpy(normals).to("cuda:0")
        ts = torch.from_numpy(seeds.view(np.int32)).to("cuda:0").view(torch.uint32)
        got = host.ambient_occlusion(tp, tn, seeds=ts)
        part = host.ambient_occlusion(tp, tn, outputs=("ao",), sort=False)
        got4 = host.ambient_occlusion(torch.nn.functional.pad(tp, (0, 1)), torch.nn.functional.pad(tn, (0, 1)), outputs=("occluded",))
        empty = host.ambient_occlusion(tp[:0], tn[:0])
    side.synchronize()
    assert got["ao"].dtype == torch.float32 and got["occluded"].dtype == torch.uint32 and got["ao"].device.type == "cuda"
    assert qo.same_words(got["ao"].cpu().numpy(), want["ao"]).all()
    assert np.array_equal(got["occluded"].cpu().numpy(), want["occluded"])
    assert set(part) == {"ao"} and qo.same_words(part["ao"].cpu().numpy(), want["ao"]).all()
    assert set(got4) == {"occluded"} and np.array_equal(got4["occluded"].cpu().numpy(), want["occluded"])
    assert empty["ao"].shape == (0,) and empty["occluded"].shape == (0,)
    assert host.last_query_ms > 0.0
    host.close()
    print("AO_QUERY_TORCH_OK", int(want["occluded"].sum()), "occluded rays at", n, "points")


if __name__ == "__main__":
    main()
