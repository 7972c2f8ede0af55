"""Child process of tests/test_directional_gpu.py::test_device_memory_form_equals_host_memory_form: torch's HIP runtime comes
up first, then the library; device tensors in and out on a non-default stream must equal the numpy path."""
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


def words(t):
    a = t.cpu()
    return a.view(torch.int32).numpy().view(np.uint32) if a.dtype == torch.uint32 else a.numpy()


def run(method: int, samples: int) -> int:
    scene = rt.Scene.load_off(bunny_path()).build_bvh(1)
    host = rt.Host(rt.Options.defaults(width=64, height=48, ao_num_samples=samples, ao_method=method), 0)
    host.upload_scene(scene)
    o4, d4 = qo.camera_rays(orc.params_from_options(rt.Options.defaults(width=96, height=72, n_super_samples=1)))
    cam = host.trace_closest(o4, d4)
    hit = cam["hit"].astype(bool)
    points, normals = cam["position"][hit], cam["normal"][hit]
    n, (R, _) = len(points), host.ao_rays_per_point
    seeds = np.flatnonzero(hit).astype(np.uint32)
    want = host.directional_occlusion(points, normals, seeds=seeds)
    want_rays = host.ao_rays(points, normals, seeds=seeds)
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):
        tp = torch.from_numpy(points).to("cuda:0")
        tn = torch.from_numpy(normals).to("cuda:0")
        ts = torch.from_numpy(seeds.view(np.int32)).to("cuda:0").view(torch.uint32)
        got = host.directional_occlusion(tp, tn, seeds=ts)
        unsorted = host.directional_occlusion(tp, tn, seeds=ts, sort=False)
        alone = {f: host.directional_occlusion(tp, tn, seeds=ts, outputs=(f,)) for f in rt.DIRECTIONAL_OUTPUTS}
        padded = host.directional_occlusion(torch.nn.functional.pad(tp, (0, 1)), torch.nn.functional.pad(tn, (0, 1)), seeds=ts,
                                            outputs=("mask",))
        rays = host.ao_rays(tp, tn, seeds=ts)
        flags = rt.unpack_ao_mask(got["mask"], R)
        empty = host.directional_occlusion(tp[:0], tn[:0])
        nothing = host.directional_occlusion(tp, tn, outputs=())
    side.synchronize()
    assert got["mask"].dtype == torch.uint32 and got["mask"].shape == (n, (R + 31) // 32) and got["mask"].device.type == "cuda"
    assert got["bent"].dtype == torch.float32 and got["bent"].shape == (n, 3)
    for f in rt.DIRECTIONAL_OUTPUTS:
        for other in (got, unsorted, alone[f]):
            assert qo.same_words(words(other[f]), want[f]).all(), f
        assert set(alone[f]) == {f}
    assert np.array_equal(words(padded["mask"]), want["mask"])
    assert rays["origins"].shape == (n, 4) and rays["directions"].shape == (n, R, 4)
    for f in ("origins", "directions"):
        assert qo.same_words(rays[f].cpu().numpy(), want_rays[f]).all(), f
    assert flags.dtype == torch.bool and np.array_equal(flags.cpu().numpy(), rt.unpack_ao_mask(want["mask"], R))
    assert empty["mask"].shape == (0, (R + 31) // 32) and empty["bent"].shape == (0, 3) and nothing == {}
    assert host.last_query_ms > 0.0
    host.close()
    return int(want["occluded"].sum())


def main():
    uniform = run(0, 3)   # R = 28
    random = run(1, 31)   # R = 33: two words per row
    print("DIRECTIONAL_TORCH_OK", uniform, random, "occluded rays")


if __name__ == "__main__":
    main()
