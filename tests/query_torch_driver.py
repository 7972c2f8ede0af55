"""Child process of tests/test_query_gpu.py::test_torch_path_equals_numpy_path: torch's HIP runtime comes up first, then
the library; device tensors in and out on a non-default stream must equal the numpy path."""
import os
import sys

import torch

torch.zeros(1, device="cuda:0")  # (before the library is loaded)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np  # noqa: E402

import opencl_raytracer_amd as rt  # noqa: E402
import query_oracle as qo  # noqa: E402
from tools.meshes import bunny_path  # noqa: E402

FIELDS = ("hit", "distance", "leaf", "barycentric", "position", "normal")


def main():
    scene = rt.Scene.load_off(bunny_path()).build_bvh(1)
    host = rt.Host(rt.Options.defaults(width=64, height=48), 0)
    host.upload_scene(scene)
    rng = np.random.default_rng(21)
    lo, hi = scene.aabbs[0, :3], scene.aabbs[1, :3]
    n = 50000
    o = (lo + rng.random((n, 3), dtype=np.float32) * (hi - lo)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    want = host.trace_closest(o, d)
    occ = host.trace_occluded(o, d, 0.2)
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):
        to = torch.from_numpy(o).to("cuda:0")
        td = torch.from_numpy(d).to("cuda:0")
        got = host.trace_closest(to, td)
        tocc = host.trace_occluded(to, td, 0.2)
        part = host.trace_closest(to, td, outputs=("leaf", "normal"), sort=False)
        t4 = torch.nn.functional.pad(to, (0, 1))
        got4 = host.trace_closest(t4, torch.nn.functional.pad(td, (0, 1)), outputs=("distance",))
    side.synchronize()
    for f in FIELDS:
        assert qo.same_words(got[f].cpu().numpy(), want[f]).all(), f
    assert np.array_equal(tocc.cpu().numpy(), occ)
    assert np.array_equal(occ, host.trace_closest(o, d, 0.2, outputs=("hit",))["hit"])  # (the same max_distance)
    assert set(part) == {"leaf", "normal"}
    assert np.array_equal(part["leaf"].cpu().numpy(), want["leaf"])
    assert qo.same_words(part["normal"].cpu().numpy(), want["normal"]).all()
    assert qo.same_words(got4["distance"].cpu().numpy(), want["distance"]).all()
    assert got["leaf"].dtype == torch.uint32 and got["hit"].device.type == "cuda"
    host.close()
    print("QUERY_TORCH_OK", int(want["hit"].sum()), "hits of", n)


if __name__ == "__main__":
    main()
