"""Child process of tests/test_multihit_gpu.py::test_torch_path_equals_numpy_path: torch's HIP runtime comes up first,
then the library; device tensors in and out on a non-default stream must equal the numpy path."""
import os
import sys

import torch

torch.zeros(1, device="cuda:0")  # (before the library is loaded)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np  # noqa: E402

import opencl_raytracer_amd as rt  # noqa: E402
from query_oracle import same_words  # noqa: E402

FIELDS = ("count", "distance", "leaf", "barycentric", "position", "normal")


def main():
    scene = rt.Scene.load_off(os.path.join(HERE, "golden", "meshes", "blob.off")).build_bvh(1)
    host = rt.Host(rt.Options.defaults(width=64, height=48), 0)
    host.upload_scene(scene)
    rng = np.random.default_rng(21)
    lo, hi = scene.aabbs[0, :3], scene.aabbs[1, :3]
    n = 20000
    o = (lo + rng.random((n, 3), dtype=np.float32) * (hi - lo)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    want = host.trace_multihit(o, d, k=4)
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):
        to = torch.from_numpy(o).to("cuda:0")  # (N, 3): padded on the device
        td = torch.from_numpy(d).to("cuda:0")
        got = host.trace_multihit(to, td, k=4)
        part = host.trace_multihit(to, td, k=4, outputs=("leaf", "normal"), sort=False)
        counts = host.count_hits(to, td)
    side.synchronize()
    for f in FIELDS:
        assert got[f].shape == want[f].shape, f
        assert same_words(got[f].cpu().numpy(), want[f]).all(), f
    assert set(part) == {"leaf", "normal"}
    assert np.array_equal(part["leaf"].cpu().numpy(), want["leaf"])
    assert same_words(part["normal"].cpu().numpy(), want["normal"]).all()
    assert np.array_equal(counts.cpu().numpy(), want["count"])
    assert got["leaf"].dtype == torch.uint32 and got["count"].dtype == torch.uint32 and got["distance"].device.type == "cuda"
    assert int(want["count"].max()) > 1
    host.close()
    print("MULTIHIT_TORCH_OK", int(want["count"].sum()), "crossings of", n, "rays")


if __name__ == "__main__":
    main()
