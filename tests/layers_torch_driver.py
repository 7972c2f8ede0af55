"""Child process of tests/test_layers_gpu.py::test_torch_path_equals_numpy_path: torch's HIP runtime comes up first, then
the library; Host.render_layers(as_torch=True) on the default stream and under a stream of the caller's must equal the
numpy path."""
import os
import sys

import torch

torch.zeros(1, device="cuda:0")  # (before the library is loaded)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np  # noqa: E402

import opencl_raytracer_amd as rt  # noqa: E402
import layers_oracle as lo  # noqa: E402
from tools.meshes import bunny_path  # noqa: E402


def main():
    scene = rt.Scene.load_off(bunny_path()).build_bvh(1)
    opt = rt.Options.defaults(width=37, height=23, n_super_samples=4, ao_num_samples=3)
    host = rt.Host(opt, 0)
    host.set_camera(rt.Camera.look_at((1.2, 0.8, 1.4), (0, 0.1, 0)))
    host.upload_scene(scene)
    want = host.render_layers()
    assert want["hit"].any() and not want["hit"].all()
    got = host.render_layers(as_torch=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):
        under = host.render_layers(as_torch=True)
        part = host.render_layers(("value", "leaf"), as_torch=True)
        depth = under["distance"] * 2.0  # (stream-ordered work on a layer)
    side.synchronize()
    for name in rt.LAYER_OUTPUTS:
        for t in (got[name], under[name]):
            assert t.device.type == "cuda" and t.device.index == 0 and tuple(t.shape) == want[name].shape, name
            assert lo.same_words(t.cpu().numpy(), want[name]).all(), name
    assert got["leaf"].dtype == torch.uint32 and got["hit"].dtype == torch.uint8 and got["normal"].dtype == torch.float32
    assert set(part) == {"value", "leaf"}
    assert lo.same_words(part["value"].cpu().numpy(), want["value"]).all() and np.array_equal(part["leaf"].cpu().numpy(), want["leaf"])
    assert lo.same_words(depth.cpu().numpy(), want["distance"] * np.float32(2.0)).all()
    host.render()
    assert np.array_equal(host.download().view(np.uint32), want["value"].view(np.uint32))
    host.close()
    print("LAYERS_TORCH_OK", int(want["hit"].sum()), "hits of", want["hit"].size)


if __name__ == "__main__":
    main()
