"""Child process of tests/test_views_gpu.py::test_torch_path_equals_numpy_path: torch's HIP runtime comes up first, then
the library; Host.render_views(as_torch=True) under a stream of the caller's -- in one chunk and in several -- must equal
the numpy path; so must a layers call with the ambient-occlusion step enqueued behind them on that stream, which leaves
rt_debug_last_views as the views calls left it."""
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


def same(t, want) -> bool:
    return bool(lo.same_words(t.cpu().numpy(), want).all())


def main():
    scene = rt.Scene.load_off(bunny_path()).build_bvh(1)
    opt = rt.Options.defaults(width=37, height=23, n_super_samples=4, ao_num_samples=3)
    host = rt.Host(opt, 0)
    host.upload_scene(scene)
    far = rt.Camera.from_vectors((0.6e7, 0.2e7, 1.0e7), (1, 0, 0), (0, 1, 0), (0, 0, -1))
    cams = [rt.Camera.look_at((1.2, 0.8, 1.4), (0, 0.1, 0)), far, rt.Camera.default(), rt.Camera.look_at((-1.5, 0.3, -1.3), (0, 0, 0)),
            rt.Camera.look_at((0, 2, 0), (0, 0, 0), up=(0, 0, -1))]
    want = host.render_views(cams, rt.VIEW_OUTPUTS)
    hits = int(want["hit"].sum())
    assert want["hit"][0].any() and not want["hit"][1].any() and not want["hit"].all() and want["image"].any()
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):
        got = host.render_views(cams, rt.VIEW_OUTPUTS, as_torch=True)
        assert host.last_views() == {"views": 5, "chunks": 1, "ao_points": hits}
        part = host.render_views(np.stack([c.as_array() for c in cams]), ("image", "leaf"), as_torch=True)
        depth = got["distance"] * 2.0  # (stream-ordered work on a layer)
        host.set_views_chunk(2)  # 2 + 2 + 1 inside one enqueued call
        chunked = host.render_views(cams, rt.VIEW_OUTPUTS, as_torch=True)
        assert host.last_views() == {"views": 5, "chunks": 3, "ao_points": hits}
        host.set_views_chunk(0)
        # a layers call with the ambient-occlusion step behind them on the same stream: enqueued like the rest, and no
        # views call -- what the last one did stays on the books
        done = host.last_views()
        layers = host.render_layers(("hit", "ao", "value"), as_torch=True)
        assert host.last_views() == done
    side.synchronize()
    layers_want = host.render_layers(("hit", "ao", "value"))
    assert host.last_views() == done
    for name in ("hit", "ao", "value"):
        assert layers[name].device.type == "cuda" and layers[name].cpu().numpy().view(np.uint8).tobytes() == layers_want[name].view(np.uint8).tobytes(), name
    assert layers_want["hit"].any() and not layers_want["hit"].all()
    assert host.last_query_ms > 0.0
    for name in rt.VIEW_OUTPUTS:
        for t in (got[name], chunked[name]):
            assert t.device.type == "cuda" and t.device.index == 0 and tuple(t.shape) == want[name].shape, name
            assert same(t, want[name]), name
    assert got["leaf"].dtype == torch.uint32 and got["hit"].dtype == torch.uint8 and got["image"].dtype == torch.uint8
    assert got["normal"].dtype == torch.float32 and tuple(got["image"].shape) == (5, 23, 37)
    assert set(part) == {"image", "leaf"} and same(part["image"], want["image"]) and same(part["leaf"], want["leaf"])
    assert same(depth, want["distance"] * np.float32(2.0))
    # the host renders its own view as before
    host.render()
    unposed = host.render_layers(("value",))["value"]
    assert np.array_equal(host.download().view(np.uint32), unposed.view(np.uint32))
    host.close()
    print("VIEWS_TORCH_OK", hits, "hits in", want["hit"].size)


if __name__ == "__main__":
    main()
