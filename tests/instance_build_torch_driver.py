"""Child process of tests/test_instance_build_gpu.py::test_tensor_form: torch's HIP runtime comes up first, then the library.
host.build_instances(tensor) -- the tensor's own pointer, on the default and on a side stream -- must leave the bytes the numpy
form leaves and the host restatement's; the tensor may be reused on return; a bad transform in a tensor is refused and the set
stays; queries on the set built from a tensor equal the oracle; and the binding refuses the wrong dtype, shape, device, a
tensor that is not contiguous and a misaligned pointer."""
import os
import sys

import torch

torch.zeros(1, device="cuda:0")  # (before the library is loaded)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np  # noqa: E402

import instance_build_cases as bc  # noqa: E402
import instance_cases as cases  # noqa: E402
import instance_oracle as io  # noqa: E402
import opencl_raytracer_amd as rt  # noqa: E402
import orc  # noqa: E402

EMPTY = np.zeros((0, 3, 4), np.float32)


def read_back(host):
    plan = host.instances()
    plan["bounds"] = host.instance_bounds()
    return plan


def raises(kind, call):
    try:
        call()
    except kind as e:
        return e
    raise AssertionError(f"{kind.__name__} was not raised")


def main():
    scene = rt.Scene.load_off(os.path.join(HERE, "golden", "meshes", "blob.off")).build_bvh(0)
    arrays = orc.SceneArrays.from_scene(scene)
    lo, hi = cases.root_box(arrays)
    host = rt.Host(rt.Options.defaults(width=64, height=48), 0)
    host.upload_scene(scene)
    side = torch.cuda.Stream(device="cuda:0")
    for n in (1, 2, 257, 1000, 65537):
        W = cases.many(arrays, n, seed=7)
        host.build_instances(W)
        first = read_back(host)
        host.build_instances(EMPTY)
        for stream in (None, side):
            with torch.cuda.stream(stream):
                t = torch.from_numpy(W).to("cuda:0")
                host.build_instances(t)
                t.zero_()  # (the caller's array may be reused on return: the library keeps its own copy)
            torch.cuda.synchronize()
            second = read_back(host)
            for f in first:
                assert first[f].tobytes() == second[f].tobytes(), (n, f, stream is side)
            assert second["world_from_object"].tobytes() == W.tobytes(), n
        want = rt.instance_plan_lbvh(lo, hi, W)
        for f in ("object_from_world", "nodes", "bounds"):
            assert second[f].tobytes() == want[f].tobytes(), (n, f)
    # queries on the set built from a tensor
    W = cases.many(arrays, 257, seed=11)
    t = torch.from_numpy(W).to("cuda:0")
    host.build_instances(t)
    plan = read_back(host)
    o, d = cases.rays(plan["nodes"], 2000, seed=83)
    answer = host.trace_instances_closest(o, d)
    io.assert_same(answer, io.closest(arrays, plan, o, d, 1e5), "built from a tensor")
    # refusals found on the device: the set stays
    for name, bad in bc.bad_transforms(arrays).items():
        for at in (0, 128, 256):
            odd = W.copy()
            odd[at] = bad
            e = raises(rt.RtError, lambda: host.build_instances(torch.from_numpy(odd).to("cuda:0")))
            assert e.code == -1, (name, at)
        after = read_back(host)
        for f in plan:
            assert plan[f].tobytes() == after[f].tobytes(), (name, f)
    io.assert_same(host.trace_instances_closest(o, d), answer, "after the refusals")
    # the binding's errors
    both = torch.from_numpy(np.concatenate([W, W])).to("cuda:0")
    flat = torch.zeros(257 * 12 + 1, dtype=torch.float32, device="cuda:0")
    for name, bad in (("dtype", t.double()), ("shape", t[:, :, :3].contiguous()), ("rank", t.reshape(-1, 12)), ("a CPU tensor", torch.from_numpy(W)),
                      ("strided", both[::2]), ("transposed", t.permute(0, 2, 1).contiguous().permute(0, 2, 1)),
                      ("misaligned", flat[1:].reshape(257, 3, 4))):
        raises(ValueError, lambda: host.build_instances(bad))
    assert rt.load_library().rt_build_instances_device(host._h, flat.data_ptr() + 4, 257, None) == -1
    assert read_back(host)["nodes"].tobytes() == plan["nodes"].tobytes()
    host.build_instances(t[:0])
    assert int(rt.load_library().rt_instance_count(host._h)) == 0
    host.close()
    print("INSTANCE_BUILD_TORCH_OK")


if __name__ == "__main__":
    main()
