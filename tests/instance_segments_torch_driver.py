"""Child process of tests/test_instance_segments_gpu.py::test_torch_path_equals_numpy_path: torch's HIP runtime comes up
first, then the library; device tensors in and device tensors out on a non-default stream must equal the numpy path -- the
pair forms (sorted and not, (N, 3) and (N, 4) inputs, a subset of the outputs) and the mask form (with and without a mask
array, so that the rows live in the caller's tensor and in the host's scratch) -- and the numpy path the oracle."""
import os
import sys

import torch

torch.zeros(1, device="cuda:0")  # (before the library is loaded)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np  # noqa: E402

import instance_cases  # noqa: E402
import instance_segment_cases as cases  # noqa: E402
import instance_segment_oracle as iso  # noqa: E402
import opencl_raytracer_amd as rt  # noqa: E402
import orc  # noqa: E402


def same(got, want, what):
    for f in got:
        assert iso.same_words(got[f].cpu().numpy(), want[f]).all(), (what, f)


def main():
    scene = rt.Scene.load_off(os.path.join(HERE, "golden", "meshes", "blob.off")).build_bvh(1)
    arrays = orc.SceneArrays.from_scene(scene)
    host = rt.Host(rt.Options.defaults(width=64, height=48), 0)
    host.upload_scene(scene)
    host.set_instances(instance_cases.family("grid", arrays))
    plan = host.instances()
    a, b = cases.box_segments(plan["nodes"], 20000, seed=83)
    odd_a, odd_b, _ = cases.odd_segments(arrays)
    a, b = np.concatenate([a, odd_a]), np.concatenate([b, odd_b])
    points, targets = cases.box_points(plan["nodes"], 700, 89), cases.box_points(plan["nodes"], 45, 90)
    want = host.instances_segments_closest(a, b)
    want_ray = host.instances_segments_closest(a, b, (-1.0, np.inf))
    want_mask = host.instances_visibility(points, targets)
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):
        ta, tb = torch.from_numpy(a).to("cuda:0"), torch.from_numpy(b).to("cuda:0")
        got = host.instances_segments_closest(ta, tb)
        occ = host.instances_segments_occluded(ta, tb, sort=False)
        got_ray = host.instances_segments_closest(torch.nn.functional.pad(ta, (0, 1)), torch.nn.functional.pad(tb, (0, 1)), (-1.0, np.inf),
                                                  sort=False)
        part = host.instances_segments_closest(ta, tb, outputs=("instance", "normal"))
        tp, tt = torch.from_numpy(points).to("cuda:0"), torch.from_numpy(targets).to("cuda:0")
        got_mask = host.instances_visibility(tp, tt)
        only_count = host.instances_visibility(tp, tt, outputs=("count",), sort=False)
        flags = rt.unpack_visibility_mask(got_mask["mask"], len(targets))
    side.synchronize()
    same(got, want, "closest")
    same(got_ray, want_ray, "closest, no far end")
    assert np.array_equal(occ.cpu().numpy(), want["hit"])
    assert set(part) == {"instance", "normal"}
    same(part, want, "subset")
    assert got["instance"].dtype == torch.uint32 and got["hit"].device.type == "cuda" and occ.dtype == torch.uint8
    same(got_mask, want_mask, "mask")
    assert set(only_count) == {"count"}
    same(only_count, want_mask, "count alone")
    assert np.array_equal(flags.cpu().numpy(), rt.unpack_visibility_mask(want_mask["mask"], len(targets)))
    iso.assert_same(want, iso.closest(arrays, plan, a, b, cases.INTERVALS[0]), "numpy path")
    expected = iso.mask_of(arrays, plan, points, targets, cases.INTERVALS[0])
    assert np.array_equal(want_mask["mask"], expected["mask"]) and np.array_equal(want_mask["count"], expected["count"])
    host.close()
    print("INSTANCE_SEGMENTS_TORCH_OK", int(want["hit"].sum()), "blocked of", len(a))


if __name__ == "__main__":
    main()
