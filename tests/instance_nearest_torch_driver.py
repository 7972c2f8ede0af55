"""Child process of tests/test_instance_nearest_gpu.py::test_torch_path_equals_numpy_path: torch's HIP runtime comes up first,
then the library; a device tensor in and device tensors out on a non-default stream must equal the numpy path -- on an
uploaded scene, and after an update given as tensors, one of them with a coordinate that is no number (the form whose
coordinates only the device sees: every pair is looked at, and the oracle's brute force stands)."""
import os
import sys

import torch

torch.zeros(1, device="cuda:0")  # (before the library is loaded)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np  # noqa: E402

import instance_nearest_cases as inc  # noqa: E402
import instance_nearest_oracle as ino  # noqa: E402
import opencl_raytracer_amd as rt  # noqa: E402


def same(got, want, what):
    for f in got:
        assert ino.same_words(got[f].cpu().numpy(), want[f]).all(), (what, f)


def main():
    scene = rt.Scene.load_off(os.path.join(HERE, "golden", "meshes", "blob.off")).build_bvh(1)
    mesh = inc.Mesh(scene)
    host = rt.Host(rt.Options.defaults(width=64, height=48), 0)
    host.upload_scene(scene)
    host.set_instances(mesh.family("shear"))
    plan = host.instances()
    points = np.concatenate([inc.in_top_box(plan, 20000, 41), inc.odd_points(plan)])
    want = host.instances_closest_points(points)
    near = host.instances_closest_points(points, 0.3)
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):
        tp = torch.from_numpy(points).to("cuda:0")
        got = host.instances_closest_points(tp)
        got_near = host.instances_closest_points(tp, 0.3, sort=False)
        part = host.instances_closest_points(torch.nn.functional.pad(tp, (0, 1)), outputs=("instance", "normal"))
    side.synchronize()
    same(got, want, "upload")
    same(got_near, near, "radius")
    assert set(part) == {"instance", "normal"}
    same(part, want, "subset")
    assert got["instance"].dtype == torch.uint32 and got["hit"].device.type == "cuda"
    same({k: v[:1500] for k, v in got.items()}, mesh.oracle(plan, points[:1500]), "oracle")
    moved = mesh.vertices.copy()
    moved[:, :3] += np.float32(0.05) * np.sin(7.0 * mesh.vertices[:, [1, 2, 0]]).astype(np.float32)
    broken = moved.copy()
    broken[int(scene.faces[3 * 17]), 1] = np.nan
    for what, v in (("moved", moved), ("broken", broken)):
        with torch.cuda.stream(side):
            host.update_vertices(torch.from_numpy(v).to("cuda:0"))
            got = host.instances_closest_points(tp[:1500])
        side.synchronize()
        mesh.vertices = v
        same(got, mesh.oracle(host.instances(), points[:1500]), what)
    host.close()
    print("INSTANCE_NEAREST_TORCH_OK", int(want["hit"].sum()), "found of", len(points))


if __name__ == "__main__":
    main()
