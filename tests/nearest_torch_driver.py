"""Child process of tests/test_nearest_gpu.py::test_torch_path_equals_numpy_path: torch's HIP runtime comes up first, then
the library; a device tensor in and device tensors out on a non-default stream must equal the numpy path -- on an uploaded
scene, after an update and after a build given as tensors (the forms whose coordinates only the device sees)."""
import os
import sys

import torch

torch.zeros(1, device="cuda:0")  # (before the library is loaded)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np  # noqa: E402

import nearest_cases as cases  # noqa: E402
import nearest_oracle as orc_n  # noqa: E402
import opencl_raytracer_amd as rt  # noqa: E402

FIELDS = ("hit", "distance", "leaf", "barycentric", "position", "normal")


def same(got, want, what):
    for f in got:
        assert orc_n.same_words(got[f].cpu().numpy(), want[f]).all(), (what, f)


def main():
    scene = rt.Scene.load_off(os.path.join(HERE, "golden", "meshes", "blob.off")).build_bvh(1)
    host = rt.Host(rt.Options.defaults(width=64, height=48), 0)
    host.upload_scene(scene)
    vertices, normals = scene.vertices.copy(), scene.vnormals.copy()
    points = np.concatenate([cases.in_box(vertices, 20000, 41), cases.odd_points(vertices)])
    want = host.closest_points(points)
    near = host.closest_points(points, 0.02)
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):
        tp = torch.from_numpy(points).to("cuda:0")
        got = host.closest_points(tp)
        got_near = host.closest_points(tp, 0.02, sort=False)
        part = host.closest_points(torch.nn.functional.pad(tp, (0, 1)), outputs=("leaf", "normal"))
    side.synchronize()
    same(got, want, "upload")
    same(got_near, near, "radius")
    assert set(part) == {"leaf", "normal"}
    same(part, want, "subset")
    assert got["leaf"].dtype == torch.uint32 and got["hit"].device.type == "cuda"
    # an update given as tensors, one of them with a coordinate that is no number: every leaf is looked at, brute force stands
    moved = vertices.copy()
    moved[:, :3] += np.float32(0.05) * np.sin(7.0 * vertices[:, [1, 2, 0]]).astype(np.float32)
    broken = moved.copy()
    broken[int(scene.faces[3 * 17]), 1] = np.nan
    for what, v in (("moved", moved), ("broken", broken)):
        with torch.cuda.stream(side):
            host.update_vertices(torch.from_numpy(v).to("cuda:0"))
            got = host.closest_points(tp[:2000])
        side.synchronize()
        same(got, orc_n.closest_points(scene.sorted_faces, v, normals, points[:2000]), what)
    # a build given as tensors
    with torch.cuda.stream(side):
        host.build_scene(torch.from_numpy(vertices).to("cuda:0"), torch.from_numpy(scene.faces.reshape(-1, 3).astype(np.int32)).to("cuda:0"),
                         torch.from_numpy(normals).to("cuda:0"))
        got = host.closest_points(tp[:2000])
    side.synchronize()
    leaf_faces = scene.faces.reshape(-1, 3)[host.face_of_leaf()].reshape(-1)
    same(got, orc_n.closest_points(leaf_faces, vertices, normals, points[:2000]), "built")
    host.close()
    print("NEAREST_TORCH_OK", int(want["hit"].sum()), "found of", len(points))


if __name__ == "__main__":
    main()
