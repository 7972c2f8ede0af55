"""Child process of tests/test_signed_gpu.py::test_torch_path_equals_numpy_path: torch's HIP runtime comes up first, then the
library; device tensors in and out on a non-default stream -- the device forms of the point and grid queries -- must equal
the numpy path word for word, on an upload, after an update given as a tensor and after a build given as tensors."""
import os
import sys

import torch

torch.zeros(1, device="cuda:0")  # (before the library is loaded)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np  # noqa: E402

import nearest_cases as ncases  # noqa: E402
import opencl_raytracer_amd as rt  # noqa: E402
import signed_cases as cases  # noqa: E402
import signed_oracle as orc_s  # noqa: E402

GRID = (np.float32([-1.5, -1.5, -0.6]), np.float32([0.375, 0.5, 0.25]), (9, 6, 5))


def same(got, want, what):
    for f in got:
        assert orc_s.same_words(got[f].cpu().numpy(), want[f]).all(), (what, f)


def main():
    v, f = cases.torus()
    scene = rt.Scene.from_arrays(v, f).build_bvh(1)
    host = rt.Host(rt.Options.defaults(width=64, height=48), 0)
    host.upload_scene(scene)
    vertices, normals = scene.vertices.copy(), scene.vnormals.copy()
    points = np.concatenate([ncases.in_box(vertices, 20000, 41), ncases.odd_points(vertices)])
    want = host.signed_distance(points)
    orc_s.assert_same({k: x[:3000] for k, x in want.items()},
                      orc_s.signed_distance(scene.sorted_faces, vertices, normals, points[:3000]), "numpy path")
    grid, grid_leaf = host.signed_distance_grid(*GRID, leaf=True)
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):
        tp = torch.from_numpy(points).to("cuda:0")
        got = host.signed_distance(tp)
        near = host.signed_distance(tp, 0.02, sort=False)
        part = host.signed_distance(torch.nn.functional.pad(tp, (0, 1)), outputs=("distance", "feature"))
        tg, tl = host.signed_distance_grid(*GRID, as_torch=True, leaf=True)
        only = host.signed_distance_grid(*GRID, max_distance=0.3, as_torch=True)
    side.synchronize()
    same(got, want, "upload")
    same(near, host.signed_distance(points, 0.02), "radius")
    assert set(part) == {"distance", "feature"}
    same(part, want, "subset")
    assert got["feature"].dtype == torch.uint8 and got["pseudonormal"].shape == (len(points), 4) and got["hit"].device.type == "cuda"
    assert tg.shape == (5, 6, 9) and tl.dtype == torch.uint32
    assert orc_s.same_words(tg.cpu().numpy(), grid).all() and orc_s.same_words(tl.cpu().numpy(), grid_leaf).all()
    assert orc_s.same_words(only.cpu().numpy(), host.signed_distance_grid(*GRID, max_distance=0.3)).all()
    # an update given as a tensor: the table's sums are redone from the kept incidence
    moved = cases.sheared(vertices)
    with torch.cuda.stream(side):
        host.update_vertices(torch.from_numpy(moved).to("cuda:0"))
        got = host.signed_distance(tp[:3000])
    side.synchronize()
    same(got, orc_s.signed_distance(scene.sorted_faces, moved, normals, points[:3000]), "moved")
    # a build given as tensors: everything is made again
    with torch.cuda.stream(side):
        host.build_scene(torch.from_numpy(vertices).to("cuda:0"), torch.from_numpy(scene.faces.reshape(-1, 3).astype(np.int32)).to("cuda:0"),
                         torch.from_numpy(normals).to("cuda:0"))
        got = host.signed_distance(tp[:3000])
    side.synchronize()
    leaf_faces = scene.faces.reshape(-1, 3)[host.face_of_leaf()].reshape(-1)
    same(got, orc_s.signed_distance(leaf_faces, vertices, normals, points[:3000]), "built")
    host.close()
    print("SIGNED_TORCH_OK", int((want["distance"] < 0).sum()), "inside of", len(points))


if __name__ == "__main__":
    main()
