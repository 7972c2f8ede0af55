"""Child process of tests/test_instance_views_gpu.py::test_torch_path_equals_numpy_path: torch's HIP runtime comes up first,
then the library; instances_ambient_occlusion with device tensors in and out, and render_instance_views(as_torch=True) -- in
one chunk and in several --, under a stream of the caller's must equal the numpy path."""
import os
import sys

import torch

torch.zeros(1, device="cuda:0")  # (before the library is loaded)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np  # noqa: E402

import instance_cases as cases  # noqa: E402
import instance_views_oracle as ivo  # noqa: E402
import opencl_raytracer_amd as rt  # noqa: E402
import orc  # noqa: E402


def same(t, want) -> bool:
    return bool(ivo.same_words(t.cpu().numpy(), want).all())


def main():
    scene = rt.Scene.load_off(os.path.join(HERE, "golden", "meshes", "blob.off")).build_bvh(1)
    arrays = orc.SceneArrays.from_scene(scene)
    opt = rt.Options.defaults(width=37, height=23, n_super_samples=2, ao_num_samples=2, ao_max_distance=0.5)
    host = rt.Host(opt, 0)
    host.upload_scene(scene)
    host.set_instances(cases.many(arrays, 65, seed=3))
    plan = host.instances()
    cams = ivo.cameras(rt, plan)
    cams = [cams[0], cams[2], cams[1], cams[0], cams[1]]
    names = rt.INSTANCE_VIEW_OUTPUTS
    want = host.render_instance_views(cams, names)
    hit = want["hit"].astype(bool)
    hits = int(hit.sum())
    assert hit[0].any() and not hit[1].any() and want["image"].any() and len(np.unique(want["instance"][hit])) > 1
    # points for the query: the hit sub-pixels' own, repeated to 20000 (enough rays for the sort), and seeds that are not the index
    points = np.ascontiguousarray(np.resize(want["position"][hit], (20000, 3)))
    normals = np.ascontiguousarray(np.resize(want["normal"][hit], (20000, 3)))
    seeds = np.arange(20000, dtype=np.uint32)[::-1].copy()
    want_ao = host.instances_ambient_occlusion(points, normals, seeds)
    assert want_ao["occluded"].any()
    small = ivo.ao(orc.params_from_options(opt), arrays, plan, points[:300], normals[:300], seeds[:300])
    assert np.array_equal(small["occluded"], want_ao["occluded"][:300]) and ivo.same_words(small["ao"], want_ao["ao"][:300]).all()
    side = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(side):
        tp, tn = torch.from_numpy(points).to("cuda:0"), torch.from_numpy(normals).to("cuda:0")
        ts = torch.from_numpy(seeds.view(np.int32)).to("cuda:0").view(torch.uint32)
        got_ao = host.instances_ambient_occlusion(tp, tn, ts)
        unsorted = host.instances_ambient_occlusion(torch.nn.functional.pad(tp, (0, 1)), torch.nn.functional.pad(tn, (0, 1)), ts, sort=False)
        only = host.instances_ambient_occlusion(tp, tn, outputs=("occluded",))
        got = host.render_instance_views(cams, names, as_torch=True)
        assert host.last_views() == {"views": 5, "chunks": 1, "ao_points": hits}
        depth = got["distance"] * 2.0  # (stream-ordered work on a layer)
        host.set_views_chunk(2)  # 2 + 2 + 1 inside one enqueued call
        chunked = host.render_instance_views(np.stack([c.as_array() for c in cams]), names, as_torch=True)
        assert host.last_views() == {"views": 5, "chunks": 3, "ao_points": hits}
        host.set_views_chunk(0)
        part = host.render_instance_views(cams, ("image", "instance"), as_torch=True)
    side.synchronize()
    for f in ("ao", "occluded"):
        assert got_ao[f].device.type == "cuda" and same(got_ao[f], want_ao[f]) and same(unsorted[f], want_ao[f]), f
    assert got_ao["occluded"].dtype == torch.uint32 and got_ao["ao"].dtype == torch.float32
    assert set(only) == {"occluded"} and same(only["occluded"], host.instances_ambient_occlusion(points, normals)["occluded"])
    for name in names:
        for t in (got[name], chunked[name]):
            assert t.device.type == "cuda" and t.device.index == 0 and tuple(t.shape) == want[name].shape, name
            assert same(t, want[name]), name
    assert got["instance"].dtype == torch.uint32 and got["image"].dtype == torch.uint8 and tuple(got["image"].shape) == (5, 23, 37)
    assert set(part) == {"image", "instance"} and same(part["image"], want["image"]) and same(part["instance"], want["instance"])
    assert same(depth, want["distance"] * np.float32(2.0))
    assert host.last_query_ms > 0.0
    host.close()
    print("INSTANCE_VIEWS_TORCH_OK", hits, "hits in", want["hit"].size)


if __name__ == "__main__":
    main()
