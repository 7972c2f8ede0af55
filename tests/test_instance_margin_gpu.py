"""GPU: the instanced queries on the sets that push the instance box margin (instance_cases.HARD_FAMILIES) with the rays that
graze the top-level boxes (instance_cases.margin_rays; tests/test_instance_margin_cpu.py has the property and its sweep).

Every form is compared word for word with its C oracle on the plan read back from the device, and that plan with the
host-only planner's; the closest form is also compared with the oracle on the OPEN plan -- every leaf box (-inf, +inf) -- over
the rays whose open answer is a hit clearly inside a triangle: no box on the device culls a copy in which the lane would have
found such a hit.  The closest-point form is compared with the brute-force oracle, which visits every copy and every
triangle, so that a prune that is wrong under a non-rigid map shows as a different word.

Left out on purpose: the float64 comparators (tests/instance_reference.py, tests/instance_nearest_reference.py) with their
existing TOL.  Those thresholds were measured on well-conditioned maps; legitimate binary32 differences exceed them when the
inverse's entries are large, and scaling them by the condition number is a separate piece of work."""
import numpy as np
import pytest

import geometry_reference as gr
import instance_cases as cases
import instance_multihit_oracle as imo
import instance_nearest_cases as inc
import instance_nearest_oracle as ino
import instance_oracle as io
import instance_segment_oracle as iso

pytestmark = pytest.mark.gpu

N_RAYS = 2000
B = gr.M
FAR = 3e38
K = 4
INTERVAL = (1e-4, 1 - 1e-4)  # the segment queries' default: fractions of the segment


@pytest.fixture(scope="module")
def posed(rt, scene_for):
    """family -> (host with blob/sah uploaded and the family set, arrays, the device's plan, the open plan, rays, the open
    answer): one host per family, kept for the tests of this file."""
    scene, arrays = scene_for("blob", "sah")
    made = {}

    def get(family):
        if family not in made:
            W = cases.family(family, arrays)
            host = rt.Host(rt.Options.defaults(width=64, height=48, n_super_samples=1), 0)
            host.upload_scene(scene)
            host.set_instances(W)
            plan = host.instances()
            real, opened = cases.margin_plans(rt, arrays, W)
            o, d = cases.margin_rays(arrays, real, W, N_RAYS, seed=4300 + cases.HARD_FAMILIES.index(family))
            answer = io.closest(arrays, opened, o, d, FAR)
            for v in answer.values():
                v.setflags(write=False)
            made[family] = (host, arrays, plan, real, opened, o, d, answer)
        return made[family]

    yield get
    for entry in made.values():
        entry[0].close()


@pytest.mark.parametrize("family", cases.HARD_FAMILIES)
def test_the_devices_plan_is_the_planners(posed, family):
    """The top-level nodes and the inverses read back equal rt.instance_plan on the device's root box, byte for byte."""
    _, _, plan, real, _, _, _, _ = posed(family)
    assert np.array_equal(plan["world_from_object"], real["world_from_object"])
    assert plan["nodes"].tobytes() == real["nodes"].tobytes()
    assert plan["object_from_world"].tobytes() == real["object_from_world"].tobytes()


@pytest.mark.parametrize("family", cases.HARD_FAMILIES)
def test_closest_and_occluded(posed, family):
    host, arrays, plan, _, opened, o, d, answer = posed(family)
    got = host.trace_instances_closest(o, d, FAR)
    io.assert_same(got, io.closest(arrays, plan, o, d, FAR), (family, "closest"))
    occluded = host.trace_instances_occluded(o, d, FAR)
    assert np.array_equal(occluded, got["hit"]) and np.array_equal(occluded, io.occluded(arrays, plan, o, d, FAR)), family
    # conservativeness on the device's records: on C the answer is the open plan's, and the ray is occluded
    C_rows = cases.clearly_inside(answer, B)
    print(f"MARGIN GPU {family}: |C| = {int(C_rows.sum())} of {N_RAYS}, instances hit {len(np.unique(answer['instance'][C_rows]))} of {len(plan['object_from_world'])}")
    assert C_rows.sum() >= N_RAYS // 6 and len(np.unique(answer["instance"][C_rows])) == len(plan["object_from_world"]), family
    io.assert_same({f: v[C_rows] for f, v in got.items()}, {f: v[C_rows] for f, v in answer.items()}, (family, "open plan"))
    assert (occluded[C_rows] == 1).all(), family
    # ... and with a finite max_distance on the device: twice the largest hit parameter of C
    r = answer["distance"].astype(np.float64) / np.linalg.norm(d.astype(np.float64), axis=1)
    finite = float(np.float32(2.0 * r[C_rows].max()))
    io.assert_same(host.trace_instances_closest(o, d, finite), io.closest(arrays, plan, o, d, finite), (family, "closest", finite))


@pytest.mark.parametrize("family", cases.HARD_FAMILIES)
def test_multihit(posed, family):
    host, arrays, plan, _, _, o, d, _ = posed(family)
    got = host.trace_instances_multihit(o, d, FAR, k=K)
    want = imo.multihit(arrays, plan, o, d, FAR, K)
    assert set(got) == set(want) and want["count"].any()
    imo.assert_same(got, want, (family, "multihit"))


@pytest.mark.parametrize("family", cases.HARD_FAMILIES)
def test_segment_pair_forms(posed, family):
    """Segments from the origin to 1.5 x the open plan's hit point (without one: to the origin plus the direction)."""
    host, arrays, plan, _, _, o, d, answer = posed(family)
    found = np.isfinite(answer["distance"])[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        b = np.where(found, o + np.float32(1.5) * (answer["position"] - o), o + d).astype(np.float32)
    assert np.isfinite(b).all()
    got = host.instances_segments_closest(o, b, INTERVAL)
    want = iso.closest(arrays, plan, o, b, INTERVAL)
    iso.assert_same(got, want, (family, "segments"))
    assert want["hit"].any()
    assert np.array_equal(host.instances_segments_occluded(o, b, INTERVAL), got["hit"]), family


@pytest.mark.parametrize("family", ["ill", "tiny_huge", "wide", "far_ill"])
def test_closest_points(rt, scene_for, posed, family):
    """About 1500 points -- in the world box, on the world surface, far away -- with radius +inf and 0.3 x the world diagonal."""
    host, _, plan, _, _, _, _, _ = posed(family)
    mesh = inc.Mesh(scene_for("blob", "sah")[0])
    points = np.concatenate([inc.in_top_box(plan, 700, 4400), inc.on_world_surface(mesh, plan, 500, 4401), inc.far_from_set(plan, 150, 4402),
                             inc.far_from_set(plan, 150, 4403, sizes=2.0)])
    lo, hi = cases.top_box(plan["nodes"])
    for radius in (np.inf, float(np.float32(0.3 * np.linalg.norm(hi - lo)))):
        got = host.instances_closest_points(points, radius)
        want = mesh.oracle(plan, points, radius)
        ino.assert_same(got, want, (family, "closest points", radius))
        assert want["hit"].any()
