"""CPU: the bound the closest-hit walk's pruning rests on (scene_pack.h, leaf_growth) under a sweep aimed at it
(tests/prune_bound_sweep.cc), and the conditions of the frames tests/test_prune_bound_gpu.py renders (tests/prune_traps.py),
from the reference's own tests alone."""
import re
import subprocess

import numpy as np
import pytest

import orc
import prune_traps as pt
import query_oracle as qo
from conftest import bits


@pytest.fixture(scope="module")
def sweep(rt, tmp_path_factory):
    return pt.sweep_program(tmp_path_factory.mktemp("prune_bound"))


def test_sweep_of_adversarial_triangles_and_rays_finds_no_hit_outside_its_grown_box(sweep):
    """5 M generated triangles -- eta from its least value to the 1/32 gate, edge ratios to 1e4, apex angles to 3e-4,
    coordinates to 1e6 --, 20 M rays aimed at the slack zone of every edge and corner from the reference's camera, random,
    grazing and box-parallel eyes, a local search on a share of them: 0 violations and every worst needed / granted growth
    below 1 (the invariant itself), with enough accepted hits per eta decade and in front of the leaves' own boxes for that
    to mean something (the program's own exit code); the leaves it makes are make_walk_array's, bit for bit."""
    r = subprocess.run([sweep, "sweep", "5000000"], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "prune_bound_sweep: ok" in r.stdout, r.stdout[-4000:]
    assert ": 0 violations" in r.stdout and ": 0 differ" in r.stdout
    worst = [float(x) for x in re.findall(r"worst needed / granted growth ([0-9.eE+-]+)", r.stdout)]
    assert len(worst) == 5 and all(w < 1.0 for w in worst), worst


def test_sweep_reports_violations_without_the_growth(sweep):
    """The teeth: with every finite growth multiplied by 0 the same run must report violations (exit code 0 only then).
    Factors 0.5 and 0.25 are run and printed for the headroom (profiles/prune_bound_notes.md); nothing asserts on them."""
    r = subprocess.run([sweep, "sweep", "1000000", "0"], capture_output=True, text=True)
    assert r.returncode == 0 and "violations are reported, as they must be" in r.stdout, r.stdout[-2000:]
    assert int(re.search(r": (\d+) violations", r.stdout).group(1)) > 0
    for factor in ("0.5", "0.25"):
        r = subprocess.run([sweep, "sweep", "1000000", factor], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:]
        print(r.stdout.splitlines()[-1])


def test_trees_with_faces_on_both_sides_of_the_gate(sweep):
    """Whole trees of 200 to 2000 faces, a sixth of them with eta in [1/64, 1/32), a sixth in [1/32, 1/8]: both copies hold
    every leaf once, skips tile, the faces without a bound -- and no others -- lie in the unpruned head, children nearest
    first outside it; every accepted hit inside its leaf's record and not pruned by any box above it."""
    r = subprocess.run([sweep, "trees"], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "prune_bound_sweep: trees ok" in r.stdout and ": 0 violations" in r.stdout, r.stdout[-4000:]


def test_posed_rays_restate_the_camera(rt):
    """prune_traps.posed_rays with the reference's pose gives query_oracle.camera_rays, bit for bit."""
    params = orc.params_from_options(pt.options(rt))
    o4, d4 = qo.camera_rays(params)
    po, pd = pt.posed_rays(params, pt.POSES["a"])
    assert np.array_equal(bits(o4), bits(po)) and np.array_equal(bits(d4), bits(pd))


_FACTS = {}


def trap_facts(rt, sweep, tmp_path_factory, placement):
    if placement not in _FACTS:
        vertices, faces, kinds = pt.trap_mesh(rt, placement)
        o4, d4 = pt.rays(rt, placement)
        _FACTS[placement] = (pt.facts(sweep, tmp_path_factory.mktemp("traps_" + placement), placement, vertices, faces, o4, d4), vertices, faces, kinds, o4, d4)
    return _FACTS[placement]


@pytest.mark.parametrize("placement", ["a", "b", "c"])
def test_trap_frames_trap(rt, sweep, tmp_path_factory, placement):
    """From the reference alone, before anything touches a GPU: traps in at least 90 % of the pixels of (a) and (b), at least
    64 trap pixels in (c); no Y or X face is a face without a bound; the stream walk array prunes (finite margin); the
    winners are the query oracle's."""
    f, vertices, faces, kinds, o4, d4 = trap_facts(rt, sweep, tmp_path_factory, placement)
    traps = int(f["trap"].sum())
    print(f"placement {placement}: {len(faces)} faces, {traps} trap pixels of {len(o4)}, margin {f['prune_margin']:.3g}")
    assert f["covered"] and np.isfinite(f["prune_margin"]) and f["unpruned_bytes"] == 0
    assert all(np.isfinite(g) and g > 0 for g in f["growth"]) and not any(f["loose"])
    assert sorted(f["face"]) == list(range(len(faces)))
    if placement == "c":
        assert traps >= 64
    else:
        assert len(faces) == 2 * pt.WIDTH and traps >= 0.9 * len(o4)
    # a trap's winner is a front triangle hit through the slack, and the query oracle (the whole tree, the reference's
    # walk) picks the same leaf for every ray
    for i in np.flatnonzero(f["trap"]):
        assert kinds[f["face"][f["winner"][i]]][0] == "Y"
    _, arrays = pt.product_scene(rt, vertices, faces)
    want = qo.closest(arrays, o4, d4, 100000.0)
    assert np.array_equal(want["hit"] != 0, f["winner"] >= 0)
    hit = f["winner"] >= 0
    assert np.array_equal(want["leaf"][hit], f["winner"][hit].astype(np.uint32))


@pytest.mark.parametrize("placement", ["a", "b", "c"])
def test_model_of_the_pruning_walk_loses_trap_pixels_without_the_growth(rt, rt_knobs, tmp_path_factory, monkeypatch, placement):
    """tests/prune_bound_sweep.cc `model`, linked against the A/B build: a sequential model of the walk with its far_limit
    on the stream walk array gives every ray the reference's leaf; with OCRT_PRUNE_GROWTH=0 it loses trap pixels -- the
    frames do reach the pruning, whatever a GPU says (the GPU test asserts the same of the kernel)."""
    exe = pt.sweep_program(tmp_path_factory.mktemp("prune_model"), "lib_knobs")
    vertices, faces, _ = pt.trap_mesh(rt, placement)
    off, ray_file = pt.write_scene(tmp_path_factory.mktemp("model_" + placement), placement, vertices, faces, *pt.rays(rt, placement))
    changed = {}
    for factor in ("1", "0"):
        monkeypatch.setenv("OCRT_PRUNE_GROWTH", factor)
        r = subprocess.run([exe, "model", off, ray_file], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        changed[factor] = int(re.search(r"(\d+) of \d+ rays end with another leaf", r.stdout).group(1))
        assert "(0 in packets of the exact form)" in r.stdout
    print(f"placement {placement}: the model loses {changed['0']} pixels without the growth, {changed['1']} with it")
    assert changed["1"] == 0 and changed["0"] >= 64


@pytest.mark.parametrize("ordinary_first", [False, True])
def test_ties_across_the_unpruned_head(rt, sweep, tmp_path_factory, ordinary_first):
    """The needle lies in the unpruned head, the ordinary face of its plane does not; rays through both get bit-equal
    distances; the reference's minimum of (distance, leaf) is the lower leaf -- the needle's in one scene, the ordinary
    face's in the other."""
    vertices, faces, names = pt.ties_mesh(ordinary_first)
    o4, d4 = pt.rays(rt, "a")
    f = pt.facts(sweep, tmp_path_factory.mktemp("ties"), "ties", vertices, faces, o4, d4)
    leaf_of = {names[face]: leaf for leaf, face in enumerate(f["face"]) if names[face] in "NOT"}
    n, o = leaf_of["N"], leaf_of["O"]
    assert np.isfinite(f["prune_margin"]) and f["unpruned_bytes"] == 2 * 32  # the root and the needle
    assert f["loose"][n] and np.isinf(f["growth"][n]) and 1 / 32 <= f["eta"][n] <= 1 / 8 + 1e-4
    assert not f["loose"][o] and np.isfinite(f["growth"][o])
    assert (o < n) == ordinary_first, "the two scenes differ in the order of the two leaves"
    ties = 0
    for i, accepted in enumerate(f["accepted"]):
        d = dict(accepted)
        if n in d and o in d:
            assert d[n] == d[o], "bit-equal distances"
            assert f["winner"][i] == min(n, o)
            ties += 1
    assert ties >= 128 and len(o4) - ties >= 128, ties
    _, arrays = pt.product_scene(rt, vertices, faces)
    want = qo.closest(arrays, o4, d4, 100000.0)
    assert np.array_equal(want["leaf"], f["winner"].astype(np.uint32))
