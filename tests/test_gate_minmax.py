"""CPU: tests/gate_minmax_check.cc -- the select form of the exact leaf gate (kernels/walk.hip.h, exact_leaf_gate) against
the min / max form that needs no selects: equal on the domain of finite, non-zero reciprocals, different outside it.

This pins an ARGUMENT, not code: the min / max form is in no kernel (it lost its A/B behind the branch it needs,
profiles/ao_tile_setup_notes.md section 2), and the select form here is a copy of exact_leaf_gate's arithmetic.  It is kept
so that the next attempt at the gate starts from the counter-example instead of finding it on the GPU."""
import os
import subprocess

from conftest import ROOT


def test_select_and_minmax_forms_of_the_leaf_gate(tmp_path):
    """20 M generated (box, ray, below) triples -- flat boxes, origins on box planes, reciprocals of either sign at both
    ends of the selectable range, coordinates up to 1e6, `below` from the smallest denormal to 1e5 --: no disagreement.
    With infinite reciprocals allowed the same run must show disagreements: why the kernel keeps the select form."""
    exe = tmp_path / "gate_minmax_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-o", str(exe),
                    os.path.join(ROOT, "tests", "gate_minmax_check.cc")], check=True)
    r = subprocess.run([str(exe), "20000000"], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "20000000 triples" in r.stdout and " 0 disagreements" in r.stdout
    r = subprocess.run([str(exe), "2000000", "1"], capture_output=True, text=True)
    assert r.returncode == 0, "no disagreement with infinite reciprocals: the check has no teeth\n" + r.stdout[-500:]
