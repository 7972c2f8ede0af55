"""CPU: the UNIFORM direction table at the ring counts tests/test_ao_direction_counts_gpu.py renders with -- its size, the
properties each count was chosen for, and the rings beyond 90 degrees of elevation (tests/ao_direction_cases.py)."""
import time

import numpy as np
import pytest

import orc
from ao_direction_cases import ALL, LIMIT


def params(r):
    p = orc.OrcParams()
    p.width, p.height, p.focal_length, p.shading_enable, p.ao_enable = 8, 8, 1.0, 1, 1
    p.ao_max_distance, p.ao_num_samples, p.ao_method, p.ao_alpha_min, p.ao_alpha_max = r.aod, r.rings, 0, r.amin, r.amax
    return p


def ring_counts(rings, amin, amax):
    """An independent float32 restatement of the count of every ring (src/intersect_kernel.cl:237-242), a negative
    quotient kept as it is."""
    f = np.float32
    degrees = f(np.pi / 180)
    alpha_min, alpha_max = f(amin) * degrees, f(amax) * degrees
    step = alpha_max / f(rings)
    out = []
    for c in range(rings):
        angle = step * f(c) + alpha_min
        out.append(float(f(2.0) * np.pi * float(np.cos(angle, dtype=np.float32))) / float(step))
    return out


@pytest.mark.parametrize("name", sorted(ALL))
def test_case_selection(oracle, name):
    """Each count is what the file says and has the property it was chosen for."""
    r = ALL[name]
    t0 = time.perf_counter()
    table = oracle.ao_table(params(r))
    assert time.perf_counter() - t0 < 1.0, "a ring's count wrapped: the table loop ran away"
    dirs = table.shape[0]
    assert dirs == r.dirs
    quotients = ring_counts(r.rings, r.amin, r.amax)
    assert dirs == sum((int(q) if q > 0 else 0) + 1 for q in quotients)
    assert r.parity == dirs % 4
    assert r.limit == ("below" if dirs < LIMIT else "at" if dirs == LIMIT else "above")
    assert r.half_mod4 == (None if dirs % 2 else (dirs // 2) % 4)
    # what the GPU file relies on, by name
    if name in ("d71", "d371", "d32719", "d33283"):
        assert dirs % 2 == 1
    if name in ("d14", "d262", "d2206", "d34986", "d32526_alpha"):
        assert dirs % 4 == 2
    if name == "d32168":
        assert dirs < LIMIT and dirs % 2 == 0 and r.half_mod4 == 0
    if name == "d32526_alpha":
        assert dirs < LIMIT and r.half_mod4 != 0 and min(quotients) > 0  # (no ring beyond 90 degrees with these angles)
    if name == "d32719":
        assert dirs < LIMIT and ALL["d33283"].rings == r.rings + 1  # the last below, the first above
    if name in ("d33283", "d34986"):
        assert dirs > LIMIT
    if name == "d34986":
        assert r.half_mod4 == 1 and 4 * -(-(dirs // 2) // 4) > dirs // 2  # four fixed shares cover more than the half
    # every direction of a ring with a positive count is a unit vector of the upper hemisphere; a ring beyond 90 degrees
    # is one entry whose azimuth is NaN
    beyond = sum(q <= 0 for q in quotients)
    nan_rows = np.isnan(table).any(axis=1)
    zero_count = sum(0 < q < 1 for q in quotients)  # (a count of 0 that is no accident: 0 / 0 as well)
    assert int(nan_rows.sum()) == beyond + zero_count
    good = table[~nan_rows].astype(np.float64)
    assert np.allclose(np.linalg.norm(good, axis=1), 1.0, atol=1e-6)
    if name in ("d2206", "d32168", "d32719", "d33283", "d34986"):
        assert beyond >= (1 if name == "d2206" else 4)


def test_rings_below_90_degrees_are_untouched(oracle):
    """Up to 22 rings (default angles) no quotient is negative: the table is what it always was (the golden frames pin
    its values; this pins that the guard is not taken)."""
    for rings in range(1, 23):
        assert min(ring_counts(rings, 4, 90)) > 0, rings
    assert min(ring_counts(23, 4, 90)) < 0
