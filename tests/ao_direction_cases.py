"""The direction counts tests/test_ao_direction_counts_{cpu,gpu}.py use, and why each is there.

`ao_dirs`, the table directions per hit, selects the form the ambient-occlusion pass takes (kernels/ao.hip.h): a wave's
claim is a fraction of it, a half-tile claim is half of it, the LDS cursor that deals a claim out holds 15 bits of it
(`end << 16 | next`: the cursor form below 0x8000 only), and only an even count can be claimed in halves.

The count of a ring is (unsigned) (2 pi cos(elevation) / step) + 1.  From 23 rings on (default angles 4 .. 90 degrees)
the last rings lie beyond 90 degrees and that quotient is NEGATIVE: the conversion is undefined in the reference's
language and in this project's, and gave 2^32 - n on the host (a loop of four thousand million turns per ring in the
oracle, a table of 64 GiB in the library).  Both now take 0 there, as the GPU's own conversion does: such a ring casts ONE
ray, its azimuth 0 / 0 = NaN, which hits nothing.  The counts below are those (`dirs`), asserted from the oracle's table
by the CPU test -- a change to the table moves a case out of its form, and the test says so.
"""
from collections import namedtuple

Rung = namedtuple("Rung", "rings amin amax aod dirs parity limit half_mod4")
# parity: dirs % 4 (odd counts are never split); limit: dirs against 0x8000; half_mod4: (dirs // 2) % 4 for even counts --
# not 0: four fixed shares of ceil(half / 4) overrun a half-tile claim, the defect tile_order.cc now keeps out of reach

LIMIT = 0x8000


def rung(rings, dirs, amin=4, amax=90, aod=0.2):
    return Rung(rings, amin, amax, aod, dirs, dirs % 4, "below" if dirs < LIMIT else "at" if dirs == LIMIT else "above",
                None if dirs & 1 else (dirs // 2) % 4)


SMALL = {
    "d4": rung(1, 4),                      # the smallest table: a claim of 1 unit per wave
    "d14": rung(2, 14),                    # 2 mod 4: half = 7, a half-tile claim in quarters of 2 with one short
    "d71": rung(5, 71),                    # odd: no tile is ever split
    "d262": rung(10, 262),                 # 2 mod 4 again, half = 131
    "d371": rung(12, 371),                 # a few hundred, odd
    "d371_far": rung(12, 371, aod=10.0),   # ... with AO_MAX_DISTANCE beyond the scene: no walk interval narrows anything
    "d79_alpha": rung(4, 79, 10, 60),      # other angles
    "d2206": rung(30, 2206),               # a few thousand; the last ring is a single NaN ray as described above
}
LARGE = {
    "d32168": rung(116, 32168),            # below the limit, even, half 0 mod 4: split claims, dealt by the cursor
    "d32526_alpha": rung(110, 32526, 10, 80),  # below, even, half 3 mod 4, other angles (no ring beyond 90 degrees)
    "d32719": rung(117, 32719),            # the last count below the limit with the default angles; odd
    "d33283": rung(118, 33283),            # the first above it; odd
    "d34986": rung(121, 34986),            # above, even, half 17493 = 1 mod 4: the case whose split claims overran
}
ALL = {**SMALL, **LARGE}
