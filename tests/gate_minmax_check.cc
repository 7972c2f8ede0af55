// gate_minmax_check.cc -- the exact gate on a leaf's own box: its select form against a min / max form (CPU, no GPU
// needed, no library).
//
// exact_leaf_gate (opencl_raytracer_amd/csrc/kernels/walk.hip.h) picks the near and the far plane of each axis by the
// sign of the reciprocal: three compares and six selects, instructions of the slow class.  Taking the smaller and the
// larger of the two products instead needs neither.  Claim: for a regular box (lo <= hi, finite), a finite origin and
// FINITE, non-zero reciprocals the two booleans are equal -- lo <= hi gives fl(lo - o) <= fl(hi - o), rounding being
// monotonic; multiplying both by the same finite i keeps the order for i > 0 and reverses it for i < 0, again because
// rounding is monotonic; so the smaller product IS the near plane's, or the two are equal, -0 and +0 included, which
// max(.., tiny) and <= do not tell apart.  This program throws generated (box, ray, below) triples of that domain at
// both forms with the kernel's arithmetic (one rounding per operation, fmax / fmin like v_max / v_min: IEEE maxNum /
// minNum) and counts the disagreements.  Exit code 0 = none, and both answers were seen often enough.
//
// The domain: coordinates up to 1e6 in magnitude; boxes flat on one, two or three axes; origins in, near, on and one
// ulp off the box planes; reciprocals of either sign from 0.5 to 1e30 (the two ends of what ray_is_selectable lets
// through, RECIPROCAL_LIMIT), the ends themselves included; `below` from the smallest denormal to 1e5.
//
// Second argument 1 = the edge of that domain: INFINITE reciprocals (a zero direction component, which
// ray_is_selectable admits and the gate therefore meets: three of the headline's 28 table directions where the normal
// lies along an axis).  With the origin's coordinate ON a box plane 0 * inf is NaN, the select form then drops ONE bound of the axis -- the
// reference's behaviour -- where min / max replaces both by the other plane's +-inf: the forms must be SEEN to disagree
// there (exit code 0 = they were).  So the min / max form could only serve packets known to be tame (ray_is_tame: no
// infinite reciprocal), behind a branch -- which measured slower than the select form for every packet
// (profiles/ao_tile_setup_notes.md): the kernel keeps the select form, and this program keeps the reason.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <random>
#include <thread>
#include <vector>

namespace {

const float INF = std::numeric_limits<float>::infinity();
const float TINY = std::numeric_limits<float>::denorm_min();  // bit pattern 1

struct Case {
	float lo[3], hi[3], o[3], inv[3], below;
};

// walk.hip.h, exact_leaf_gate
bool gate_select(const Case &c) {
	float near[3], far[3];
	for (int k = 0; k < 3; ++k) {
		const float t0 = (c.lo[k] - c.o[k]) * c.inv[k], t1 = (c.hi[k] - c.o[k]) * c.inv[k];
		const bool positive = c.inv[k] >= 0.0f;
		near[k] = positive ? t0 : t1;
		far[k] = positive ? t1 : t0;
	}
	const float t_near = std::fmax(std::fmax(near[0], near[1]), std::fmax(near[2], TINY));
	const float t_far = std::fmin(std::fmin(far[0], far[1]), std::fmin(far[2], c.below));
	return t_near <= t_far;
}

// the min / max form
bool gate_minmax(const Case &c) {
	float near[3], far[3];
	for (int k = 0; k < 3; ++k) {
		const float t0 = (c.lo[k] - c.o[k]) * c.inv[k], t1 = (c.hi[k] - c.o[k]) * c.inv[k];
		near[k] = std::fmin(t0, t1);
		far[k] = std::fmax(t0, t1);
	}
	const float t_near = std::fmax(std::fmax(near[0], near[1]), std::fmax(near[2], TINY));
	const float t_far = std::fmin(std::fmin(far[0], far[1]), std::fmin(far[2], c.below));
	return t_near <= t_far;
}

void print_case(const char *what, const Case &c) {
	std::printf("%s: lo %a %a %a hi %a %a %a o %a %a %a inv %a %a %a below %a\n", what, c.lo[0], c.lo[1], c.lo[2], c.hi[0], c.hi[1],
	            c.hi[2], c.o[0], c.o[1], c.o[2], c.inv[0], c.inv[1], c.inv[2], c.below);
}

struct Tally {
	long disagreements = 0, passed = 0, flat[4] = { 0, 0, 0, 0 }, on_plane = 0, end_low = 0, end_high = 0;
};

// `cases` triples from the generator seeded with `seed`
void sweep(uint64_t seed, long cases, bool infinite, Tally &tally) {
	const float LIMIT = 1.0e30f;  // RECIPROCAL_LIMIT
	const float COORD = 1.0e6f;
	std::mt19937_64 rng(seed);
	std::uniform_real_distribution<float> unit(-1.0f, 1.0f);
	auto pick = [&](int n) { return (int) (rng() % (uint64_t) n); };
	auto clampc = [&](float v) { return std::fmin(std::fmax(v, -COORD), COORD); };
	long disagreements = 0, passed = 0, flat[4] = { 0, 0, 0, 0 }, on_plane = 0, end_low = 0, end_high = 0;
	for (long n = 0; n < cases; ++n) {
		Case c;
		// scene extents 1/16 ... 1e6
		const float extent = std::fmin(std::ldexp(1.0f, pick(25) - 4), COORD);
		// how many axes of the box are flat: forced for a share of the cases, by chance for the rest
		const int forced_flat = (n & 15) < 4 ? (int) (n & 3) : -1;
		int flat_axes = 0;
		// the ray aims at the box on most cases, so that near and far are close calls and both answers occur
		const float t_aim = std::fabs(unit(rng)) * extent;
		for (int k = 0; k < 3; ++k) {
			const float centre = unit(rng) * extent;
			const float half = std::fabs(unit(rng)) * extent * std::ldexp(1.0f, -pick(12));
			c.lo[k] = clampc(centre - half);
			c.hi[k] = clampc(centre + half);
			const bool flat_here = forced_flat >= 0 ? k < forced_flat : pick(8) == 0;
			if (flat_here)
				c.hi[k] = c.lo[k];
			flat_axes += c.lo[k] == c.hi[k] ? 1 : 0;
			// the reciprocal, straight: magnitude log-uniform over [0.5, 1e30] or one of the ends, either sign
			float magnitude;
			switch (pick(16)) {
			case 0: magnitude = 0.5f; ++end_low; break;
			case 1: magnitude = LIMIT; ++end_high; break;
			case 2: magnitude = std::nextafter(0.5f, INF); break;
			case 3: magnitude = std::nextafter(LIMIT, 0.0f); break;
			case 4: magnitude = 0x1.0p+99f; break;                                   // the end of the tame range
			case 5: case 6: magnitude = std::exp2(-1.0f + 100.7f * std::fabs(unit(rng))); break;  // up to ~1e30
			default: magnitude = 1.0f / std::fmax(std::fabs(unit(rng)), 0x1.0p-20f); break;        // a unit vector's component
			}
			magnitude = std::fmin(std::fmax(magnitude, 0.5f), LIMIT);
			c.inv[k] = (rng() & 1) ? magnitude : -magnitude;
			if (infinite && pick(2) == 0)
				c.inv[k] = (rng() & 1) ? INF : -INF;
			// the origin: where a point of the box is reached at t_aim, or in / near / on the slab, or anywhere
			const float target = c.lo[k] + (c.hi[k] - c.lo[k]) * std::fabs(unit(rng));
			c.o[k] = target - t_aim / c.inv[k];
			if (!(std::fabs(c.o[k]) <= COORD))
				c.o[k] = centre + unit(rng) * half * 1.5f;
			switch (pick(16)) {
			case 0: c.o[k] = c.lo[k]; ++on_plane; break;
			case 1: c.o[k] = c.hi[k]; ++on_plane; break;
			case 2: c.o[k] = std::nextafter(c.lo[k], -INF); break;
			case 3: c.o[k] = std::nextafter(c.hi[k], INF); break;
			case 4: c.o[k] = std::nextafter(c.lo[k], INF); break;
			case 5: c.o[k] = std::nextafter(c.hi[k], -INF); break;
			case 6: c.o[k] = centre + unit(rng) * half * 1.5f; break;
			case 7: c.o[k] = unit(rng) * extent; break;
			case 8: c.o[k] = (rng() & 1) ? COORD : -COORD; break;
			default: break;
			}
			c.o[k] = clampc(c.o[k]);
		}
		++flat[flat_axes];
		// `below`: the smallest denormal ... 1e5, and the values the product uses (just under a max_distance)
		switch (pick(12)) {
		case 0: c.below = TINY; break;
		case 1: c.below = 2.0f * TINY; break;
		case 2: c.below = std::numeric_limits<float>::min(); break;
		case 3: c.below = 1.0e5f; break;
		case 4: c.below = std::nextafter(0.2f, 0.0f); break;
		case 5: c.below = std::nextafter(100000.0f, 0.0f); break;
		case 6: c.below = std::nextafter(t_aim, (rng() & 1) ? INF : 0.0f); break;
		case 7: c.below = std::fmax(t_aim * 2.0f, TINY); break;
		default: c.below = std::exp2(-149.0f + 165.6f * std::fabs(unit(rng))); break;  // 2^-149 ... ~1e5
		}
		c.below = std::fmin(std::fmax(c.below, TINY), 1.0e5f);
		const bool a = gate_select(c), b = gate_minmax(c);
		passed += a ? 1 : 0;
		if (a != b && ++disagreements <= 10 && !infinite)
			print_case(a ? "select passes, min/max fails" : "select fails, min/max passes", c);
	}
	tally.disagreements = disagreements;
	tally.passed = passed;
	tally.on_plane = on_plane;
	tally.end_low = end_low;
	tally.end_high = end_high;
	std::memcpy(tally.flat, flat, sizeof flat);
}

}  // namespace

int main(int argc, char **argv) {
	const long cases = argc > 1 ? std::atol(argv[1]) : 20000000L;
	const bool infinite = argc > 2 && std::atoi(argv[2]) != 0;  // self-check: outside the domain the forms MUST differ
	// the sweep in eight parts, each with a generator of its own (the same triples whatever the machine), on up to eight threads
	const int parts = 8;
	std::vector<Tally> tallies(parts);
	std::vector<std::thread> threads;
	for (int p = 0; p < parts; ++p)
		threads.emplace_back(sweep, 20261018ull + (uint64_t) p, cases / parts + (p < cases % parts ? 1 : 0), infinite, std::ref(tallies[p]));
	for (std::thread &t : threads)
		t.join();
	long disagreements = 0, passed = 0, flat[4] = { 0, 0, 0, 0 }, on_plane = 0, end_low = 0, end_high = 0;
	for (const Tally &t : tallies) {
		disagreements += t.disagreements;
		passed += t.passed;
		on_plane += t.on_plane;
		end_low += t.end_low;
		end_high += t.end_high;
		for (int k = 0; k < 4; ++k)
			flat[k] += t.flat[k];
	}
	std::printf("%ld triples, %ld pass the select form, %ld disagreements; boxes flat on 0/1/2/3 axes: %ld %ld %ld %ld; origins on a "
	            "plane: %ld; reciprocals at 0.5: %ld, at 1e30: %ld\n",
	            cases, passed, disagreements, flat[0], flat[1], flat[2], flat[3], on_plane, end_low, end_high);
	if (infinite)
		return disagreements > 0 ? 0 : 1;
	const bool covered = passed > cases / 50 && cases - passed > cases / 50 && flat[1] > cases / 100 && flat[2] > cases / 100 &&
	                     flat[3] > cases / 100 && on_plane > cases / 100 && end_low > cases / 100 && end_high > cases / 100;
	if (!covered)
		std::printf("the generator does not cover its domain\n");
	return disagreements == 0 && covered ? 0 : 1;
}
