// nearest_margin_check.cc -- the pruning bound of the closest-point queries (csrc/nearest_point.h, np_limit2), swept, and a
// host-side walk built on it against brute force.  A stand-alone host program (tests/test_nearest_cpu.py compiles it, with
// the sanitizers, and runs it); it compiles the same nearest_point.h as the kernel and the C oracle.
//
// 1. The sweep.  Over random and adversarial (point, triangle, enclosing box) triples -- slivers, needles, coordinates from
//    1e-3 to 1e4, boxes tight and loose, points on, near and far from the triangle -- the predicate must never pass by a box
//    whose triangle's float32 d2 is <= the bound: with the bound at that very d2 (a tie), one ulp above it, and with the
//    radius at that triangle's float32 distance.  `magnitude` is the box's and the point's own, the tightest the kernel
//    could use (it uses the root box's, which is no smaller).
// 2. The walk.  For every scene file given (header: nodes, leaves, vertices; then the skips, the boxes as float4 pairs, the
//    leaf-ordered faces, the vertices as float4): each point descends into the nearer child for a starting bound and then
//    walks the skip-pointer order with np_prune, as kernels/nearest.hip.h does lane by lane; (d2, leaf, s, t, p) must equal
//    the brute-force minimum bit for bit, for radii inf, 0.3, 0.02, 0.
// Prints "violations N" and "walk mismatches N"; exit code 0 = both 0.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../opencl_raytracer_amd/csrc/nearest_point.h"

namespace {

struct Box {
	float lo[3], hi[3];
};

np_tri make_tri(const float a[3], const float b[3], const float c[3]) {
	np_tri t;
	t.tax = a[0]; t.tay = a[1]; t.taz = a[2];
	t.ux = b[0] - a[0]; t.uy = b[1] - a[1]; t.uz = b[2] - a[2];
	t.vx = c[0] - a[0]; t.vy = c[1] - a[1]; t.vz = c[2] - a[2];
	t.uu = np_dot(t.ux, t.uy, t.uz, t.ux, t.uy, t.uz);
	t.uv = np_dot(t.ux, t.uy, t.uz, t.vx, t.vy, t.vz);
	t.vv = np_dot(t.vx, t.vy, t.vz, t.vx, t.vy, t.vz);
	t.D = t.uv * t.uv - t.uu * t.vv;
	return t;
}

uint64_t g_triples = 0, g_violations = 0, g_nan = 0;

void check_triple(const float a[3], const float b[3], const float c[3], const Box &box, const float q[3]) {
	const np_point r = np_nearest(make_tri(a, b, c), q[0], q[1], q[2]);
	++g_triples;
	if (!(r.d2 >= 0.0f) || !(r.d2 < INFINITY)) {  // finite input must give a number
		if (g_nan++ < 5)
			std::printf("no number: d2 %g for q (%g %g %g)\n", r.d2, q[0], q[1], q[2]);
		return;
	}
	const float bd2 = np_box_d2(box.lo[0], box.lo[1], box.lo[2], box.hi[0], box.hi[1], box.hi[2], q[0], q[1], q[2]);
	const float m = np_magnitude(box.lo[0], box.lo[1], box.lo[2], box.hi[0], box.hi[1], box.hi[2], q[0], q[1], q[2]);
	const bool tie = np_prune(bd2, np_limit2(r.d2, m));
	const bool above = np_prune(bd2, np_limit2(std::nextafterf(r.d2, INFINITY), m));
	const bool radius = np_prune(bd2, np_limit2_of_distance(sqrtf(r.d2), m));
	if (tie || above || radius) {
		if (g_violations++ < 10)
			std::printf("violation: box d2 %.9g, triangle d2 %.9g, magnitude %g (tie %d, above %d, radius %d)\n", bd2, r.d2, m, tie, above, radius);
	}
}

void sweep() {
	std::mt19937_64 rng(12345);
	std::uniform_real_distribution<float> unit(-1.0f, 1.0f), zero_one(0.0f, 1.0f);
	const float scales[] = { 1e-3f, 1e-2f, 1.0f, 37.0f, 1e3f, 1e4f };
	for (int round = 0; round < 60000; ++round) {
		const float scale = scales[round % 6];
		const float offset = (round / 6) % 3 == 0 ? 0.0f : scale * unit(rng) * ((round / 18) % 2 ? 1.0f : 100.0f);
		float a[3], b[3], c[3];
		for (int k = 0; k < 3; ++k) {
			a[k] = offset + scale * unit(rng);
			b[k] = offset + scale * unit(rng);
			c[k] = offset + scale * unit(rng);
		}
		const int kind = (round / 36) % 6;
		if (kind == 1)  // a sliver: c almost on ab
			for (int k = 0; k < 3; ++k)
				c[k] = a[k] + (b[k] - a[k]) * 0.37f + scale * 1e-6f * unit(rng);
		if (kind == 2)  // a needle: b next to a
			for (int k = 0; k < 3; ++k)
				b[k] = a[k] + scale * 1e-5f * unit(rng);
		if (kind == 3)  // collinear up to rounding
			for (int k = 0; k < 3; ++k)
				c[k] = a[k] + (b[k] - a[k]) * 2.5f;
		if (kind == 4)  // two vertices coincide
			for (int k = 0; k < 3; ++k)
				c[k] = b[k];
		if (kind == 5)  // axis-aligned: the box's faces touch the triangle everywhere
			a[2] = b[2] = c[2];
		Box tight;
		for (int k = 0; k < 3; ++k) {
			tight.lo[k] = fminf(a[k], fminf(b[k], c[k]));
			tight.hi[k] = fmaxf(a[k], fmaxf(b[k], c[k]));
		}
		Box loose = tight;
		for (int k = 0; k < 3; ++k) {
			loose.lo[k] -= scale * zero_one(rng);
			loose.hi[k] += scale * zero_one(rng);
		}
		// points: on the triangle (vertices, edge and face points as float32 combinations), near it, far from it
		const float s = zero_one(rng), t = zero_one(rng) * (1.0f - s);
		float on[5][3];
		for (int k = 0; k < 3; ++k) {
			on[0][k] = a[k];
			on[1][k] = b[k];
			on[2][k] = c[k];
			on[3][k] = a[k] + (b[k] - a[k]) * s;
			on[4][k] = a[k] + ((b[k] - a[k]) * s + (c[k] - a[k]) * t);
		}
		const float reach[] = { 0.0f, 1e-7f, 1e-5f, 1e-3f, 0.1f, 1.0f, 10.0f, 1e3f };
		for (const auto &p : on)
			for (float d : reach) {
				float q[3];
				for (int k = 0; k < 3; ++k)
					q[k] = p[k] + (fabsf(offset) + scale) * d * unit(rng);
				check_triple(a, b, c, tight, q);
				check_triple(a, b, c, loose, q);
			}
	}
}

// ---- the walk -----------------------------------------------------------------------------------------------------------
struct Scene {
	std::vector<uint32_t> skips, leaf_of_node, faces;
	std::vector<float> boxes, vertices;  // float4 pairs; float4
	uint32_t nodes = 0, leaves = 0;
	np_tri leaf(uint32_t l) const { return make_tri(&vertices[4 * faces[3 * l]], &vertices[4 * faces[3 * l + 1]], &vertices[4 * faces[3 * l + 2]]); }
	float box_d2(uint32_t i, const float q[3]) const {
		const float *lo = &boxes[8 * i], *hi = lo + 4;
		return np_box_d2(lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], q[0], q[1], q[2]);
	}
};

bool load(const char *path, Scene &s) {
	std::FILE *f = std::fopen(path, "rb");
	if (!f)
		return false;
	uint32_t head[3];
	bool ok = std::fread(head, 4, 3, f) == 3;
	if (ok) {
		s.nodes = head[0];
		s.leaves = head[1];
		s.skips.resize(head[0]);
		s.boxes.resize(8 * (size_t) head[0]);
		s.faces.resize(3 * (size_t) head[1]);
		s.vertices.resize(4 * (size_t) head[2]);
		ok = std::fread(s.skips.data(), 4, s.skips.size(), f) == s.skips.size() && std::fread(s.boxes.data(), 4, s.boxes.size(), f) == s.boxes.size() &&
		     std::fread(s.faces.data(), 4, s.faces.size(), f) == s.faces.size() &&
		     std::fread(s.vertices.data(), 4, s.vertices.size(), f) == s.vertices.size();
	}
	std::fclose(f);
	s.leaf_of_node.assign(s.nodes, 0xFFFFFFFFu);
	uint32_t next = 0;
	for (uint32_t i = 0; ok && i < s.nodes; ++i) {
		if (s.skips[i] == 0 || i + s.skips[i] > s.nodes)
			ok = false;
		else if (s.skips[i] == 1)
			s.leaf_of_node[i] = next++;
	}
	for (uint32_t id : s.faces)
		ok = ok && id < s.vertices.size() / 4;
	return ok && next == s.leaves;
}

struct Record {
	float d2 = INFINITY;
	uint32_t leaf = 0xFFFFFFFFu;
	np_point p = { 0, 0, 0, 0, 0, 0 };
	uint64_t tests = 0;
	void take(const Scene &s, uint32_t l, const float q[3]) {
		const np_point r = np_nearest(s.leaf(l), q[0], q[1], q[2]);
		++tests;
		if (np_better(r.d2, l, d2, leaf)) {
			d2 = r.d2;
			leaf = l;
			p = r;
		}
	}
};

Record brute(const Scene &s, const float q[3]) {
	Record best;
	for (uint32_t l = 0; l < s.leaves; ++l)
		best.take(s, l, q);
	return best;
}

Record walk(const Scene &s, const float q[3], float max_distance) {
	Record best;
	const float *lo = &s.boxes[0], *hi = lo + 4;
	const float m = np_magnitude(lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], q[0], q[1], q[2]);
	const float radius2 = np_limit2_of_distance(max_distance, m);
	// the descent
	uint32_t at = 0;
	while (s.skips[at] != 1) {
		const uint32_t end = at + s.skips[at];
		uint32_t pick = 0xFFFFFFFFu;
		float pick_d2 = 0.0f;
		for (uint32_t c = at + 1; c < end; c += s.skips[c]) {
			const float d2 = s.box_d2(c, q);
			if (pick == 0xFFFFFFFFu || d2 < pick_d2) {
				pick = c;
				pick_d2 = d2;
			}
		}
		at = pick;
	}
	best.take(s, s.leaf_of_node[at], q);
	float limit2 = fminf(radius2, np_limit2(best.d2, m));
	// the fixed order
	for (uint32_t i = 0; i < s.nodes;) {
		if (np_prune(s.box_d2(i, q), limit2)) {
			i += s.skips[i];
			continue;
		}
		if (s.skips[i] == 1) {
			best.take(s, s.leaf_of_node[i], q);
			limit2 = fminf(radius2, np_limit2(best.d2, m));
		}
		++i;
	}
	return best;
}

uint64_t g_walks = 0, g_mismatches = 0, g_walk_tests = 0, g_brute_tests = 0;

void walk_scene(const Scene &s, const char *name) {
	std::mt19937_64 rng(777);
	std::uniform_real_distribution<float> unit(-1.0f, 1.0f);
	const float *lo = &s.boxes[0], *hi = lo + 4;
	std::vector<float> points;
	for (int i = 0; i < 600; ++i) {
		const float reach = i < 400 ? 0.75f : (i < 500 ? 3.0f : 1500.0f);  // in the box x 1.5, a few box sizes out, 1e3 out
		for (int k = 0; k < 3; ++k) {
			const float extent = hi[k] - lo[k] > 0.0f ? hi[k] - lo[k] : 1.0f;
			points.push_back((lo[k] + hi[k]) * 0.5f + extent * reach * unit(rng));
		}
	}
	for (uint32_t v = 0; v < s.vertices.size() / 4 && v < 200; ++v)  // on the surface: the vertices themselves
		for (int k = 0; k < 3; ++k)
			points.push_back(s.vertices[4 * v + k]);
	const float radii[] = { INFINITY, 0.3f, 0.02f, 0.0f };
	for (size_t i = 0; i + 2 < points.size(); i += 3) {
		const float *q = &points[i];
		const Record want = brute(s, q);
		g_brute_tests += want.tests;
		for (float radius : radii) {
			const Record got = walk(s, q, radius);
			++g_walks;
			g_walk_tests += got.tests;
			// within the radius the record is brute force's, bit for bit; beyond it both sides say "not found"
			const bool found = want.d2 < INFINITY && sqrtf(want.d2) <= radius;
			const bool got_found = got.d2 < INFINITY && sqrtf(got.d2) <= radius;
			const bool same = found ? (got_found && got.leaf == want.leaf && std::memcmp(&got.p, &want.p, sizeof got.p) == 0) : !got_found;
			if (!same && g_mismatches++ < 10)
				std::printf("%s: point %zu radius %g: walk (%.9g, leaf %u), brute force (%.9g, leaf %u)\n", name, i / 3, radius, got.d2, got.leaf, want.d2, want.leaf);
		}
	}
}

}  // namespace

int main(int argc, char **argv) {
	sweep();
	std::printf("triples %" PRIu64 ", no number %" PRIu64 ", violations %" PRIu64 "\n", g_triples, g_nan, g_violations + g_nan);
	for (int i = 1; i < argc; ++i) {
		Scene s;
		if (!load(argv[i], s)) {
			std::printf("cannot read %s\n", argv[i]);
			return 2;
		}
		walk_scene(s, argv[i]);
	}
	std::printf("walks %" PRIu64 ", triangle tests per walk %.1f (brute force %.1f), walk mismatches %" PRIu64 "\n", g_walks,
	            g_walks ? (double) g_walk_tests / (double) g_walks : 0.0, g_walks ? (double) g_brute_tests * 4.0 / (double) g_walks : 0.0, g_mismatches);
	return g_violations + g_nan + g_mismatches == 0 ? 0 : 1;
}
