// prune_bound_sweep.cc -- CPU sweep (no GPU) AIMED at the bound the closest-hit walk's pruning rests on (scene_pack.h,
// leaf_growth; scene_pack.cc, make_walk_array; kernels/primary.hip.h, far_limit): every hit the reference's triangle test
// accepts must lie inside its leaf's GROWN box of the primary rays' records.  prune_check.cc and camera_margin_check.cc
// meet that bound with two meshes; this program throws triangles and rays at it that are made to strain it.
//
//   prune_bound_sweep sweep <triangles> [factor]
//       Generated triangles (edge lengths 1e-3 .. 1e4, edge ratios up to 1e4, apex angles down to 3e-4, coordinates up to
//       1e6, eta -- leaf_growth's measure of how fuzzy Cramer's rule makes the accepted region -- from its least value up to
//       the 1/32 gate and beyond, axis-aligned and oblique planes, either vertex order, triangles a few ulps of their
//       coordinates in size), packed by pack_scene (the float n, uu, uv, vv, D are the product's), grown by leaf_growth as
//       make_walk_array grows them, padded by padded_bound as make_walk_array pads them, prune_margin formed the same way --
//       and every so often compared, bit for bit, with what make_walk_array itself makes of the one triangle.  Eyes: the
//       reference's camera, random eyes within 2e6 + 4, eyes in the triangle's plane up to a height of 1e-6 of the distance
//       (|n.d| dominated by rounding) and a little above, eyes from which the ray is nearly parallel to a face of the leaf's
//       box.  Rays: at points 0.5 .. 1.5 x 1e-5 (parametric) outside each edge and corner, up to 2 eta outside, inside; on
//       a share of them a local search nudges the direction by ulps, a fixed number of steps, towards the largest
//       needed / granted growth.  Per accepted hit whose leaf's own box the ray meets (the reference tests no other):
//         1. the kernel's node test on the grown, padded record passes;
//         2. the REAL point of the ray at the accepted distance lies inside the grown box on every axis, and the float hit
//            point inside the record;
//         3. the record's near value as the kernel forms it is <= d * 1.00001f + prune_margin.
//       `factor` multiplies every finite growth (what OCRT_PRUNE_GROWTH does in the A/B build).  Exit code, no factor or 1:
//       0 = no violation, every worst ratio below 1 and the run was large enough to mean something.  factor 0: the self-
//       check -- 0 if the run REPORTS violations, 1 if the sweep has no teeth.  Any other factor: reports, exit 0.
//   prune_bound_sweep trees
//       Whole trees of 200 .. 2000 faces through BVH, pack_scene and make_walk_array(scene, d, true, eye), faces with eta in
//       [1/64, 1/32), in [1/32, 1/8] and ordinary ones mixed: prune_check.cc's structure checks, the faces without a bound
//       in the unpruned head and nowhere else, and the three conditions above up the whole chain of boxes over a hit.
//   prune_bound_sweep facts <scene.off> <rays.f32> <out.txt>
//       For tests/prune_traps.py: the stream walk array's facts for the eye the rays start at, leaf_growth per leaf, and per
//       ray the reference's accepted hits, the winner and whether the pixel is a TRAP (see prune_traps.py).
//   prune_bound_sweep model <scene.off> <rays.f32>
//       A sequential model of the pruning walk (kernels/primary.hip.h: a lane enters a record if the kernel's node test
//       passes with its far_limit, tests a leaf as the reference does, lowers far_limit outside the unpruned head) on the
//       stream walk array: how many rays end with another leaf than the reference's minimum of (distance, leaf).  Linked
//       against the A/B build of the library it honours OCRT_PRUNE_GROWTH: 0 rays with the growth, some without.
// Totals do not depend on the number of threads: 16 seeded streams, each its own share of the triangles.
#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "bvh.h"
#include "mesh.h"
#include "reference_tests.h"
#include "scene_pack.h"

using namespace ocrt;
using namespace reference_tests;

namespace {

const float INF = std::numeric_limits<float>::infinity();
const double DINF = std::numeric_limits<double>::infinity();
const int STREAMS = 16;
const int DECADES = 5;  // eta in [1e-6, 1e-5) ... [1e-2, 1e-1)

struct Rng {
	std::mt19937_64 g;
	explicit Rng(uint64_t seed) : g(seed) {}
	double u() { return (double) (g() >> 11) * (1.0 / 9007199254740992.0); }
	double range(double a, double b) { return a + (b - a) * u(); }
	double log_range(double a, double b) { return std::exp(range(std::log(a), std::log(b))); }
	double sign() { return (g() & 1) ? 1.0 : -1.0; }
	unsigned below(unsigned n) { return (unsigned) (g() % n); }
	void unit(double v[3]) {
		for (;;) {
			double s = 0;
			for (int k = 0; k < 3; ++k) {
				v[k] = range(-1, 1);
				s += v[k] * v[k];
			}
			if (s > 1e-4 && s <= 1.0) {
				s = std::sqrt(s);
				for (int k = 0; k < 3; ++k)
					v[k] /= s;
				return;
			}
		}
	}
};

// eta as leaf_growth forms it: for the tally by decade only (the growth itself is leaf_growth's)
double eta_of(const TriRec &t) {
	const double uu = t.uu, vv = t.vv, area2 = std::fabs((double) t.D);
	const double lu = std::sqrt(uu), lv = std::sqrt(vv);
	const double k = area2 > 0.0 ? uu * vv / area2 : DINF;
	const double r = lu > lv ? lu / lv : lv / lu;
	return 128.0 * std::ldexp(1.0, -24) * k * r;
}

// One leaf as make_walk_array makes it for a scene of this one triangle and this eye: the own box grown by leaf_growth
// (x factor), the grown box padded, prune_margin.
struct Leaf {
	bool bounded = false;      // leaf_growth finite: the face gets a box that promises something
	float growth = 0.0f;       // as applied (a float, rounded up)
	NodeRec grown{}, record{};  // the grown box; the grown, padded box (what the kernel tests)
	float margin = INF, origin_limit = 0.0f;
	bool covered = false;      // the eye is one the fast walk covers
};
Leaf make_leaf(const TriRec &t, const float eye[3], double factor) {
	Leaf out;
	float extent = 0.0f;
	for (int k = 0; k < 3; ++k)
		extent = std::fmax(extent, std::fmax(std::fabs(t.lo[k]), std::fabs(t.hi[k])));
	if (!(extent <= 1.0e6f))
		return out;
	const double reach = 2.0 * (double) extent;
	out.origin_limit = 2.0f * extent + 4.0f;
	float eye_reach = 0.0f;
	for (int k = 0; k < 3; ++k)
		eye_reach = std::fmax(eye_reach, std::fabs(eye[k]));
	out.covered = eye_reach <= out.origin_limit;
	if (!out.covered && eye_reach <= 2.0e6f + 4.0f) {
		out.origin_limit = eye_reach;
		out.covered = true;
	}
	if (!out.covered)
		return out;
	const double eye_distance = std::sqrt((double) eye[0] * eye[0] + (double) eye[1] * eye[1] + (double) eye[2] * eye[2]);
	double g = leaf_growth(t, eye_distance);
	if (!(g < 1e30))
		return out;
	g *= factor;
	out.bounded = true;
	out.growth = std::nextafterf((float) g, INF);
	const double grow = out.growth;
	double largest = eye_distance;
	for (int k = 0; k < 3; ++k) {
		out.grown.lo[k] = std::nextafterf((float) ((double) t.lo[k] - grow), -INF);
		out.grown.hi[k] = std::nextafterf((float) ((double) t.hi[k] + grow), INF);
		largest = std::fmax(largest, std::fmax(std::fabs((double) out.grown.lo[k]), std::fabs((double) out.grown.hi[k])));
	}
	out.margin = (float) (1e-5 * largest) + 1e-30f;
	out.record = out.grown;
	for (int k = 0; k < 3; ++k) {
		const double box = std::fmax(std::fabs((double) out.grown.lo[k]), std::fabs((double) out.grown.hi[k]));
		const double origin = std::fmin((double) out.origin_limit, std::fmax(std::fabs((double) eye[k]), box + reach));
		out.record.lo[k] = padded_bound(out.grown.lo[k], (float) origin, false, 0.0f);
		out.record.hi[k] = padded_bound(out.grown.hi[k], (float) origin, true, 0.0f);
	}
	return out;
}

struct Tally {
	unsigned long long triangles = 0, unbounded = 0, uncovered = 0, rays = 0, exact_form = 0, accepted = 0, outside_own_box = 0;
	unsigned long long hits[DECADES] = {}, in_front[DECADES] = {};
	double worst[DECADES] = {};
	unsigned long long missed_box = 0, outside_real = 0, outside_float = 0, pruned = 0, compared = 0, differs = 0;
	double worst_case[12] = {};  // the ray and triangle of the worst ratio seen (for the report)
	double worst_any = 0.0;
	unsigned long long violations() const { return missed_box + outside_real + outside_float + pruned; }
	void add(const Tally &o) {
		triangles += o.triangles; unbounded += o.unbounded; uncovered += o.uncovered; rays += o.rays; exact_form += o.exact_form;
		accepted += o.accepted; outside_own_box += o.outside_own_box;
		for (int k = 0; k < DECADES; ++k) {
			hits[k] += o.hits[k];
			in_front[k] += o.in_front[k];
			worst[k] = std::fmax(worst[k], o.worst[k]);
		}
		missed_box += o.missed_box; outside_real += o.outside_real; outside_float += o.outside_float; pruned += o.pruned;
		compared += o.compared; differs += o.differs;
		if (o.worst_any > worst_any) {
			worst_any = o.worst_any;
			std::memcpy(worst_case, o.worst_case, sizeof worst_case);
		}
	}
};

int decade_of(double eta) {
	if (!(eta >= 1e-6))
		return 0;
	const int k = (int) std::floor(std::log10(eta)) + 6;
	return k < 0 ? 0 : k >= DECADES ? DECADES - 1 : k;
}

// One ray against one leaf: the three conditions; returns needed / granted growth (-1: nothing to hold).
double cast(const TriRec &t, const Leaf &leaf, int decade, const float o[3], const float d[3], Tally &tally) {
	++tally.rays;
	const Accepted h = reference_triangle(t, o, d);
	if (!h.ok || !(h.distance < INF))
		return -1.0;
	++tally.accepted;
	if (!reference_slab(t.lo, t.hi, o, d, 100000.0f)) {  // (the reference tests a triangle only if the ray meets its leaf's own box)
		++tally.outside_own_box;
		return -1.0;
	}
	++tally.hits[decade];
	double own_near = 0.0;
	if (!box_near(t.lo, t.hi, o, d, &own_near) || own_near > (double) h.distance)
		++tally.in_front[decade];  // the hit lies in front of the leaf's OWN box: the case the growth is for
	// 2. the real point of the ray at the accepted distance; the float hit point
	double needed = 0.0;
	bool inside_real = true, inside_float = true;
	for (int k = 0; k < 3; ++k) {
		const double p = (double) o[k] + (double) d[k] * (double) h.distance;
		needed = std::fmax(needed, std::fmax((double) t.lo[k] - p, p - (double) t.hi[k]));
		inside_real = inside_real && p >= (double) leaf.grown.lo[k] && p <= (double) leaf.grown.hi[k];
		inside_float = inside_float && h.ip[k] >= leaf.record.lo[k] && h.ip[k] <= leaf.record.hi[k];
	}
	tally.outside_real += !inside_real;
	tally.outside_float += !inside_float;
	const double ratio = needed <= 0.0 ? 0.0 : needed / (double) leaf.growth;
	if (ratio > tally.worst[decade])
		tally.worst[decade] = ratio;
	if (ratio > tally.worst_any) {
		tally.worst_any = ratio;
		const double c[12] = { o[0], o[1], o[2], d[0], d[1], d[2], t.ta[0], t.ta[1], t.ta[2], needed, leaf.growth, h.distance };
		std::memcpy(tally.worst_case, c, sizeof c);
	}
	// 1. and 3.: the kernel's own test on the record (packets of rays it does not select take the exact form of the walk)
	if (!selectable(o, d, leaf.origin_limit)) {
		++tally.exact_form;
		return ratio;
	}
	const KernelRay kr = kernel_ray(o, d);
	float far;
	const float near = kernel_near(leaf.record, kr, &far);
	if (!(near <= std::fmin(far, std::nextafterf(100000.0f, 0.0f))))
		++tally.missed_box;
	else if (near > h.distance * 1.00001f + leaf.margin)
		++tally.pruned;
	return ratio;
}

void normalise_to_float(const double w[3], float d[3]) {
	const double l = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
	for (int k = 0; k < 3; ++k)
		d[k] = (float) (w[k] / l);
}

// A point of the triangle's plane in its own parameters: outside an edge or a corner by `x` (and `y`), or inside.
void target_parameters(Rng &rng, double eta, double *s, double *q) {
	const unsigned kind = rng.below(16);
	double x = rng.range(0.5e-5, 1.5e-5), y = rng.range(0.5e-5, 1.5e-5);
	if (kind >= 10 && kind < 14) {  // up to 2 eta outside
		x = rng.u() * 2.0 * eta;
		y = rng.u() * 2.0 * eta;
	}
	if (kind >= 14) {  // inside
		*s = rng.u();
		*q = (1.0 - *s) * rng.u();
		return;
	}
	const double w = rng.u();
	switch (kind % 6) {
	case 0: *s = -x; *q = w; break;                                // outside the edge along v
	case 1: *s = w; *q = -x; break;                                // outside the edge along u
	case 2: *s = w * (1.0 + x); *q = (1.0 - w) * (1.0 + x); break;  // outside the third edge
	case 3: *s = -x; *q = -y; break;                               // outside the corner a
	case 4: *s = 1.0 + x + y; *q = -y; break;                      // outside the corner b
	default: *s = -y; *q = 1.0 + x + y; break;                     // outside the corner c
	}
}

// A triangle of these edge lengths and this apex angle at `place` from the origin, in a random frame, as float vertices.
void lay_triangle(Rng &rng, double longer, double shorter, double theta, double place, float v[3][3]) {
	// the frame: axis-aligned (a signed permutation) or oblique
	double e0[3], e1[3];
	if (rng.below(3) == 0) {
		const unsigned a = rng.below(3), b = (a + 1 + rng.below(2)) % 3;
		for (int k = 0; k < 3; ++k)
			e0[k] = e1[k] = 0.0;
		e0[a] = rng.sign();
		e1[b] = rng.sign();
	} else {
		double n[3];
		rng.unit(e0);
		do {
			rng.unit(n);
			e1[0] = e0[1] * n[2] - e0[2] * n[1];
			e1[1] = e0[2] * n[0] - e0[0] * n[2];
			e1[2] = e0[0] * n[1] - e0[1] * n[0];
		} while (e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2] < 0.01);
		const double l = std::sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
		for (int k = 0; k < 3; ++k)
			e1[k] /= l;
	}
	const bool u_is_longer = rng.below(2) != 0;
	const double lu = u_is_longer ? longer : shorter, lv = u_is_longer ? shorter : longer;
	double at[3], dir[3];
	rng.unit(dir);
	if (rng.below(4) == 0)  // (the whole offset on one axis)
		for (int k = 1; k < 3; ++k)
			dir[k] = 0.0;
	for (int k = 0; k < 3; ++k)
		at[k] = place * dir[k];
	double p[3][3];
	for (int k = 0; k < 3; ++k) {
		p[0][k] = at[k];
		p[1][k] = at[k] + lu * e0[k];
		p[2][k] = at[k] + lv * (std::cos(theta) * e0[k] + std::sin(theta) * e1[k]);
	}
	const bool swap = rng.below(2) != 0;  // either vertex order
	for (int k = 0; k < 3; ++k) {
		v[0][k] = (float) std::fmax(-1e6, std::fmin(1e6, p[0][k]));
		v[swap ? 2 : 1][k] = (float) std::fmax(-1e6, std::fmin(1e6, p[1][k]));
		v[swap ? 1 : 2][k] = (float) std::fmax(-1e6, std::fmin(1e6, p[2][k]));
	}
}

// The vertices of one generated triangle of the sweep.
void make_triangle(Rng &rng, float v[3][3]) {
	const unsigned family = rng.below(20);
	double ratio, theta, shorter = rng.log_range(1e-3, 1e4), place;
	bool tiny_in_its_coordinates = false;
	if (family < 10) {  // k r log-uniform from its least value to the gate (k r = 4096 is eta = 1/32)
		const double kr = rng.log_range(1.0, 4096.0);
		ratio = std::exp(rng.u() * std::log(kr));
		theta = std::asin(std::fmin(1.0, 1.0 / std::sqrt(kr / ratio)));
	} else if (family < 13) {  // up to the gate from below, and just across
		const double kr = 4096.0 * (rng.below(4) ? 1.0 - rng.log_range(1e-7, 0.5) : 1.0 + rng.log_range(1e-7, 1e-2));
		ratio = std::exp(rng.u() * std::log(kr));
		theta = std::asin(std::fmin(1.0, 1.0 / std::sqrt(kr / ratio)));
	} else if (family < 17) {  // the extremes: mostly faces without a bound
		ratio = rng.log_range(1.0, 1e4);
		theta = rng.log_range(3e-4, 1.5707);
	} else {  // a few ulps of its coordinates in size: u, v and with them D are what the rounding of the vertices left
		ratio = rng.log_range(1.0, 8.0);
		theta = rng.log_range(0.05, 1.5707);
		tiny_in_its_coordinates = true;
	}
	if (rng.below(8) == 0)
		theta = 3.14159265358979 - theta;  // (an obtuse apex: the same sine)
	if (shorter * ratio > 1e4)
		shorter = 1e4 / ratio;
	const double longer = shorter * ratio;
	if (tiny_in_its_coordinates)
		place = std::fmin(1e6, longer * rng.log_range(2e4, 4e6));
	else if (family >= 10 && family < 13)
		place = longer * rng.log_range(1e-3, 16.0);  // (the shape survives the rounding: eta stays where it was aimed)
	else
		place = rng.below(4) ? longer * rng.log_range(1e-3, 1e4) : rng.log_range(1e-3, 1e6);
	place = std::fmin(place, 1e6 - 2.0 * longer > 0 ? 1e6 - 2.0 * longer : 0.0);
	lay_triangle(rng, longer, shorter, theta, place, v);
}

// An eye for a ray through `target` (a point of the triangle's plane).
void make_eye(Rng &rng, const TriRec &t, const double target[3], unsigned kind, float eye[3]) {
	const double size = std::sqrt(std::fmax((double) t.uu, (double) t.vv));
	double e[3] = { 0.0, 0.0, 2.0 };  // kind 0: the reference's camera
	if (kind == 1) {  // anywhere within 2e6 + 4
		double dir[3];
		rng.unit(dir);
		const double far = rng.below(4) ? size * rng.log_range(0.1, 1e3) : rng.log_range(1e-2, 2e6);
		for (int k = 0; k < 3; ++k)
			e[k] = target[k] + far * dir[k];
	} else if (kind == 2) {  // in the triangle's plane, up to a height of 1e-6 of the distance; some a little above
		const double a = rng.range(0, 6.283185307179586), far = size * rng.log_range(0.5, 1e3);
		const double lu = std::sqrt((double) t.uu), ln = std::sqrt((double) t.n[0] * t.n[0] + (double) t.n[1] * t.n[1] + (double) t.n[2] * t.n[2]);
		const double height = far * (rng.below(3) ? rng.log_range(1e-9, 1e-6) : rng.log_range(1e-6, 1e-2)) * rng.sign();
		for (int k = 0; k < 3; ++k) {
			const double uk = lu > 0 ? t.u[k] / lu : 0.0, nk = ln > 0 ? t.n[k] / ln : 0.0;
			// (u and n x u span the plane)
			const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
			const double wk = ln > 0 && lu > 0 ? ((double) t.n[k1] * t.u[k2] - (double) t.n[k2] * t.u[k1]) / (ln * lu) : 0.0;
			e[k] = target[k] + far * (std::cos(a) * uk + std::sin(a) * wk) + height * nk;
		}
	} else if (kind == 3) {  // the ray nearly parallel to a face of the leaf's box: one or two components of the direction tiny or zero
		const unsigned along = rng.below(3);
		const double far = size * rng.log_range(0.5, 1e3) * rng.sign();
		for (int k = 0; k < 3; ++k) {
			const unsigned how = rng.below(4);
			const double small = how == 0 ? 0.0 : rng.log_range(1e-9, 1e-3) * rng.sign();
			e[k] = target[k] + far * ((unsigned) k == along ? 1.0 : how == 3 ? rng.range(-1, 1) : small);
		}
	}
	for (int k = 0; k < 3; ++k)
		eye[k] = (float) std::fmax(-2.0e6, std::fmin(2.0e6, e[k]));
}

// One stream's share of the sweep.
void sweep_stream(int stream, unsigned long long triangles, double factor, Tally &tally) {
	Rng rng(0x5eed0000ull + 7919ull * (uint64_t) stream);
	const unsigned BATCH = 256;
	std::vector<Vec3f> vertices(3 * BATCH), normals(3 * BATCH);
	std::vector<uint32_t> faces(3 * BATCH), nodes;
	std::vector<Vec3f> aabbs;
	for (unsigned long long done = 0; done < triangles; done += BATCH) {
		const unsigned count = (unsigned) std::min<unsigned long long>(BATCH, triangles - done);
		// a batch of triangles as one scene: a chain of inner nodes, leaf i holds triangle i, boxes the unions of what is below
		vertices.resize(3 * count);
		normals.assign(3 * count, Vec3f{ 0.0f, 0.0f, 1.0f });
		faces.resize(3 * count);
		for (unsigned i = 0; i < count; ++i) {
			float v[3][3];
			make_triangle(rng, v);
			for (int c = 0; c < 3; ++c) {
				vertices[3 * i + c] = Vec3f{ v[c][0], v[c][1], v[c][2] };
				faces[3 * i + c] = 3 * i + c;
			}
		}
		nodes.assign(2 * count - 1, 1);
		aabbs.assign(2 * (2 * count - 1), Vec3f{ 0, 0, 0 });
		auto leaf_box = [&](unsigned i, Vec3f *lo, Vec3f *hi) {
			*lo = *hi = vertices[3 * i];
			for (int c = 1; c < 3; ++c)
				for (int k = 0; k < 3; ++k) {
					(*lo)[k] = std::fmin((*lo)[k], vertices[3 * i + c][k]);
					(*hi)[k] = std::fmax((*hi)[k], vertices[3 * i + c][k]);
				}
		};
		// pre-order: inner(0), leaf 0, inner(1), leaf 1, ..., leaf count-2, leaf count-1
		for (unsigned i = 0; i + 1 < count; ++i) {
			nodes[2 * i] = 2 * (count - i) - 1;
			leaf_box(i, &aabbs[2 * (2 * i + 1)], &aabbs[2 * (2 * i + 1) + 1]);
		}
		leaf_box(count - 1, &aabbs[2 * (2 * count - 2)], &aabbs[2 * (2 * count - 2) + 1]);
		for (unsigned i = count - 1; i-- > 0;) {  // the inner boxes, from the end of the chain
			const unsigned leaf = 2 * i + 1, rest = 2 * i + 2;
			for (int k = 0; k < 3; ++k) {
				aabbs[2 * (2 * i)][k] = std::fmin(aabbs[2 * leaf][k], aabbs[2 * rest][k]);
				aabbs[2 * (2 * i) + 1][k] = std::fmax(aabbs[2 * leaf + 1][k], aabbs[2 * rest + 1][k]);
			}
		}
		const PackedScene scene = pack_scene(faces, nodes, aabbs, vertices, normals);
		for (unsigned i = 0; i < count; ++i) {
			const TriRec &t = scene.tris[i];
			++tally.triangles;
			const double eta = eta_of(t);
			const int decade = decade_of(eta);
			// the first ray's target places the eye; every ray of the triangle starts there (one walk array has one eye)
			double s, q, target[3];
			target_parameters(rng, eta, &s, &q);
			for (int k = 0; k < 3; ++k)
				target[k] = (double) t.ta[k] + s * (double) t.u[k] + q * (double) t.v[k];
			float eye[3];
			make_eye(rng, t, target, rng.below(4), eye);
			const Leaf leaf = make_leaf(t, eye, factor);
			if (!leaf.covered) {
				++tally.uncovered;
				continue;
			}
			if (!leaf.bounded) {
				++tally.unbounded;
				continue;
			}
			if (factor == 1.0 && (tally.triangles & 63) == 0) {  // what make_walk_array itself makes of this one triangle
				PackedScene one;
				one.nodes.resize(1);
				for (int k = 0; k < 3; ++k) {
					one.nodes[0].lo[k] = t.lo[k];
					one.nodes[0].hi[k] = t.hi[k];
				}
				one.nodes[0].skip = 1;
				one.nodes[0].leaf = 0;
				one.tris.push_back(t);
				one.regular = one.nested = true;
				const WalkArray w = make_walk_array(one, 0.0f, true, eye);
				++tally.compared;
				bool same = !w.nodes.empty() && w.eye_covered && std::memcmp(&w.prune_margin, &leaf.margin, sizeof(float)) == 0 &&
				            w.origin_limit == leaf.origin_limit && w.unpruned_bytes == 0 && w.primary_bytes == sizeof(NodeRec);
				if (same)
					same = std::memcmp(w.nodes[0].lo, leaf.record.lo, 3 * sizeof(float)) == 0 && std::memcmp(w.nodes[0].hi, leaf.record.hi, 3 * sizeof(float)) == 0;
				tally.differs += !same;
			}
			const bool search = rng.below(8) == 0;
			for (int ray = 0; ray < 4; ++ray) {
				if (ray) {
					target_parameters(rng, eta, &s, &q);
					for (int k = 0; k < 3; ++k)
						target[k] = (double) t.ta[k] + s * (double) t.u[k] + q * (double) t.v[k];
				}
				const double w[3] = { target[0] - eye[0], target[1] - eye[1], target[2] - eye[2] };
				if (!(w[0] * w[0] + w[1] * w[1] + w[2] * w[2] > 0.0))
					continue;
				float d[3];
				normalise_to_float(w, d);
				double best = cast(t, leaf, decade, eye, d, tally);
				if (!search || ray != 0)
					continue;
				// a local search: the direction nudged by ulps, kept where needed / granted grows; a fixed number of steps
				for (int step = 0; step < 8; ++step) {
					float trial[3] = { d[0], d[1], d[2] };
					const unsigned axis = rng.below(3);
					const float towards = rng.below(2) ? INF : -INF;
					for (unsigned n = 1 + rng.below(2); n-- > 0;)
						trial[axis] = std::nextafterf(trial[axis], towards);
					const double length2 = (double) trial[0] * trial[0] + (double) trial[1] * trial[1] + (double) trial[2] * trial[2];
					if (std::fabs(length2 - 1.0) > 4e-7)  // (stays what normalising in float can give: a unit vector up to a few ulps)
						continue;
					const double now = cast(t, leaf, decade, eye, trial, tally);
					if (now > best) {
						best = now;
						std::memcpy(d, trial, sizeof d);
					}
				}
			}
		}
	}
}

int run_sweep(unsigned long long triangles, double factor) {
	const auto begin = std::chrono::steady_clock::now();
	std::vector<Tally> tallies(STREAMS);
	unsigned threads = std::thread::hardware_concurrency();
	threads = threads < 1 ? 1 : threads > (unsigned) STREAMS ? (unsigned) STREAMS : threads;
	std::vector<std::thread> pool;
	for (unsigned th = 0; th < threads; ++th)
		pool.emplace_back([&, th] {
			for (int s = (int) th; s < STREAMS; s += (int) threads) {
				const unsigned long long share = triangles / STREAMS + ((unsigned long long) s < triangles % STREAMS ? 1 : 0);
				sweep_stream(s, share, factor, tallies[s]);
			}
		});
	for (auto &t : pool)
		t.join();
	Tally all;
	for (const Tally &t : tallies)
		all.add(t);
	const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - begin).count();
	std::printf("prune_bound_sweep: growth factor %g: %llu triangles (%llu without a bound, %llu with an eye the fast walk does not cover), %llu rays, "
	            "%llu accepted hits (%llu of them missing the leaf's own box, %llu in packets of the exact form), %u threads, %.1f s\n",
	            factor, all.triangles, all.unbounded, all.uncovered, all.rays, all.accepted, all.outside_own_box, all.exact_form, threads, seconds);
	unsigned long long in_front = 0;
	for (int k = 0; k < DECADES; ++k) {
		std::printf("prune_bound_sweep:   eta in [1e%d, 1e%d): %llu accepted hits, %llu in front of their leaf's own box, worst needed / granted growth %.4f\n",
		            k - 6, k - 5, all.hits[k], all.in_front[k], all.worst[k]);
		in_front += all.in_front[k];
	}
	std::printf("prune_bound_sweep:   the worst: eye (%.9g, %.9g, %.9g) direction (%.9g, %.9g, %.9g) vertex a (%.9g, %.9g, %.9g): needed %.6g, granted %.6g, distance %.9g\n",
	            all.worst_case[0], all.worst_case[1], all.worst_case[2], all.worst_case[3], all.worst_case[4], all.worst_case[5], all.worst_case[6],
	            all.worst_case[7], all.worst_case[8], all.worst_case[9], all.worst_case[10], all.worst_case[11]);
	std::printf("prune_bound_sweep:   %llu leaves compared with make_walk_array's own record: %llu differ\n", all.compared, all.differs);
	std::printf("prune_bound_sweep: %llu grown boxes missed, %llu real points outside the grown box, %llu float hit points outside the record, %llu pruned wrongly: %llu violations\n",
	            all.missed_box, all.outside_real, all.outside_float, all.pruned, all.violations());
	if (factor == 0.0) {
		if (all.violations() == 0) {
			std::printf("prune_bound_sweep: without the growth the run shows no violation: the sweep has no teeth\n");
			return 1;
		}
		std::printf("prune_bound_sweep: without the growth violations are reported, as they must be\n");
		return 0;
	}
	if (factor != 1.0)
		return 0;
	int bad = 0;
	auto expect = [&](bool ok, const char *what) {
		if (!ok) {
			std::printf("FAILED: %s\n", what);
			++bad;
		}
	};
	expect(all.differs == 0 && all.compared > 0, "the leaves made here are make_walk_array's, bit for bit");
	expect(all.violations() == 0, "no accepted hit lies outside its leaf's grown box or is pruned");
	for (int k = 0; k < DECADES; ++k)
		expect(all.worst[k] < 1.0, "every worst needed / granted growth is below 1");
	// what keeps the sweep from saying nothing (the reference side alone); scaled down for a short run
	const double scale = std::fmin(1.0, (double) triangles / 5.0e6);
	for (int k = 1; k < DECADES; ++k)
		expect((double) all.hits[k] >= 100000.0 * scale, "at least 100 000 accepted hits in each eta decade from 1e-5 to 1e-2");
	expect((double) all.hits[0] >= 5000.0 * scale, "at least 5 000 accepted hits with eta below 1e-5");
	expect((double) in_front >= 50000.0 * scale, "at least 50 000 accepted hits in front of their leaf's own box");
	expect((double) all.unbounded <= 0.6 * (double) all.triangles, "no more than 60 % of the triangles are faces without a bound");
	if (triangles >= 5000000ull)
		expect(all.rays >= 20000000ull, "at least 20 M rays over at least 5 M triangles");
	if (!bad)
		std::printf("prune_bound_sweep: ok\n");
	return bad ? 1 : 0;
}

}  // namespace

int run_trees();
int run_facts(const char *off, const char *rays, const char *out);
int run_model(const char *off, const char *rays);

int main(int argc, char **argv) {
	const std::string mode = argc > 1 ? argv[1] : "";
	if (mode == "sweep" && argc >= 3)
		return run_sweep(std::strtoull(argv[2], nullptr, 10), argc > 3 ? std::atof(argv[3]) : 1.0);
	if (mode == "trees")
		return run_trees();
	if (mode == "facts" && argc >= 5)
		return run_facts(argv[2], argv[3], argv[4]);
	if (mode == "model" && argc >= 4)
		return run_model(argv[2], argv[3]);
	std::printf("usage: prune_bound_sweep sweep <triangles> [factor] | trees | facts <scene.off> <rays.f32> <out.txt> | model <scene.off> <rays.f32>\n");
	return 2;
}


namespace {

PackedScene pack(Mesh &m) {
	compute_vertex_normals(&m);
	BVH bvh(BVH::Method::CUT_LONGEST_AXIS);
	bvh.buildBVH(m);
	const auto sorted = sort_faces_by_leaf_order(m, bvh);
	return pack_scene(sorted, bvh.nodes, bvh.aabbs, m.vertices, m.vnormals);
}

// The primary rays' records of a walk array: who is whose parent, where each leaf's record is.
struct Records {
	const NodeRec *rec;
	size_t count, loose_end;
	std::vector<uint32_t> parent, record_of;
	Records(const PackedScene &scene, const WalkArray &walk)
	    : rec(walk.nodes.data()), count(walk.primary_bytes / sizeof(NodeRec)), loose_end(walk.unpruned_bytes / sizeof(NodeRec)),
	      parent(count, 0xFFFFFFFFu), record_of(scene.tris.size(), 0xFFFFFFFFu) {
		std::vector<size_t> ends;
		std::vector<uint32_t> open;
		for (size_t i = 0; i < count; ++i) {
			while (!ends.empty() && ends.back() <= i) {
				ends.pop_back();
				open.pop_back();
			}
			if (!open.empty())
				parent[i] = open.back();
			const size_t skip = rec[i].skip / sizeof(NodeRec);
			if (skip > 1) {
				ends.push_back(i + skip);
				open.push_back((uint32_t) i);
			} else if (rec[i].leaf < scene.tris.size()) {
				record_of[rec[i].leaf] = (uint32_t) i;
			}
		}
	}
	bool loose(uint32_t leaf) const { return record_of[leaf] >= 1 && record_of[leaf] < loose_end; }
};

// prune_check.cc's structure checks on one walk array: skips tile both copies, both hold every leaf once, children nearest
// to the eye first outside the unpruned head.
void check_structure(const PackedScene &scene, const WalkArray &walk, const double eye[3], bool *tiles_out, bool *same_out, bool *ordered_out) {
	const size_t count = scene.nodes.size(), camera_count = walk.primary_bytes / sizeof(NodeRec), loose_end = walk.unpruned_bytes / sizeof(NodeRec);
	const NodeRec *by_camera = walk.nodes.data(), *any_hit = (const NodeRec *) ((const char *) walk.nodes.data() + walk.ce_offset);
	std::vector<uint32_t> seen[2];
	seen[0].assign(scene.tris.size(), 0);
	seen[1].assign(scene.tris.size(), 0);
	bool tiles = true, ordered = true;
	auto outside2 = [&](const NodeRec &n) {
		double s = 0;
		for (int k = 0; k < 3; ++k) {
			const double dd = eye[k] < n.lo[k] ? n.lo[k] - eye[k] : eye[k] > n.hi[k] ? eye[k] - n.hi[k] : 0.0;
			s += dd * dd;
		}
		return s;
	};
	for (int copy = 0; copy < (walk.ce_offset ? 2 : 1); ++copy) {
		const NodeRec *nodes = copy ? any_hit : by_camera;
		const size_t here = copy ? count : camera_count;
		for (size_t i = 0; i < here; ++i) {
			const size_t skip = nodes[i].skip / sizeof(NodeRec);
			tiles = tiles && skip >= 1 && i + skip <= here;
			if (skip == 1) {
				if (nodes[i].leaf < scene.tris.size())
					++seen[copy][nodes[i].leaf];
				continue;
			}
			size_t c = i + 1, inside = 0;
			double before = -1.0;
			while (c < i + skip && c < here) {
				const size_t cs = nodes[c].skip / sizeof(NodeRec);
				if (cs == 0) { tiles = false; break; }
				if (copy == 0 && !(i == 0 && c < loose_end) && !(i >= 1 && i < loose_end)) {  // (the loose faces' subtree comes first whatever its distance)
					const double now = outside2(nodes[c]);
					ordered = ordered && now >= before - 1e-3 * (1.0 + before);  // (the records are padded: equal up to that)
					before = now;
				}
				inside += cs;
				c += cs;
			}
			tiles = tiles && inside + 1 == skip;
		}
	}
	bool same = true;
	for (size_t t = 0; t < scene.tris.size(); ++t)
		same = same && seen[0][t] == 1 && (!walk.ce_offset || seen[1][t] == 1);
	*tiles_out = tiles;
	*same_out = same;
	*ordered_out = ordered;
}

struct TreeTotals {
	unsigned long long rays = 0, exact = 0, pairs = 0, hits = 0, bounded_hits = 0, in_front = 0, missed_boxes = 0, outside = 0, pruned = 0;
};

// camera_margin_check.cc's three conditions for one ray against a whole walk array, every box above the leaf included.
void cast_through(const PackedScene &scene, const WalkArray &walk, const Records &r, const float eye[3], const float d[3], std::vector<char> &reached,
                  TreeTotals &t) {
	if (!selectable(eye, d, walk.origin_limit)) {
		++t.exact;
		return;
	}
	++t.rays;
	const KernelRay kr = kernel_ray(eye, d);
	const float below = std::nextafterf(100000.0f, 0.0f);
	std::fill(reached.begin(), reached.end(), 0);
	for (size_t i = 0; i < r.count;) {
		float far;
		const float near = kernel_near(r.rec[i], kr, &far);
		if (near <= std::fmin(far, below)) {
			reached[i] = 1;
			++i;
		} else {
			i += r.rec[i].skip / sizeof(NodeRec);
		}
	}
	for (size_t leaf = 0; leaf < scene.tris.size(); ++leaf) {
		const TriRec &tri = scene.tris[leaf];
		if (!reference_slab(tri.lo, tri.hi, eye, d, 100000.0f))
			continue;
		++t.pairs;
		const uint32_t at = r.record_of[leaf];
		if (at == 0xFFFFFFFFu || !reached[at]) {
			++t.missed_boxes;
			continue;
		}
		const Accepted h = reference_triangle(tri, eye, d);
		if (!h.ok)
			continue;
		++t.hits;
		if (!std::isfinite(walk.prune_margin) || r.loose((uint32_t) leaf) || !(h.distance < INF))
			continue;
		++t.bounded_hits;
		double own_near = 0.0;
		if (!box_near(tri.lo, tri.hi, eye, d, &own_near) || own_near > (double) h.distance)
			++t.in_front;
		bool inside = true;
		for (int k = 0; k < 3; ++k)
			inside = inside && h.ip[k] >= r.rec[at].lo[k] && h.ip[k] <= r.rec[at].hi[k];
		t.outside += !inside;
		const float limit = h.distance * 1.00001f + walk.prune_margin;
		for (uint32_t up = at; up != 0xFFFFFFFFu; up = r.parent[up]) {
			float far;
			if (kernel_near(r.rec[up], kr, &far) > limit) {
				++t.pruned;
				break;
			}
		}
	}
}

}  // namespace

int run_trees() {
	int bad = 0;
	auto expect = [&](bool ok, const char *what) {
		if (!ok) {
			std::printf("FAILED: %s\n", what);
			++bad;
		}
	};
	struct Case {
		unsigned faces;
		bool posed;
		float eye[3];
	};
	const Case cases[] = { { 200, false, { 0, 0, 2 } }, { 500, true, { 5.0f, -3.0f, 7.0f } }, { 1000, false, { 0, 0, 2 } },
		                   { 1000, true, { 0.3f, 0.2f, -0.4f } }, { 2000, true, { -40.0f, 25.0f, 10.0f } }, { 2000, false, { 0, 0, 2 } } };
	TreeTotals all;
	int number = 0;
	for (const Case &c : cases) {
		Rng rng(0x7ee50000ull + 104729ull * (uint64_t) number++);
		Mesh mesh;
		for (unsigned f = 0; f < c.faces; ++f) {
			// one face in six with eta in [1/64, 1/32), one in six in [1/32, 1/8], the others ordinary
			const unsigned kind = f % 6;
			const double kr = kind == 0 ? rng.range(2048.0 * 1.001, 4096.0 * 0.999) : kind == 1 ? rng.range(4096.0 * 1.001, 16384.0) : rng.log_range(1.0, 200.0);
			const double ratio = std::exp(rng.u() * std::log(std::fmin(kr, 16.0)));
			const double theta = std::asin(std::fmin(1.0, 1.0 / std::sqrt(kr / ratio)));
			const double shorter = rng.log_range(0.02, 0.3);
			float v[3][3];
			lay_triangle(rng, shorter * ratio, shorter, theta, rng.range(0.5, 3.0), v);
			for (int k = 0; k < 3; ++k) {
				mesh.vertices.push_back(Vec3f(v[k][0], v[k][1], v[k][2]));
				mesh.faces.push_back(3 * f + k);
			}
		}
		const PackedScene scene = pack(mesh);
		const WalkArray walk = make_walk_array(scene, 0.2f, true, c.posed ? c.eye : nullptr);
		expect(!walk.nodes.empty() && walk.eye_covered && std::isfinite(walk.prune_margin), "the tree is pruned for its eye");
		if (walk.nodes.empty() || !std::isfinite(walk.prune_margin))
			continue;
		const double eye_d[3] = { c.eye[0], c.eye[1], c.eye[2] };
		const double eye_distance = std::sqrt(eye_d[0] * eye_d[0] + eye_d[1] * eye_d[1] + eye_d[2] * eye_d[2]);
		bool tiles, same, ordered;
		check_structure(scene, walk, eye_d, &tiles, &same, &ordered);
		expect(tiles, "skip counts tile both copies");
		expect(same, "both copies hold every leaf once");
		expect(ordered, "the primary rays' copy lists children nearest to the eye first outside the unpruned head");
		const Records records(scene, walk);
		// faces without a bound lie in [1, unpruned_bytes / sizeof(NodeRec)), the others do not; both sides of the gate occur
		unsigned without = 0, just_below = 0, misplaced = 0;
		std::vector<uint32_t> bounded;
		for (uint32_t leaf = 0; leaf < scene.tris.size(); ++leaf) {
			const bool finite = leaf_growth(scene.tris[leaf], eye_distance) < 1e30;
			const double eta = eta_of(scene.tris[leaf]);
			without += !finite;
			just_below += finite && eta >= 1.0 / 64.0;
			misplaced += records.loose(leaf) == finite;
			if (finite)
				bounded.push_back(leaf);
		}
		expect(misplaced == 0, "the faces without a bound, and no others, lie in the unpruned head");
		expect(without >= c.faces / 8 && just_below >= c.faces / 8, "faces on both sides of the gate");
		expect(records.loose_end == 0 ? without == 0 : records.loose_end >= 1 + without, "the unpruned head holds a record per face without a bound");
		// rays aimed as in the sweep, at the faces that have a bound and at those that have none (their hits lower limits too)
		TreeTotals t;
		std::vector<char> reached(records.count);
		for (int ray = 0; ray < 1200; ++ray) {
			const uint32_t leaf = ray % 4 == 3 ? rng.below((unsigned) scene.tris.size()) : bounded[rng.below((unsigned) bounded.size())];
			const TriRec &tri = scene.tris[leaf];
			double s, q, w[3];
			target_parameters(rng, std::fmin(eta_of(tri), 0.05), &s, &q);
			for (int k = 0; k < 3; ++k)
				w[k] = (double) tri.ta[k] + s * (double) tri.u[k] + q * (double) tri.v[k] - (double) c.eye[k];
			if (!(w[0] * w[0] + w[1] * w[1] + w[2] * w[2] > 0.0))
				continue;
			float d[3];
			normalise_to_float(w, d);
			cast_through(scene, walk, records, c.eye, d, reached, t);
		}
		std::printf("prune_bound_sweep: tree of %u faces, eye (%g, %g, %g): %u faces without a bound (head of %zu records), %u with eta in [1/64, 1/32), margin %g; "
		            "%llu rays, %llu (ray, leaf) pairs, %llu accepted hits (%llu on faces with a bound, %llu of those in front of the own box): %llu boxes missed, %llu hits outside their box, %llu pruned wrongly\n",
		            c.faces, (double) c.eye[0], (double) c.eye[1], (double) c.eye[2], without, records.loose_end, just_below, (double) walk.prune_margin, t.rays,
		            t.pairs, t.hits, t.bounded_hits, t.in_front, t.missed_boxes, t.outside, t.pruned);
		all.rays += t.rays; all.pairs += t.pairs; all.hits += t.hits; all.bounded_hits += t.bounded_hits; all.in_front += t.in_front;
		all.missed_boxes += t.missed_boxes; all.outside += t.outside; all.pruned += t.pruned;
	}
	const unsigned long long violations = all.missed_boxes + all.outside + all.pruned;
	std::printf("prune_bound_sweep: trees: %llu rays, %llu accepted hits, %llu in front of their leaf's own box: %llu violations\n", all.rays, all.hits, all.in_front, violations);
	expect(all.bounded_hits >= 3000 && all.in_front >= 100, "the rays hit something, the slack zone too");
	expect(violations == 0, "no accepted hit lies outside a box above it or is pruned");
	if (!bad)
		std::printf("prune_bound_sweep: trees ok\n");
	return bad ? 1 : 0;
}

// See tests/prune_traps.py.  rays.f32: per ray eight floats (origin x y z 0, direction x y z 0), all from one eye.
int run_facts(const char *off, const char *rays_path, const char *out_path) {
	Mesh mesh;
	load_off_mesh(off, &mesh);
	BVH bvh(BVH::Method::CUT_LONGEST_AXIS);
	compute_vertex_normals(&mesh);
	bvh.buildBVH(mesh);
	const std::vector<uint32_t> sorted = sort_faces_by_leaf_order(mesh, bvh);
	const PackedScene scene = pack_scene(sorted, bvh.nodes, bvh.aabbs, mesh.vertices, mesh.vnormals);
	std::vector<float> rays;
	{
		FILE *f = std::fopen(rays_path, "rb");
		if (!f)
			return 2;
		float buffer[8];
		while (std::fread(buffer, sizeof(float), 8, f) == 8)
			rays.insert(rays.end(), buffer, buffer + 8);
		std::fclose(f);
	}
	if (rays.empty())
		return 2;
	const float eye[3] = { rays[0], rays[1], rays[2] };
	const WalkArray walk = make_walk_array(scene, 0.2f, true, eye);
	FILE *out = std::fopen(out_path, "w");
	if (!out)
		return 2;
	const double eye_distance = std::sqrt((double) eye[0] * eye[0] + (double) eye[1] * eye[1] + (double) eye[2] * eye[2]);
	std::fprintf(out, "facts %a %u %u %d %zu %zu\n", (double) walk.prune_margin, walk.unpruned_bytes, walk.primary_bytes, walk.eye_covered && !walk.nodes.empty() ? 1 : 0,
	             scene.tris.size(), rays.size() / 8);
	const Records records(scene, walk);
	for (uint32_t leaf = 0; leaf < scene.tris.size(); ++leaf) {
		// which of the file's faces the leaf holds: the one with its three vertices
		uint32_t face = 0xFFFFFFFFu;
		for (uint32_t f = 0; f < mesh.faces.size() / 3 && face == 0xFFFFFFFFu; ++f)
			if (mesh.faces[3 * f] == sorted[3 * leaf] && mesh.faces[3 * f + 1] == sorted[3 * leaf + 1] && mesh.faces[3 * f + 2] == sorted[3 * leaf + 2])
				face = f;
		const double g = leaf_growth(scene.tris[leaf], eye_distance);
		std::fprintf(out, "leaf %u %u %a %d %a\n", leaf, face, g, walk.nodes.empty() ? 0 : (int) records.loose(leaf), eta_of(scene.tris[leaf]));
	}
	for (size_t r = 0; r < rays.size() / 8; ++r) {
		const float *o = &rays[8 * r], *d = &rays[8 * r + 4];
		struct Hit {
			uint32_t leaf;
			float distance;
		};
		std::vector<Hit> accepted;
		for (uint32_t leaf = 0; leaf < scene.tris.size(); ++leaf) {
			const TriRec &t = scene.tris[leaf];
			if (!reference_slab(t.lo, t.hi, o, d, 100000.0f))
				continue;
			const Accepted h = reference_triangle(t, o, d);
			if (h.ok && h.distance < 100000.0f)
				accepted.push_back({ leaf, h.distance });
		}
		int winner = -1;
		for (size_t k = 0; k < accepted.size(); ++k)
			if (winner < 0 || accepted[k].distance < accepted[winner].distance)
				winner = (int) k;  // (leaves ascend: the first of equal distances is the lower leaf)
		bool in_front = false, trap = false;
		if (winner >= 0) {
			const TriRec &t = scene.tris[accepted[winner].leaf];
			double own_near = 0.0;
			const bool met = box_near(t.lo, t.hi, o, d, &own_near);
			in_front = met && own_near > (double) accepted[winner].distance;
			for (size_t k = 0; in_front && k < accepted.size(); ++k)
				if ((int) k != winner && accepted[k].distance > accepted[winner].distance &&
				    own_near > (double) accepted[k].distance * (1.0 + 1e-5) + (double) walk.prune_margin)
					trap = true;
		}
		std::fprintf(out, "ray %zu %d %d %d %zu", r, winner >= 0 ? (int) accepted[winner].leaf : -1, (int) in_front, (int) trap, accepted.size());
		for (const Hit &h : accepted) {
			uint32_t word;
			std::memcpy(&word, &h.distance, sizeof word);
			std::fprintf(out, " %u %u", h.leaf, word);
		}
		std::fprintf(out, "\n");
	}
	std::fclose(out);
	return 0;
}

int run_model(const char *off, const char *rays_path) {
	Mesh mesh;
	load_off_mesh(off, &mesh);
	const PackedScene scene = pack(mesh);
	std::vector<float> rays;
	{
		FILE *f = std::fopen(rays_path, "rb");
		if (!f)
			return 2;
		float buffer[8];
		while (std::fread(buffer, sizeof(float), 8, f) == 8)
			rays.insert(rays.end(), buffer, buffer + 8);
		std::fclose(f);
	}
	if (rays.empty())
		return 2;
	const float eye[3] = { rays[0], rays[1], rays[2] };
	const WalkArray walk = make_walk_array(scene, 0.2f, true, eye);
	if (walk.nodes.empty() || !walk.eye_covered)
		return 2;
	const size_t count = walk.primary_bytes / sizeof(NodeRec);
	unsigned changed = 0, exact = 0;
	for (size_t r = 0; r < rays.size() / 8; ++r) {
		const float *o = &rays[8 * r], *d = &rays[8 * r + 4];
		if (!selectable(o, d, walk.origin_limit)) {
			++exact;
			continue;
		}
		float reference = INF, best = INF;
		uint32_t reference_leaf = 0xFFFFFFFFu, best_leaf = 0xFFFFFFFFu;
		for (uint32_t leaf = 0; leaf < scene.tris.size(); ++leaf) {
			const TriRec &t = scene.tris[leaf];
			if (!reference_slab(t.lo, t.hi, o, d, 100000.0f))
				continue;
			const Accepted h = reference_triangle(t, o, d);
			if (h.ok && h.distance < reference) {
				reference = h.distance;
				reference_leaf = leaf;
			}
		}
		const KernelRay kr = kernel_ray(o, d);
		float far_limit = std::nextafterf(100000.0f, 0.0f);
		for (size_t i = 0; i < count;) {
			float far;
			const float near = kernel_near(walk.nodes[i], kr, &far);
			if (!(near <= std::fmin(far, far_limit))) {
				i += walk.nodes[i].skip / sizeof(NodeRec);
				continue;
			}
			if (walk.nodes[i].skip == sizeof(NodeRec) && walk.nodes[i].leaf < scene.tris.size()) {
				const uint32_t leaf = walk.nodes[i].leaf;
				const TriRec &t = scene.tris[leaf];
				if (reference_slab(t.lo, t.hi, o, d, 100000.0f)) {
					const Accepted h = reference_triangle(t, o, d);
					if (h.ok && (h.distance < best || (h.distance == best && leaf < best_leaf))) {
						best = h.distance;
						best_leaf = leaf;
					}
					if (h.ok && best < INF && i * sizeof(NodeRec) >= walk.unpruned_bytes)
						far_limit = std::fmin(far_limit, best * 1.00001f + walk.prune_margin);
				}
			}
			++i;
		}
		changed += best_leaf != reference_leaf;
	}
	std::printf("prune_bound_sweep: model: margin %g, %u of %zu rays end with another leaf than the reference (%u in packets of the exact form)\n",
	            (double) walk.prune_margin, changed, rays.size() / 8, exact);
	return 0;
}
