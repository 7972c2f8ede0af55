// instance_nearest_margin_check.cc -- the pruning bounds of the instanced closest-point queries (csrc/instance_nearest.h:
// inp_reach, inp_object_limit2; csrc/instances.cc: instance_bounds), swept, and a host-side nested walk built on them against
// brute force.  A stand-alone host program (tests/test_instance_nearest_cpu.py compiles it with csrc/instances.cc, with the
// sanitizers, and runs it); it compiles the same instance_nearest.h and nearest_point.h as the kernel and the C oracle.
//
// 1. The sweep.  Over adversarial (transform, object triangle, enclosing object box, world point) quadruples -- uniform scales
//    1/4 .. 4, shears with singular-value ratios up to 8, mirrors, rotations, copies moved far from the origin; boxes tight and
//    loose; points on, near and far from the copy; and the TIGHT family: a triangle lying in a face of its box, the point
//    straight above it, the face's normal along the map's smallest singular direction, where the bound is met with equality
//    but for the margins -- neither predicate may pass by a box whose world triangle's float32 d2 is <= the bound: the
//    top-level box by inp_reach squared, the object box by inp_object_limit2, with the bound at that very d2 (a tie), one ulp
//    above it, and with the radius at that triangle's float32 distance.
// 2. The walk.  For every scene file given (header: nodes, leaves, vertices, instances; then the skips, the boxes as float4
//    pairs, the leaf-ordered faces, the vertices as float4, the transforms as 12 floats): each point goes down both trees for
//    a starting bound and then walks the top-level and the scene's skip-pointer order as kernels/instance_nearest.hip.h does
//    lane by lane; (d2, instance, leaf, s, t, p) must equal the brute-force minimum bit for bit, for radii inf, 0.3, 0.02, 0.
// --inflate-scale X multiplies every copy's `scale` by X (the test runs 1.02 and expects violations): the sweep has teeth.
// --box-points N: the walk alone, radius inf, on N points uniform in the top-level root box (the first 64 against brute force),
// to print the share of all pairs it tests.
// Prints "violations N" and "walk mismatches N"; exit code 0 = both 0.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../opencl_raytracer_amd/csrc/instance_nearest.h"
#include "../opencl_raytracer_amd/csrc/instances.h"

namespace {

float g_inflate = 1.0f;

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

inp_rows rows_of(const float *m12) {
	inp_rows r;
	std::memcpy(r.m, m12, sizeof r.m);
	return r;
}

inp_bounds bounds_of(const float *b4) {
	inp_bounds b;
	b.scale = b4[0] * g_inflate;
	b.per_q = b4[1];
	b.fixed = b4[2];
	b.world = b4[3];
	return b;
}

float max_abs(const float q[3]) { return fmaxf(fmaxf(fabsf(q[0]), fabsf(q[1])), fabsf(q[2])); }

// What the library makes of a set for a scene with this root box.
struct Plan {
	std::vector<float> W, O, bounds;
	std::vector<ocrt::InstanceNode> nodes;
	bool make(const float root_lo[3], const float root_hi[3], const std::vector<float> &transforms) {
		W = transforms;
		const uint32_t n = (uint32_t) (W.size() / 12u);
		if (!ocrt::instance_inverses(W.data(), n, O))
			return false;
		ocrt::instance_bounds(root_lo, root_hi, W.data(), O.data(), n, bounds);
		ocrt::instance_tree(root_lo, root_hi, W.data(), O.data(), n, nodes);
		return true;
	}
	float magnitude(const float q[3]) const {
		const ocrt::InstanceNode &r = nodes[0];
		return np_magnitude(r.lo[0], r.lo[1], r.lo[2], r.hi[0], r.hi[1], r.hi[2], q[0], q[1], q[2]);
	}
};

// ---- the sweep ------------------------------------------------------------------------------------------------------------
uint64_t g_quads = 0, g_violations = 0, g_nan = 0, g_refused = 0;

void rotation(std::mt19937_64 &rng, double R[3][3]) {  // a random rotation from a unit quaternion
	std::normal_distribution<double> normal(0.0, 1.0);
	double q[4], len = 0.0;
	for (double &x : q) {
		x = normal(rng);
		len += x * x;
	}
	len = std::sqrt(len);
	for (double &x : q)
		x /= len;
	const double w = q[0], x = q[1], y = q[2], z = q[3];
	const double r[3][3] = { { 1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w) },
		                     { 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w) },
		                     { 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y) } };
	std::memcpy(R, r, sizeof r);
}

struct Box {
	float lo[3], hi[3];
};

void check_quad(const Plan &plan, const float a[3], const float b[3], const float c[3], const Box &box, const float q[3]) {
	const inp_rows W = rows_of(plan.W.data()), O = rows_of(plan.O.data());
	const np_point r = np_nearest(inp_world_tri(W, make_tri(a, b, c)), q[0], q[1], q[2]);
	++g_quads;
	if (!(r.d2 >= 0.0f) || !(r.d2 < INFINITY)) {
		if (g_nan++ < 5)
			std::printf("no number: d2 %g for q (%g %g %g)\n", r.d2, q[0], q[1], q[2]);
		return;
	}
	const float m = plan.magnitude(q);
	const inp_bounds bounds = bounds_of(plan.bounds.data());
	float o[3];
	inp_object_point(O, q[0], q[1], q[2], &o[0], &o[1], &o[2]);
	const float slack = inp_slack(bounds, max_abs(q));
	const float object_d2 = np_box_d2(box.lo[0], box.lo[1], box.lo[2], box.hi[0], box.hi[1], box.hi[2], o[0], o[1], o[2]);
	const ocrt::InstanceNode &top = plan.nodes[0];
	const float top_d2 = np_box_d2(top.lo[0], top.lo[1], top.lo[2], top.hi[0], top.hi[1], top.hi[2], q[0], q[1], q[2]);
	const float reaches[3] = { inp_reach(r.d2, m), inp_reach(std::nextafterf(r.d2, INFINITY), m), inp_reach_of_distance(sqrtf(r.d2), m) };
	for (int k = 0; k < 3; ++k) {
		const bool object = np_prune(object_d2, inp_object_limit2(reaches[k], bounds, slack));
		const bool world = np_prune(top_d2, reaches[k] * reaches[k]);
		if ((object || world) && g_violations++ < 10)
			std::printf("violation (%s, bound %d): box d2 %.9g (object) %.9g (top level), triangle d2 %.9g, magnitude %g, scale %g\n",
			            object ? "object box" : "top-level box", k, object_d2, top_d2, r.d2, m, bounds.scale);
	}
}

void sweep() {
	std::mt19937_64 rng(2468);
	std::uniform_real_distribution<float> unit(-1.0f, 1.0f), zero_one(0.0f, 1.0f);
	const double scales[] = { 0.25, 0.5, 1.0, 2.0, 4.0 };
	const double shears[][3] = { { 1, 2, 8 }, { 0.5, 1, 3 }, { 2, 0.25, 1 }, { 1, 1, 6 }, { 8, 4, 1 }, { 1, 1, 1 } };
	for (int round = 0; round < 24000; ++round) {
		// the transform: A = U diag(s) V^T, about the triangle's neighbourhood, moved by `shift`
		double U[3][3], V[3][3], s[3];
		rotation(rng, U);
		rotation(rng, V);
		const int family = round % 6;  // 0 uniform scale, 1 shear, 2 mirror, 3 rotation, 4 axis-aligned stretch, 5 TIGHT
		if (family == 0)
			s[0] = s[1] = s[2] = scales[(round / 6) % 5];
		else if (family == 3)
			s[0] = s[1] = s[2] = 1.0;
		else
			for (int k = 0; k < 3; ++k)
				s[k] = shears[(round / 6) % 6][k];
		if (family == 2)
			s[(round / 36) % 3] *= -1.0;
		if (family == 4 || family == 5)  // V = I: the singular directions are the object axes
			for (int i = 0; i < 3; ++i)
				for (int j = 0; j < 3; ++j)
					V[i][j] = i == j ? 1.0 : 0.0;
		if (family == 5 && (round / 6) % 2)  // ... a uniform scale half of the time: every direction is the smallest
			s[0] = s[1] = s[2] = scales[(round / 12) % 5];
		const float size = (round / 72) % 3 == 0 ? 1.0f : ((round / 72) % 3 == 1 ? 37.0f : 1e-2f);
		const float offset = (round / 216) % 2 ? size * 20.0f * unit(rng) : 0.0f;  // the object far from its own origin
		const double far = (round / 432) % 2 ? 300.0 * size : 0.0;               // the copy far from the world's
		std::vector<float> W(12);
		for (int i = 0; i < 3; ++i) {
			for (int j = 0; j < 3; ++j) {
				double e = 0.0;
				for (int k = 0; k < 3; ++k)
					e += U[i][k] * s[k] * V[j][k];
				W[4 * i + j] = (float) e;
			}
			W[4 * i + 3] = (float) (far * unit(rng) + size * unit(rng));
		}
		// the object triangle and its boxes
		float a[3], b[3], c[3];
		for (int k = 0; k < 3; ++k) {
			a[k] = offset + size * unit(rng);
			b[k] = offset + size * unit(rng);
			c[k] = offset + size * unit(rng);
		}
		int axis = 2;  // TIGHT: the axis of the smallest |s|
		for (int k = 0; k < 3; ++k)
			if (std::fabs(s[k]) < std::fabs(s[axis]))
				axis = k;
		const int kind = (round / 6) % 4;
		if (family == 5)
			a[axis] = b[axis] = c[axis];  // the triangle lies in a face of its tight box
		else if (kind == 1)  // a sliver
			for (int k = 0; k < 3; ++k)
				c[k] = a[k] + (b[k] - a[k]) * 0.37f + size * 1e-6f * unit(rng);
		else if (kind == 2)  // two vertices coincide
			for (int k = 0; k < 3; ++k)
				c[k] = b[k];
		Box tight, loose, root;
		for (int k = 0; k < 3; ++k) {
			tight.lo[k] = fminf(a[k], fminf(b[k], c[k]));
			tight.hi[k] = fmaxf(a[k], fmaxf(b[k], c[k]));
			loose.lo[k] = tight.lo[k] - size * zero_one(rng);
			loose.hi[k] = tight.hi[k] + size * zero_one(rng);
			root.lo[k] = loose.lo[k] - size * zero_one(rng);  // (the scene's root box holds every box)
			root.hi[k] = loose.hi[k] + size * zero_one(rng);
		}
		Plan plan;
		if (!plan.make(root.lo, root.hi, W)) {
			++g_refused;
			continue;
		}
		// points, given in object space and mapped by W in binary64: on the triangle, near it, far from it
		const float u = zero_one(rng), v = zero_one(rng) * (1.0f - u);
		double on[4][3];
		for (int k = 0; k < 3; ++k) {
			on[0][k] = a[k];
			on[1][k] = (double) a[k] + ((double) b[k] - a[k]) * u;
			on[2][k] = (double) a[k] + (((double) b[k] - a[k]) * u + ((double) c[k] - a[k]) * v);
			on[3][k] = ((double) a[k] + b[k] + c[k]) / 3.0;
		}
		const double reach[] = { 0.0, 1e-6, 1e-3, 0.1, 1.0, 10.0, 1e3 };
		for (const auto &p : on)
			for (double d : reach) {
				double x[3];
				for (int k = 0; k < 3; ++k)
					x[k] = p[k] + (family == 5 ? 0.0 : (std::fabs(offset) + size) * d * unit(rng));
				if (family == 5)  // straight off the face, along the smallest singular direction
					x[axis] = p[axis] + ((round / 6) % 2 ? 1.0 : -1.0) * size * (d == 0.0 ? 0.25 : d);
				float q[3];
				for (int i = 0; i < 3; ++i)
					q[i] = (float) ((((double) W[4 * i] * x[0] + (double) W[4 * i + 1] * x[1]) + (double) W[4 * i + 2] * x[2]) + (double) W[4 * i + 3]);
				check_quad(plan, a, b, c, tight, q);
				check_quad(plan, a, b, c, loose, q);
			}
	}
}

// ---- the walk -------------------------------------------------------------------------------------------------------------
struct Scene {
	std::vector<uint32_t> skips, leaf_of_node, faces;
	std::vector<float> boxes, vertices, transforms;  // float4 pairs; float4; 12 floats
	uint32_t nodes = 0, leaves = 0;
	Plan plan;
	np_tri leaf(uint32_t l) const { return make_tri(&vertices[4 * faces[3 * l]], &vertices[4 * faces[3 * l + 1]], &vertices[4 * faces[3 * l + 2]]); }
	float box_d2(uint32_t i, const float q[3]) const {
		const float *lo = &boxes[8 * i], *hi = lo + 4;
		return np_box_d2(lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], q[0], q[1], q[2]);
	}
	uint32_t instances() const { return (uint32_t) (transforms.size() / 12u); }
};

bool load(const char *path, Scene &s) {
	std::FILE *f = std::fopen(path, "rb");
	if (!f)
		return false;
	uint32_t head[4];
	bool ok = std::fread(head, 4, 4, f) == 4 && head[0] > 0 && head[3] > 0;
	if (ok) {
		s.nodes = head[0];
		s.leaves = head[1];
		s.skips.resize(head[0]);
		s.boxes.resize(8 * (size_t) head[0]);
		s.faces.resize(3 * (size_t) head[1]);
		s.vertices.resize(4 * (size_t) head[2]);
		s.transforms.resize(12 * (size_t) head[3]);
		ok = std::fread(s.skips.data(), 4, s.skips.size(), f) == s.skips.size() && std::fread(s.boxes.data(), 4, s.boxes.size(), f) == s.boxes.size() &&
		     std::fread(s.faces.data(), 4, s.faces.size(), f) == s.faces.size() &&
		     std::fread(s.vertices.data(), 4, s.vertices.size(), f) == s.vertices.size() &&
		     std::fread(s.transforms.data(), 4, s.transforms.size(), f) == s.transforms.size();
	}
	std::fclose(f);
	if (!ok)
		return false;
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
	return ok && next == s.leaves && s.plan.make(&s.boxes[0], &s.boxes[4], s.transforms);
}

struct Record {
	float d2 = INFINITY;
	uint32_t instance = 0xFFFFFFFFu, leaf = 0xFFFFFFFFu;
	np_point p = { 0, 0, 0, 0, 0, 0 };
	uint64_t tests = 0;
	bool take(const Scene &s, uint32_t k, uint32_t l, const float q[3]) {
		const np_point r = np_nearest(inp_world_tri(rows_of(&s.plan.W[12 * (size_t) k]), s.leaf(l)), q[0], q[1], q[2]);
		++tests;
		if (!inp_better(r.d2, k, l, d2, instance, leaf))
			return false;
		d2 = r.d2;
		instance = k;
		leaf = l;
		p = r;
		return true;
	}
};

Record brute(const Scene &s, const float q[3]) {
	Record best;
	for (uint32_t k = 0; k < s.instances(); ++k)
		for (uint32_t l = 0; l < s.leaves; ++l)
			best.take(s, k, l, q);
	return best;
}

// A lane's own way down a tree of skip records: the node it ends at.
template <class Skip, class BoxD2> uint32_t down(uint32_t count, Skip &&skip, BoxD2 &&box_d2) {
	uint32_t at = 0;
	while (at < count && skip(at) != 1) {
		const uint32_t end = at + skip(at);
		uint32_t pick = 0xFFFFFFFFu;
		float pick_d2 = 0.0f;
		for (uint32_t c = at + 1; c < end; c += skip(c)) {
			const float d2 = box_d2(c);
			if (pick == 0xFFFFFFFFu || d2 < pick_d2) {
				pick = c;
				pick_d2 = d2;
			}
		}
		at = pick;
	}
	return at;
}

Record walk(const Scene &s, const float q[3], float max_distance) {
	Record best;
	const Plan &plan = s.plan;
	const std::vector<ocrt::InstanceNode> &top = plan.nodes;
	const float m = plan.magnitude(q), q_max = max_abs(q);
	const float radius_reach = inp_reach_of_distance(max_distance, m);
	auto top_d2 = [&](uint32_t i) { return np_box_d2(top[i].lo[0], top[i].lo[1], top[i].lo[2], top[i].hi[0], top[i].hi[1], top[i].hi[2], q[0], q[1], q[2]); };
	auto object_point = [&](uint32_t k, float o[3]) { inp_object_point(rows_of(&plan.O[12 * (size_t) k]), q[0], q[1], q[2], &o[0], &o[1], &o[2]); };
	// the descent, through both trees
	{
		const uint32_t k = top[down((uint32_t) top.size(), [&](uint32_t i) { return top[i].skip; }, top_d2)].leaf;
		float o[3];
		object_point(k, o);
		const uint32_t at = down(s.nodes, [&](uint32_t i) { return s.skips[i]; }, [&](uint32_t i) { return s.box_d2(i, o); });
		best.take(s, k, s.leaf_of_node[at], q);
	}
	float reach = fminf(radius_reach, inp_reach(best.d2, m));
	// the fixed order, nested
	for (uint32_t t = 0; t < top.size();) {
		if (np_prune(top_d2(t), reach * reach)) {
			t += top[t].skip;
			continue;
		}
		if (top[t].skip == 1) {
			const uint32_t k = top[t].leaf;
			const inp_bounds bounds = bounds_of(&plan.bounds[4 * (size_t) k]);
			float o[3];
			object_point(k, o);
			const float slack = inp_slack(bounds, q_max);
			float limit2 = inp_object_limit2(reach, bounds, slack);
			for (uint32_t i = 0; i < s.nodes;) {
				if (np_prune(s.box_d2(i, o), limit2)) {
					i += s.skips[i];
					continue;
				}
				if (s.skips[i] == 1 && best.take(s, k, s.leaf_of_node[i], q)) {
					reach = fminf(radius_reach, inp_reach(best.d2, m));
					limit2 = inp_object_limit2(reach, bounds, slack);
				}
				++i;
			}
		}
		++t;
	}
	return best;
}

uint64_t g_walks = 0, g_mismatches = 0, g_walk_tests = 0, g_brute_tests = 0, g_compared = 0;

void compare(const Scene &s, const char *name, size_t i, const float *q, float radius, const Record &want) {
	const Record got = walk(s, q, radius);
	++g_walks;
	g_walk_tests += got.tests;
	// within the radius the record is brute force's, bit for bit; beyond it both sides say "not found"
	const bool found = want.d2 < INFINITY && sqrtf(want.d2) <= radius;
	const bool got_found = got.d2 < INFINITY && sqrtf(got.d2) <= radius;
	const bool same = found ? (got_found && got.instance == want.instance && got.leaf == want.leaf && std::memcmp(&got.p, &want.p, sizeof got.p) == 0)
	                        : !got_found;
	if (!same && g_mismatches++ < 10)
		std::printf("%s: point %zu radius %g: walk (%.9g, instance %u, leaf %u), brute force (%.9g, instance %u, leaf %u)\n", name, i, radius,
		            got.d2, got.instance, got.leaf, want.d2, want.instance, want.leaf);
}

void walk_scene(const Scene &s, const char *name, uint32_t box_points) {
	std::mt19937_64 rng(777);
	std::uniform_real_distribution<float> unit(-1.0f, 1.0f);
	const ocrt::InstanceNode &root = s.plan.nodes[0];
	std::vector<float> points;
	if (box_points) {
		for (uint32_t i = 0; i < box_points; ++i)
			for (int k = 0; k < 3; ++k)
				points.push_back((root.lo[k] + root.hi[k]) * 0.5f + (root.hi[k] - root.lo[k]) * 0.5f * unit(rng));
		uint64_t tests = 0;
		for (size_t i = 0; i + 2 < points.size(); i += 3) {
			if (i / 3 < 64) {
				const Record want = brute(s, &points[i]);
				g_brute_tests += want.tests;
				++g_compared;
				compare(s, name, i / 3, &points[i], INFINITY, want);
			}
			tests += walk(s, &points[i], INFINITY).tests;
		}
		std::printf("%s: %u points in the top-level box: share of all pairs tested %.6f\n", name, box_points,
		            (double) tests / ((double) box_points * s.instances() * s.leaves));
		return;
	}
	for (int i = 0; i < 240; ++i) {
		const float reach = i < 160 ? 0.625f : (i < 200 ? 3.0f : 1500.0f);  // in the top-level box x 1.25, a few sizes out, 1e3 out
		for (int k = 0; k < 3; ++k) {
			const float extent = root.hi[k] - root.lo[k] > 0.0f ? root.hi[k] - root.lo[k] : 1.0f;
			points.push_back((root.lo[k] + root.hi[k]) * 0.5f + extent * reach * unit(rng));
		}
	}
	for (uint32_t j = 0; j < 60; ++j) {  // on the world surface: vertices of world triangles
		const uint32_t k = j % s.instances(), l = (j * 7u) % s.leaves;
		const np_tri t = inp_world_tri(rows_of(&s.plan.W[12 * (size_t) k]), s.leaf(l));
		points.insert(points.end(), { t.tax, t.tay, t.taz });
	}
	const float radii[] = { INFINITY, 0.3f, 0.02f, 0.0f };
	for (size_t i = 0; i + 2 < points.size(); i += 3) {
		const Record want = brute(s, &points[i]);
		g_brute_tests += 4 * want.tests;
		g_compared += 4;
		for (float radius : radii)
			compare(s, name, i / 3, &points[i], radius, want);
	}
}

}  // namespace

int main(int argc, char **argv) {
	uint32_t box_points = 0;
	std::vector<const char *> files;
	for (int i = 1; i < argc; ++i) {
		if (!std::strcmp(argv[i], "--inflate-scale") && i + 1 < argc)
			g_inflate = (float) std::atof(argv[++i]);
		else if (!std::strcmp(argv[i], "--box-points") && i + 1 < argc)
			box_points = (uint32_t) std::atoi(argv[++i]);
		else
			files.push_back(argv[i]);
	}
	if (!box_points)
		sweep();
	std::printf("quadruples %" PRIu64 " (transforms refused %" PRIu64 "), no number %" PRIu64 ", violations %" PRIu64 "\n", g_quads, g_refused, g_nan,
	            g_violations + g_nan);
	for (const char *path : files) {
		Scene s;
		if (!load(path, s)) {
			std::printf("cannot read %s\n", path);
			return 2;
		}
		walk_scene(s, path, box_points);
	}
	std::printf("walks %" PRIu64 ", triangle tests per compared walk %.1f (brute force %.1f), walk mismatches %" PRIu64 "\n", g_walks,
	            g_walks ? (double) g_walk_tests / (double) g_walks : 0.0, g_compared ? (double) g_brute_tests / (double) g_compared : 0.0, g_mismatches);
	return g_violations + g_nan + g_mismatches == 0 ? 0 : 1;
}
