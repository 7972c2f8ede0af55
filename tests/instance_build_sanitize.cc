// instance_build_sanitize.cc -- the host restatement of a device-side instance build (csrc/instance_build.cc,
// rt_instance_plan_lbvh; include/rt_hip_instance_build.h) under the address and undefined-behaviour sanitizers: a stand-alone
// program, no device.  TEST INFRASTRUCTURE ONLY.
// Built and run by tests/test_instance_build_cpu.py: g++ -fsanitize=address,undefined instance_build_sanitize.cc
// csrc/instance_build.cc csrc/instances.cc.
// It plans sets of its own making at the instance counts of the tests, sets whose keys are all equal, root boxes that are not
// finite and coordinates at the ends of binary32's range into buffers of exactly the documented sizes, walks every tree, holds
// inverses, leaf boxes and bounds against the host planner's (rt_instance_plan, ocrt::instance_bounds), and tries the refusals.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/rt_hip_instance_build.h"
#include "../opencl_raytracer_amd/csrc/instances.h"

namespace {

struct Node {
	float lo[3];
	uint32_t skip;
	float hi[3];
	uint32_t leaf;
};

uint32_t state = 2463534242u;
float uniform() {  // xorshift, [0, 1)
	state ^= state << 13;
	state ^= state >> 17;
	state ^= state << 5;
	return (float) (state >> 8) * (1.0f / 16777216.0f);
}

void pose(float *W, float sx, float sy, float sz, float shear, float tx, float ty, float tz) {
	const float angle = uniform() * 6.2831853f, c = std::cos(angle), s = std::sin(angle);
	const float R[3][3] = { { c, -s, 0.0f }, { s, c, 0.0f }, { 0.0f, 0.0f, 1.0f } };
	const float S[3][3] = { { sx, shear, 0.0f }, { 0.0f, sy, shear }, { 0.0f, 0.0f, sz } };
	for (int i = 0; i < 3; ++i) {
		for (int j = 0; j < 3; ++j)
			W[4 * i + j] = R[i][0] * S[0][j] + R[i][1] * S[1][j] + R[i][2] * S[2][j];
		W[4 * i + 3] = i == 0 ? tx : i == 1 ? ty : tz;
	}
}

int failures = 0;
void expect(bool ok, const char *what) {
	if (!ok) {
		std::printf("FAILED: %s\n", what);
		++failures;
	}
}

bool same_bits(const float *a, const float *b, size_t n) { return std::memcmp(a, b, n * sizeof(float)) == 0; }

// Plans `W` into buffers of exactly 12 n floats, 2 n - 1 records and 4 n floats; the tree's shape, every inner box, and the
// numbers against the host planner's.
void plan(const float lo[3], const float hi[3], const std::vector<float> &W, const char *what, bool finite_root = true) {
	const uint32_t n = (uint32_t) (W.size() / 12u);
	std::vector<float> O((size_t) n * 12u), bounds((size_t) n * 4u), O_host((size_t) n * 12u);
	std::vector<Node> nodes(2u * (size_t) n - 1u), host(2u * (size_t) n - 1u);
	expect(rt_instance_plan_lbvh(lo, hi, W.data(), n, O.data(), nodes.data(), bounds.data()) == RT_OK, what);
	expect(rt_instance_plan(lo, hi, W.data(), n, O_host.data(), host.data()) == RT_OK, what);
	expect(same_bits(O.data(), O_host.data(), O.size()), "the inverses are the host planner's");
	std::vector<const Node *> mine(n, nullptr), theirs(n, nullptr);
	for (size_t i = 0; i < nodes.size(); ++i) {
		expect(nodes[i].skip >= 1u && nodes[i].skip % 2u == 1u && i + nodes[i].skip <= nodes.size(), "a skip leaves the array");
		if (nodes[i].leaf != 0xFFFFFFFFu) {
			expect(nodes[i].leaf < n && nodes[i].skip == 1u, "a leaf record");
			if (nodes[i].leaf < n) {
				expect(mine[nodes[i].leaf] == nullptr, "every instance once");
				mine[nodes[i].leaf] = &nodes[i];
			}
		} else if (nodes[i].skip >= 3u && i + nodes[i].skip <= nodes.size()) {
			const Node &a = nodes[i + 1u], &b = nodes[i + 1u + a.skip];
			expect(a.skip + b.skip + 1u == nodes[i].skip, "the children tile their parent");
			for (int k = 0; k < 3; ++k) {
				const float want_lo = b.lo[k] < a.lo[k] ? b.lo[k] : a.lo[k], want_hi = a.hi[k] < b.hi[k] ? b.hi[k] : a.hi[k];
				expect(same_bits(&nodes[i].lo[k], &want_lo, 1) && same_bits(&nodes[i].hi[k], &want_hi, 1), "an inner box");
			}
		} else {
			expect(false, "an inner record with a leaf's skip");
		}
		if (host[i].leaf != 0xFFFFFFFFu && host[i].leaf < n)
			theirs[host[i].leaf] = &host[i];
	}
	for (uint32_t k = 0; k < n; ++k) {
		expect(mine[k] && theirs[k], "every instance once");
		if (mine[k] && theirs[k])
			expect(same_bits(mine[k]->lo, theirs[k]->lo, 3) && same_bits(mine[k]->hi, theirs[k]->hi, 3), "the leaf box is the host planner's");
	}
	std::vector<float> bounds_host;
	ocrt::instance_bounds(lo, hi, W.data(), O_host.data(), n, bounds_host);
	if (finite_root)  // (a root box that is not finite leaves NaNs in the bounds' last words: their payload is nobody's promise)
		expect(same_bits(bounds.data(), bounds_host.data(), bounds.size()), "the bounds are instance_bounds's");
	for (uint32_t k = 0; k < n && !finite_root; ++k)
		expect(bounds[4u * k] == 0.0f, "nothing is passed by under a root box that is not finite");
	expect(rt_instance_plan_lbvh(lo, hi, W.data(), n, nullptr, nullptr, nullptr) == RT_OK, "no outputs");
	expect(rt_instance_plan_lbvh(lo, hi, W.data(), n, nullptr, nodes.data(), nullptr) == RT_OK, "the tree alone");
}

}  // namespace

int main() {
	const float lo[3] = { -0.3f, 0.1f, -0.2f }, hi[3] = { 0.4f, 0.9f, 0.25f };
	const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
	std::vector<float> W;
	auto add = [&](float sx, float sy, float sz, float shear, float tx, float ty, float tz) {
		W.resize(W.size() + 12u);
		pose(W.data() + W.size() - 12u, sx, sy, sz, shear, tx, ty, tz);
	};
	const float identity[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
	plan(lo, hi, std::vector<float>(identity, identity + 12), "identity");
	for (uint32_t n : { 1u, 2u, 3u, 64u, 65u, 257u, 1000u, 4099u }) {
		W.clear();
		for (uint32_t k = 0; k < n; ++k)
			add(0.5f + uniform(), 0.5f + uniform(), 0.5f + uniform(), 0.3f * uniform(), 20.0f * uniform(), 20.0f * uniform(), 20.0f * uniform());
		plan(lo, hi, W, "counts");
		const float broken[3] = { hi[0], n % 2u ? inf : nan, hi[2] };
		plan(lo, broken, W, "a root box that is not finite", false);
	}
	W.clear();  // shear, a mirror, a flat spread: no extent on two axes of the keys
	add(1, 2, 8, 0.5f, 1, 0, 0);
	add(0.5f, 1, 3, -0.25f, 0, 2, 0);
	add(-1, 1, 1, 0, 0, 0, 0);
	plan(lo, hi, W, "shear and mirror");
	W.clear();
	for (int k = 0; k < 300; ++k) {
		W.insert(W.end(), identity, identity + 12);
		W[W.size() - 12u + 3u] = 0.01f * (float) k;
	}
	plan(lo, hi, W, "a row of copies");
	// every key equal: the order is by index, the tree a chain of splits behind the first rank
	W.clear();
	for (int k = 0; k < 513; ++k)
		W.insert(W.end(), identity, identity + 12);
	plan(lo, hi, W, "equal keys");
	{
		std::vector<Node> nodes(2u * 513u - 1u);
		expect(rt_instance_plan_lbvh(lo, hi, W.data(), 513u, nullptr, nodes.data(), nullptr) == RT_OK, "equal keys");
		uint32_t next = 0;
		for (const Node &node : nodes)
			if (node.leaf != 0xFFFFFFFFu)
				expect(node.leaf == next++, "equal keys come out in rising index");
	}
	W[3] = 3.0e38f;
	W[12 + 7] = -3.0e38f;
	W[24 + 0] = 1.0e-30f;
	plan(lo, hi, W, "huge and tiny");
	// the refusals, at the first, a middle and the last index: nothing is written
	for (uint32_t n : { 1u, 3u, 257u }) {
		for (uint32_t at : { 0u, n / 2u, n - 1u }) {
			for (int kind = 0; kind < 4; ++kind) {
				W.clear();
				for (uint32_t k = 0; k < n; ++k)
					add(1, 1, 1, 0, uniform(), uniform(), uniform());
				float *bad = W.data() + 12u * at;
				if (kind == 0)
					bad[6] = nan;
				else if (kind == 1)
					bad[3] = inf;
				else if (kind == 2)
					bad[8] = bad[0] + bad[4], bad[9] = bad[1] + bad[5], bad[10] = bad[2] + bad[6];  // row 2 = row 0 + row 1
				else
					for (int j = 0; j < 12; ++j)
						bad[j] = (j % 5 == 0) ? 1.0e-39f : 0.0f;  // (the inverse's entries exceed binary32)
				std::vector<float> O((size_t) n * 12u, 7.0f), bounds((size_t) n * 4u, 7.0f);
				std::vector<Node> nodes(2u * (size_t) n - 1u);
				std::memset(nodes.data(), 0x5A, nodes.size() * sizeof(Node));
				const std::vector<float> O_before = O, bounds_before = bounds;
				const std::vector<Node> nodes_before = nodes;
				expect(rt_instance_plan_lbvh(lo, hi, W.data(), n, O.data(), nodes.data(), bounds.data()) == RT_E_INVALID, "a refusal");
				expect(O == O_before && bounds == bounds_before && std::memcmp(nodes.data(), nodes_before.data(), nodes.size() * sizeof(Node)) == 0,
				       "a refusal wrote");
			}
		}
	}
	W.assign(identity, identity + 12);
	expect(rt_instance_plan_lbvh(lo, hi, W.data(), 0u, nullptr, nullptr, nullptr) == RT_E_INVALID, "no instances");
	expect(rt_instance_plan_lbvh(lo, hi, W.data(), RT_INSTANCES_MAX + 1u, nullptr, nullptr, nullptr) == RT_E_INVALID, "too many");
	expect(rt_instance_plan_lbvh(nullptr, hi, W.data(), 1u, nullptr, nullptr, nullptr) == RT_E_INVALID, "null box");
	expect(rt_instance_plan_lbvh(lo, hi, nullptr, 1u, nullptr, nullptr, nullptr) == RT_E_INVALID, "null transforms");
	if (failures)
		return 1;
	std::printf("INSTANCE_BUILD_SANITIZE_OK\n");
	return 0;
}
