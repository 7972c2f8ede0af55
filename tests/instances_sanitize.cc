// instances_sanitize.cc -- the planner of an instance set (csrc/instances.cc, rt_instance_plan) under the address and
// undefined-behaviour sanitizers: a stand-alone program, no device.  TEST INFRASTRUCTURE ONLY.
// Built and run by tests/test_instances_cpu.py: g++ -fsanitize=address,undefined instances_sanitize.cc csrc/instances.cc.
// It plans every family of transforms of tests/instance_cases.py in a simple form of its own, the instance counts of the
// tests, root boxes that are not finite, and the odd transforms, into buffers of exactly the documented sizes.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/rt_hip_instances.h"

namespace {

struct Node {
	float lo[3];
	uint32_t skip;
	float hi[3];
	uint32_t leaf;
};

uint32_t state = 12345u;
float uniform() {  // xorshift, [0, 1)
	state ^= state << 13;
	state ^= state >> 17;
	state ^= state << 5;
	return (float) (state >> 8) * (1.0f / 16777216.0f);
}

// Rows of [A | t]: a rotation about a drawn axis, scaled per axis, sheared, moved.
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

// Plans `W` into buffers of exactly 12 n floats and 2 n - 1 records and walks the tree once.
void plan(const float lo[3], const float hi[3], const std::vector<float> &W, const char *what) {
	const uint32_t n = (uint32_t) (W.size() / 12u);
	std::vector<float> O((size_t) n * 12u);
	std::vector<Node> nodes(2u * (size_t) n - 1u);
	expect(rt_instance_plan(lo, hi, W.data(), n, O.data(), nodes.data()) == RT_OK, what);
	std::vector<uint32_t> seen(n, 0u);
	for (size_t i = 0; i < nodes.size(); ++i) {
		expect(nodes[i].skip >= 1u && i + nodes[i].skip <= nodes.size(), "a skip leaves the array");
		if (nodes[i].leaf != 0xFFFFFFFFu) {
			expect(nodes[i].leaf < n && nodes[i].skip == 1u, "a leaf record");
			if (nodes[i].leaf < n)
				++seen[nodes[i].leaf];
		}
	}
	for (uint32_t k = 0; k < n; ++k)
		expect(seen[k] == 1u, "every instance once");
	expect(rt_instance_plan(lo, hi, W.data(), n, nullptr, nullptr) == RT_OK, "no outputs");
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
	W.clear();  // translations and rotations
	for (int k = 0; k < 6; ++k)
		add(1, 1, 1, 0, 0.8f * (float) k, -0.5f * (float) k, 4.0f * uniform());
	plan(lo, hi, W, "translations and rotations");
	W.clear();  // uniform scales in [1/4, 4]
	for (float s : { 0.25f, 0.5f, 1.0f, 2.0f, 4.0f })
		add(s, s, s, 0, uniform(), uniform(), uniform());
	plan(lo, hi, W, "scales");
	W.clear();  // non-uniform scale with shear, a mirror
	add(1, 2, 8, 0.5f, 1, 0, 0);
	add(0.5f, 1, 3, -0.25f, 0, 2, 0);
	add(-1, 1, 1, 0, 0, 0, 0);
	plan(lo, hi, W, "shear and mirror");
	W.clear();  // a pair of identical transforms, a pair half a box apart
	add(1, 1, 1, 0, 0.1f, 0.2f, 0.3f);
	W.insert(W.end(), W.begin(), W.begin() + 12);
	W.insert(W.end(), identity, identity + 12);
	W.insert(W.end(), identity, identity + 12);
	W[W.size() - 12u + 3u] = 0.35f;
	plan(lo, hi, W, "pairs");
	W.clear();  // a 5 x 5 x 5 grid
	for (int i = 0; i < 5; ++i)
		for (int j = 0; j < 5; ++j)
			for (int k = 0; k < 5; ++k)
				add(1, 1, 1, 0, 1.3f * (float) i, 1.3f * (float) j, 1.3f * (float) k);
	plan(lo, hi, W, "grid");
	for (uint32_t n : { 1u, 2u, 3u, 64u, 65u, 1000u }) {
		W.clear();
		for (uint32_t k = 0; k < n; ++k)
			add(0.5f + uniform(), 0.5f + uniform(), 0.5f + uniform(), 0, 20.0f * uniform(), 20.0f * uniform(), 20.0f * uniform());
		plan(lo, hi, W, "counts");
		const float broken[3] = { hi[0], n % 2u ? inf : nan, hi[2] };
		plan(lo, broken, W, "a root box that is not finite");
	}
	// every centre equal, huge and tiny coordinates
	W.clear();
	for (int k = 0; k < 33; ++k)
		W.insert(W.end(), identity, identity + 12);
	plan(lo, hi, W, "equal centres");
	W[3] = 3.0e38f;
	W[12 + 7] = -3.0e38f;
	W[24 + 0] = 1.0e-30f;
	plan(lo, hi, W, "huge and tiny");
	// the odd transforms: refused, and the outputs untouched
	W.assign(identity, identity + 12);
	W.insert(W.end(), identity, identity + 12);
	std::vector<float> O(24, 7.0f), before;
	std::vector<Node> nodes(3);
	std::memset(nodes.data(), 0x5A, nodes.size() * sizeof(Node));
	const std::vector<Node> nodes_before = nodes;
	before = O;
	auto refused = [&](const char *what) {
		expect(rt_instance_plan(lo, hi, W.data(), 2u, O.data(), nodes.data()) == RT_E_INVALID, what);
		expect(O == before && std::memcmp(nodes.data(), nodes_before.data(), nodes.size() * sizeof(Node)) == 0, "a refusal wrote");
	};
	W[12 + 5] = nan;
	refused("a NaN entry");
	W[12 + 5] = 1.0f;
	W[12 + 3] = inf;
	refused("an infinite entry");
	W[12 + 3] = 0.0f;
	W[12 + 0] = W[12 + 5] = W[12 + 10] = 0.0f;
	refused("a singular A");
	W[12 + 0] = 1.0f;
	W[12 + 5] = 1.0f;
	W[12 + 8] = 1.0f;
	W[12 + 9] = 1.0f;  // row 2 = row 0 + row 1
	refused("a rank-2 A");
	W.assign(identity, identity + 12);
	expect(rt_instance_plan(lo, hi, W.data(), 0u, nullptr, nullptr) == RT_E_INVALID, "no instances");
	expect(rt_instance_plan(lo, hi, W.data(), RT_INSTANCES_MAX + 1u, nullptr, nullptr) == RT_E_INVALID, "too many");
	expect(rt_instance_plan(nullptr, hi, W.data(), 1u, nullptr, nullptr) == RT_E_INVALID, "null box");
	expect(rt_instance_plan(lo, hi, nullptr, 1u, nullptr, nullptr) == RT_E_INVALID, "null transforms");
	if (failures)
		return 1;
	std::printf("INSTANCES_SANITIZE_OK\n");
	return 0;
}
