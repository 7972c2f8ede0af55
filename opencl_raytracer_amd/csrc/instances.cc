// instances.cc -- the planner of an instance set (instances.h, include/rt_hip_instances.h).  Host only.  The arithmetic of
// one instance -- inverse, reach, margin, leaf box, bounds -- is instance_plan.h's, the text the device's planner runs too
// (kernels/instance_build.hip.h); this file has the loops over a set and the median-split tree.
#include "instances.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "../../include/rt_hip_instances.h"

namespace ocrt {

bool instance_inverses(const float *W, uint32_t n, std::vector<float> &O) {
	std::vector<float> made((size_t) n * 12u);
	for (uint32_t k = 0; k < n; ++k)
		if (!instance_inverse(W + 12u * (size_t) k, made.data() + 12u * (size_t) k))
			return false;
	O.swap(made);
	return true;
}

namespace {

// A box's centre on an axis as a sort key: a number whatever the box holds.
double centre_key(const InstanceNode &leaf, int axis) {
	const double c = 0.5 * (double) leaf.lo[axis] + 0.5 * (double) leaf.hi[axis];
	return std::isfinite(c) ? c : 0.0;
}

// The subtree over order[first, first + count) into nodes[at, at + 2 count - 1): a median split of the centres along
// their widest axis (equal centres: by instance index), the first child behind its parent, the second behind the first.
void split(const std::vector<InstanceNode> &leaves, std::vector<uint32_t> &order, uint32_t first, uint32_t count, std::vector<InstanceNode> &nodes,
           uint32_t at) {
	if (count == 1u) {
		nodes[at] = leaves[order[first]];
		return;
	}
	int axis = 0;
	double widest = -1.0;
	for (int k = 0; k < 3; ++k) {
		double lo = std::numeric_limits<double>::infinity(), hi = -lo;
		for (uint32_t i = first; i < first + count; ++i) {
			const double c = centre_key(leaves[order[i]], k);
			lo = std::min(lo, c);
			hi = std::max(hi, c);
		}
		if (hi - lo > widest)
			widest = hi - lo, axis = k;
	}
	const uint32_t half = count / 2u;
	std::nth_element(order.begin() + first, order.begin() + first + half, order.begin() + first + count, [&](uint32_t p, uint32_t q) {
		const double cp = centre_key(leaves[p], axis), cq = centre_key(leaves[q], axis);
		return cp < cq || (cp == cq && p < q);
	});
	const uint32_t left = at + 1u, right = at + 2u * half;
	split(leaves, order, first, half, nodes, left);
	split(leaves, order, first + half, count - half, nodes, right);
	InstanceNode &node = nodes[at];
	for (int k = 0; k < 3; ++k) {
		node.lo[k] = std::min(nodes[left].lo[k], nodes[right].lo[k]);
		node.hi[k] = std::max(nodes[left].hi[k], nodes[right].hi[k]);
	}
	node.skip = 2u * count - 1u;
	node.leaf = INSTANCE_INNER;
}

}  // namespace

void instance_bounds(const float root_lo[3], const float root_hi[3], const float *W, const float *O, uint32_t n, std::vector<float> &bounds) {
	bounds.assign((size_t) n * 4u, 0.0f);
	for (uint32_t k = 0; k < n; ++k)
		instance_bound(root_lo, root_hi, W + 12u * (size_t) k, O + 12u * (size_t) k, bounds.data() + 4u * (size_t) k);
}

void instance_leaves(const float root_lo[3], const float root_hi[3], const float *W, const float *O, uint32_t n, std::vector<InstanceNode> &leaves) {
	leaves.assign(n, InstanceNode{});
	double reach = 0.0;  // (of the whole set: the margin's G, instance_margin)
	for (uint32_t k = 0; k < n; ++k)
		reach = std::max(reach, instance_reach(root_lo, root_hi, W + 12u * (size_t) k));
	for (uint32_t k = 0; k < n; ++k) {
		instance_box(root_lo, root_hi, W + 12u * (size_t) k, O + 12u * (size_t) k, 4.0 * reach, leaves[k].lo, leaves[k].hi);
		leaves[k].skip = 1u;
		leaves[k].leaf = k;
	}
}

void instance_tree(const float root_lo[3], const float root_hi[3], const float *W, const float *O, uint32_t n, std::vector<InstanceNode> &nodes) {
	std::vector<InstanceNode> leaves;
	instance_leaves(root_lo, root_hi, W, O, n, leaves);
	std::vector<uint32_t> order(n);
	for (uint32_t k = 0; k < n; ++k)
		order[k] = k;
	nodes.assign(2u * (size_t) n - 1u, InstanceNode{});
	split(leaves, order, 0u, n, nodes, 0u);
}

}  // namespace ocrt

extern "C" int rt_instance_plan(const float root_lo[3], const float root_hi[3], const float *world_from_object, uint32_t n, float *O_out,
                                void *nodes_out) {
	if (!root_lo || !root_hi || !world_from_object || n == 0u || n > RT_INSTANCES_MAX)
		return RT_E_INVALID;
	try {
		std::vector<float> O;
		if (!ocrt::instance_inverses(world_from_object, n, O))
			return RT_E_INVALID;
		if (nodes_out) {
			std::vector<ocrt::InstanceNode> nodes;
			ocrt::instance_tree(root_lo, root_hi, world_from_object, O.data(), n, nodes);
			std::memcpy(nodes_out, nodes.data(), nodes.size() * sizeof(ocrt::InstanceNode));
		}
		if (O_out)
			std::copy(O.begin(), O.end(), O_out);
		return RT_OK;
	} catch (...) {
		return RT_E_INVALID;
	}
}
