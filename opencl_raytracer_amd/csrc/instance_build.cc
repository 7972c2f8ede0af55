// instance_build.cc -- a device-side instance build restated on the host (include/rt_hip_instance_build.h,
// rt_instance_plan_lbvh): the inverses, leaf boxes and bounds by instance_plan.h's functions, the keys, the shape and the
// layout by lbvh.h's -- the functions kernels/instance_build.hip.h runs with a lane per instance or node.  Host only.
#include <algorithm>
#include <cstring>
#include <numeric>

#include "../../include/rt_hip_instance_build.h"
#include "instances.h"
#include "lbvh.h"

namespace ocrt {

void instance_lbvh_tree(const std::vector<InstanceNode> &leaves, std::vector<InstanceNode> &nodes) {
	const uint32_t n = (uint32_t) leaves.size();
	nodes.assign(n ? 2u * (size_t) n - 1u : 0u, InstanceNode{});
	if (n == 0)
		return;
	// the root box: per axis the minimum and maximum of the leaf boxes, by comparison
	float root_lo[3], root_hi[3];
	for (int k = 0; k < 3; ++k) {
		root_lo[k] = leaves[0].lo[k], root_hi[k] = leaves[0].hi[k];
		for (uint32_t i = 1; i < n; ++i) {
			root_lo[k] = leaves[i].lo[k] < root_lo[k] ? leaves[i].lo[k] : root_lo[k];
			root_hi[k] = root_hi[k] < leaves[i].hi[k] ? leaves[i].hi[k] : root_hi[k];
		}
	}
	std::vector<uint32_t> keys(n), order(n), sorted(n);
	for (uint32_t i = 0; i < n; ++i) {
		uint32_t cell[3];
		for (int k = 0; k < 3; ++k)
			cell[k] = lbvh_cell(lbvh_centre(leaves[i].lo[k], leaves[i].hi[k]), root_lo[k], root_hi[k]);
		keys[i] = lbvh_key(cell[0], cell[1], cell[2]);
	}
	std::iota(order.begin(), order.end(), 0u);
	std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
	for (uint32_t i = 0; i < n; ++i)
		sorted[i] = keys[order[i]];
	// shape and layout: every inner node's own search, parent links, the count of first-child turns (lbvh.h)
	const uint32_t inner = n - 1u;
	std::vector<uint32_t> first(inner), last(inner), inner_links(inner, LBVH_NONE), leaf_links(n, LBVH_NONE), inner_at(inner);
	for (uint32_t i = 0; i < inner; ++i) {
		uint32_t split;
		lbvh_node(sorted.data(), n, i, &first[i], &last[i], &split);
		(first[i] == split ? leaf_links : inner_links)[split] = i | LBVH_FIRST;
		(last[i] == split + 1u ? leaf_links : inner_links)[split + 1u] = i;
	}
	if (inner)
		inner_links[0] = LBVH_NONE;
	for (uint32_t i = 0; i < inner; ++i) {
		inner_at[i] = 2u * first[i] + lbvh_first_child_turns(inner_links.data(), inner, inner_links[i]);
		InstanceNode &node = nodes.at(inner_at[i]);
		node.skip = 2u * (last[i] - first[i] + 1u) - 1u;
		node.leaf = INSTANCE_INNER;
	}
	for (uint32_t i = 0; i < n; ++i) {
		const uint32_t at = 2u * i + lbvh_first_child_turns(inner_links.data(), inner, leaf_links[i]);
		nodes.at(at) = leaves[order[i]];
		nodes[at].skip = 1u;
		nodes[at].leaf = order[i];
	}
	// inner boxes, children before parents (pre-order backwards): the exact minimum / maximum of the two children, the first
	// child's value where they compare equal
	for (size_t at = nodes.size(); at-- > 0;) {
		InstanceNode &node = nodes[at];
		if (node.skip == 1u)
			continue;
		const InstanceNode &a = nodes.at(at + 1u), &b = nodes.at(at + 1u + a.skip);
		for (int k = 0; k < 3; ++k) {
			node.lo[k] = b.lo[k] < a.lo[k] ? b.lo[k] : a.lo[k];
			node.hi[k] = a.hi[k] < b.hi[k] ? b.hi[k] : a.hi[k];
		}
	}
}

}  // namespace ocrt

extern "C" int rt_instance_plan_lbvh(const float root_lo[3], const float root_hi[3], const float *world_from_object, uint32_t n, float *O_out,
                                     void *nodes_out, float *bounds_out) {
	if (!root_lo || !root_hi || !world_from_object || n == 0u || n > RT_INSTANCES_MAX)
		return RT_E_INVALID;
	try {
		std::vector<float> O;
		if (!ocrt::instance_inverses(world_from_object, n, O))
			return RT_E_INVALID;
		if (nodes_out) {
			std::vector<ocrt::InstanceNode> leaves, nodes;
			ocrt::instance_leaves(root_lo, root_hi, world_from_object, O.data(), n, leaves);
			ocrt::instance_lbvh_tree(leaves, nodes);
			std::memcpy(nodes_out, nodes.data(), nodes.size() * sizeof(ocrt::InstanceNode));
		}
		if (bounds_out) {
			std::vector<float> bounds;
			ocrt::instance_bounds(root_lo, root_hi, world_from_object, O.data(), n, bounds);
			std::copy(bounds.begin(), bounds.end(), bounds_out);
		}
		if (O_out)
			std::copy(O.begin(), O.end(), O_out);
		return RT_OK;
	} catch (...) {
		return RT_E_INVALID;
	}
}
