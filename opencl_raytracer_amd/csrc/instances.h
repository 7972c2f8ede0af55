// instances.h -- the planner of an instance set (include/rt_hip_instances.h): from the scene's root box and the caller's
// transforms to the inverses the kernel uses and the top-level tree it walks.  Host only; no HIP headers, so that the CPU
// tests and a stand-alone sanitizer program take it without a device (rt_instance_plan, defined in instances.cc).
#pragma once
#include <cstdint>
#include <vector>

#include "instance_plan.h"

namespace ocrt {

// The record the exact walk reads (device_types.h, NodeRec): `skip` the subtree's size, `leaf` the instance or INSTANCE_INNER.
struct InstanceNode {
	float lo[3];
	uint32_t skip;
	float hi[3];
	uint32_t leaf;
};
static_assert(sizeof(InstanceNode) == 32, "InstanceNode is NodeRec");
constexpr uint32_t INSTANCE_INNER = 0xFFFFFFFFu;

// (instance_inverse -- object_from_world of one transform by the header's formula -- and the rest of one instance's
// arithmetic: instance_plan.h, included above)
// Every transform of the set, or none: false, and `O` untouched, where one is refused.  O: n * 12 floats.
bool instance_inverses(const float *W, uint32_t n, std::vector<float> &O);
// What the instanced closest-point walk holds a copy's object-space boxes against (instance_nearest.h, inp_bounds: scale,
// per_q, fixed, world), four floats per instance, from the transforms, their binary32 inverses and the scene's root box; made
// in binary64 and rounded in the safe direction.  A root box that is not finite gives scale 0: nothing is passed by.
void instance_bounds(const float root_lo[3], const float root_hi[3], const float *W, const float *O, uint32_t n, std::vector<float> &bounds);
// The tree over n >= 1 accepted transforms and their inverses: 2n - 1 records in pre-order.
void instance_tree(const float root_lo[3], const float root_hi[3], const float *W, const float *O, uint32_t n, std::vector<InstanceNode> &nodes);
// The leaf records of that tree alone, by instance index (skip 1, leaf k): the boxes both trees are made over.
void instance_leaves(const float root_lo[3], const float root_hi[3], const float *W, const float *O, uint32_t n, std::vector<InstanceNode> &leaves);
// What a device-side instance build makes (include/rt_hip_instance_build.h; instance_build.cc), restated on the host: the
// radix tree of lbvh.h over the leaves' keys, 2n - 1 records in pre-order, from leaf records by instance index.
void instance_lbvh_tree(const std::vector<InstanceNode> &leaves, std::vector<InstanceNode> &nodes);

}  // namespace ocrt
