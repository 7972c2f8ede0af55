// kernels/instance_directional.hip.h -- directional occlusion against the posed copies of an instance set: which of a
// world-space point's ambient-occlusion rays were blocked (include/rt_hip_instance_directional.h)
// (part of the one translation unit kernels.hip; see its head for the passes and the arithmetic contract)
//
// instance_ao_mask_kernel<MODE>: ao_mask_kernel's packet and rays (ao_mask_ray: ao_point / ao_direction, nothing of which
// involves the set), the nested walk in its occlusion form with instance_tri_eval at the leaf (kernels/instances.hip.h has
// the walk and its rules), and ao_mask_kernel's tail (ao_mask_flags: ballot, at most one vector atomic per (packet, point,
// mask word), none where nothing was hit).  What is made of the rows -- count, value, the ordered sum of the open rays'
// directions -- is ao_directional_finish_kernel's, as it is: the directions are the plain query's.
#pragma once
#include "directional.hip.h"
#include "instances.hip.h"

namespace ocrt {

struct InstanceAoMaskArgs : AoMaskArgs {  // (nodes_ptr, tris_ptr, node_count: the scene's own; max_distance: in both spaces)
	InstanceSet set;
};

template <int MODE>
__global__ __launch_bounds__(64 * QUERY_WAVES) void instance_ao_mask_kernel(InstanceAoMaskArgs a) {
	const uint32_t r = blockIdx.x * (64u * QUERY_WAVES) + threadIdx.x;
	bool live;
	uint32_t idx, k;
	const Ray ray = ao_mask_ray<MODE>(a, r, live, idx, k);
	const bool hit = instance_walk<false>(a.set, a.nodes_ptr, a.node_count, a.tris_ptr, ray, a.max_distance, live, InstanceTriEval{}, NoCandidate{});
	ao_mask_flags(a, live, idx, k, hit);
}

}  // namespace ocrt
