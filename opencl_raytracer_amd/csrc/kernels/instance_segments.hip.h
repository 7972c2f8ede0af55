// kernels/instance_segments.hip.h -- instanced segment queries: is the straight line between two world-space points free of
// every posed copy of the scene, where is it blocked first, and the masks of many points against many targets
// (include/rt_hip_instance_segments.h)
// (part of the one translation unit kernels.hip; see its head for the passes and the arithmetic contract)
//
// A segment (a, b) is the WORLD ray o = a, d = b - a -- one subtraction per component, nothing normalised -- and an interval
// (t_lo, t_hi) of ray parameters.  An affine map keeps ray parameters, so the interval means the same in an instance's
// object space: the walk is instance_walk<CLOSEST> (kernels/instances.hip.h has it and its rules) with max_distance = t_hi
// in both walks, and the leaf step is segment_tri_eval<false> (kernels/segment.hip.h) on the OBJECT ray: the reference's
// triangle test with r > t_lo and r < t_hi on its plane parameter, whose early-out ballots save the two divisions once no
// lane of the packet is left in the interval.  (Not segment_tri_eval<true>: its distance would be the object ray's.)
//
// instance_segment_kernel<CLOSEST>: segment_kernel's packet (segment_packet_ray), the nested walk, and for CLOSEST
// instance_kernel's candidate and record (instance_candidate, instance_record_store).
// instance_visibility_kernel: visibility_mask_kernel's ray and tail (visibility_ray, visibility_mask_store) around the
// nested walk in its occlusion form.  The sort's kernels, visibility_count_kernel and the scan are the plain forms' own.
#pragma once
#include "instances.hip.h"
#include "segment.hip.h"

namespace ocrt {

// The leaf test of the segment forms: the interval on the object ray's plane parameter.
struct SegmentTriEval {
	float t_lo, t_hi;
	__device__ __forceinline__ TriResult operator()(const float4 q0, const float4 q1, const float4 q2, const float4 q3, const Ray &object,
	                                                float &r) const {
		return segment_tri_eval<false>(q0, q1, q2, q3, object, t_lo, t_hi, r);
	}
};

// ---- the pair forms ---------------------------------------------------------------------------------------------------
struct InstanceSegmentArgs : SegmentArgs {  // (nodes_ptr, tris_ptr, shade: the scene's own; t_lo, t_hi: in both spaces)
	InstanceSet set;
	uint32_t *instance;  // by segment index, or null (CLOSEST)
};

template <bool CLOSEST>
__global__ __launch_bounds__(64 * QUERY_WAVES) void instance_segment_kernel(InstanceSegmentArgs a) {
	bool live;
	uint32_t idx;
	const Ray ray = segment_packet_ray(a.from, a.to, a.order, a.n, blockIdx.x * (64u * QUERY_WAVES) + threadIdx.x, live, idx);
	Hit best = closest_entry();
	uint32_t best_instance = 0u;
	const bool hit = instance_walk<CLOSEST>(a.set, a.nodes_ptr, a.node_count, a.tris_ptr, ray, a.t_hi, live, SegmentTriEval{a.t_lo, a.t_hi},
	                                        [&](uint32_t k, uint32_t leaf, const TriResult &tr, float r) {
		                                        instance_candidate(ray, k, leaf, tr, r, best, best_instance);
	                                        });
	if (!live)
		return;
	if (a.hit)
		a.hit[idx] = hit ? 1u : 0u;
	if (CLOSEST)
		instance_record_store(a.out, a.instance, idx, a.shade, a.set.inverses, hit, best, best_instance);
}

// ---- the many-to-many form --------------------------------------------------------------------------------------------
struct InstanceVisibilityArgs : VisibilityArgs {  // (nodes_ptr, tris_ptr: the scene's own; points and targets in world space)
	InstanceSet set;
};

__global__ __launch_bounds__(64 * QUERY_WAVES) void instance_visibility_kernel(InstanceVisibilityArgs a) {
	bool live;
	uint32_t idx, j;
	const Ray ray = visibility_ray(a, blockIdx.x * (64u * QUERY_WAVES) + threadIdx.x, live, idx, j);
	const bool hit = instance_walk<false>(a.set, a.nodes_ptr, a.node_count, a.tris_ptr, ray, a.t_hi, live, SegmentTriEval{a.t_lo, a.t_hi},
	                                      NoCandidate{});
	visibility_mask_store(a, live, idx, j, hit);
}

}  // namespace ocrt
