// kernels/instance_multihit.hip.h -- instanced multi-hit ray queries: the number of (instance, triangle) pairs a world-space
// ray's nested walk accepts among the posed copies of an instance set, and the first K of them
// (include/rt_hip_instance_multihit.h)
// (part of the one translation unit kernels.hip; see its head for the passes and the arithmetic contract)
//
// The composition of kernels/multihit.hip.h and kernels/instances.hip.h.  Neither walk of instance_walk<true> prunes on a
// distance, so the candidates of a ray -- the pairs (instance entered through the top-level boxes, leaf the scene's own walk
// accepts for the object ray) -- are a set that depends on the scene arrays, the set, the ray and max_distance alone.
// instance_multihit_walk_kernel<K> is multihit_walk_kernel<K>'s shape around that walk: instance_tri_eval at the leaves, and
// a candidate step that forms the world position and distance as instance_candidate does, counts the member and offers the
// key (reported distance, instance, leaf) to the lane's list -- multihit.hip.h's MultiHitList with the instance array, which
// has the order of the slots, the insertion and the write-out.  instance_multihit_resolve_kernel is multihit.hip.h's
// resolve pass with the object ray of the kept instance formed again (instance_object_ray, from the same twelve floats),
// instance_tri_eval on the kept leaf (the same inputs: the same bits) and the normal by instance_normal.
#pragma once
#include "instances.hip.h"
#include "multihit.hip.h"

namespace ocrt {

struct InstanceMultiHitArgs : MultiHitArgs {  // (`list`: three words per slot)
	InstanceSet set;
	uint32_t *instance;  // [n * k], or null: not written
};

// K: the slots kept per lane (a power of two >= the call's k; 0: the count alone, no list at all).
template <uint32_t K>
__global__ __launch_bounds__(64 * QUERY_WAVES) void instance_multihit_walk_kernel(InstanceMultiHitArgs a) {
	__shared__ float list_distance[K > 1u ? K * MULTIHIT_LANES : 1u];
	__shared__ uint32_t list_instance[K > 1u ? K * MULTIHIT_LANES : 1u];
	__shared__ uint32_t list_leaf[K > 1u ? K * MULTIHIT_LANES : 1u];
	bool live;
	uint32_t idx;
	const Ray ray = packet_ray(a, blockIdx.x * MULTIHIT_LANES + threadIdx.x, live, idx);
	uint32_t accepted = 0u;
	MultiHitList<K, true> list{list_distance, list_instance, list_leaf, threadIdx.x};
	instance_walk<true>(a.set, a.nodes_ptr, a.node_count, a.tris_ptr, ray, a.max_distance, live, InstanceTriEval{},
	                    [&](uint32_t instance, uint32_t leaf, const TriResult &, float r) {
		                    ++accepted;
		                    if (K == 0u)
			                    return;
		                    // the candidate's record is the WORLD ray's (instance_candidate)
		                    const float px = ray.ox + r * ray.dx, py = ray.oy + r * ray.dy, pz = ray.oz + r * ray.dz;
		                    list.offer(MultiHitKey{reported_distance(length3(px - ray.ox, py - ray.oy, pz - ray.oz)), instance, leaf});
	                    });
	if (live)
		multihit_walk_store(a, idx, accepted, list);
}

// The record: position and barycentrics as instance_candidate and instance_record_store make them.
__global__ __launch_bounds__(256) void instance_multihit_resolve_kernel(InstanceMultiHitArgs a) {
	multihit_resolve<true>(
	    a, a.instance,
	    [&](const float4 o, const float4 d, const MultiHitKey &key) {
		    const float4 *rows = a.set.inverses + 3u * (size_t) key.instance;
		    Ray object;
		    instance_object_ray(rows[0], rows[1], rows[2], o.x, o.y, o.z, d.x, d.y, d.z, object.ox, object.oy, object.oz, object.dx, object.dy,
		                        object.dz);
		    object.ix = object.iy = object.iz = 0.0f;  // (the triangle test reads no reciprocal)
		    const float4 *tri = a.tris_ptr + LEAF_F4 * key.leaf + LEAF_TRI_F4;
		    float r;
		    TriResult tr = instance_tri_eval(tri[0], tri[1], tri[2], tri[3], object, r);
		    tr.px = o.x + r * d.x;
		    tr.py = o.y + r * d.y;
		    tr.pz = o.z + r * d.z;
		    return tr;
	    },
	    [&](const MultiHitKey &key, float b0, float b1, float b2, float &wx, float &wy, float &wz) {
		    instance_normal(a.shade, a.set.inverses, key.leaf, key.instance, b0, b1, b2, wx, wy, wz);
	    });
}

}  // namespace ocrt
