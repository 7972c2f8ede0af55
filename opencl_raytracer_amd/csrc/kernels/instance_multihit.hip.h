// kernels/instance_multihit.hip.h -- instanced multi-hit ray queries: the number of (instance, triangle) pairs a world-space
// ray's nested walk accepts among the posed copies of an instance set, and the first K of them
// (include/rt_hip_instance_multihit.h)
// (part of the one translation unit kernels.hip; see its head for the passes and the arithmetic contract)
//
// The composition of kernels/multihit.hip.h and kernels/instances.hip.h.  Neither walk of instance_walk<true> prunes on a
// distance, so the candidates of a ray -- the pairs (instance entered through the top-level boxes, leaf the scene's own walk
// accepts for the object ray) -- are a set that depends on the scene arrays, the set, the ray and max_distance alone.
// instance_multihit_walk_kernel<K> is multihit_walk_kernel<K>'s shape around that walk: instance_tri_eval at the leaves, and
// a candidate step that forms the world position and distance as instance_candidate does, counts the member and keeps the K
// first by (reported distance, instance, leaf).  instance_multihit_resolve_kernel, one thread per (ray, slot), forms the
// object ray of the kept instance again -- the header's products and sums, from the same twelve floats --, runs
// instance_tri_eval on the kept leaf again (the same inputs: the same bits) and writes the whole record, the normal by
// instance_normal.
//
// The list of a lane: multihit_walk_kernel's, with a third lane-strided array for the instance -- slot j of lane l at word
// [j * 256 + l] of a distance, an instance and a leaf array, so the 32 lanes one LDS cycle serves fall on 32 different banks
// whatever slot each of them is at.  256 lanes x K slots x 12 bytes: 48 KiB per workgroup at K = 16 (3 workgroups per CU in
// 160 KiB), none at K <= 1, where the one key lives in registers.  The K-th key is held in registers as
// the bound: a candidate that does not precede it costs two comparisons and no LDS access.  No per-thread array, no scratch.
#pragma once
#include "instances.hip.h"
#include "multihit.hip.h"

namespace ocrt {

struct InstanceMultiHitArgs : RayQueryArgs {  // (`order`: the walk's; `out`: slot j of ray i at i * k + j)
	InstanceSet set;
	uint32_t k;
	uint32_t *list;      // [n * k * 3] scratch: the keys (distance bits, instance, leaf) of ray i at 3 * i * k; unused: (+inf, NONE, NONE)
	uint32_t *count;     // [n], or null: not written
	uint32_t *instance;  // [n * k], or null: not written
};

namespace {

// The order of the slots: reported distance ascending (never NaN), then instance, then leaf index ascending.
__device__ __forceinline__ bool instance_key_before(float d, uint32_t instance, uint32_t leaf, float than_d, uint32_t than_instance,
                                                    uint32_t than_leaf) {
	return d < than_d || (d == than_d && (instance < than_instance || (instance == than_instance && leaf < than_leaf)));
}

}  // namespace

// K: the slots kept per lane (a power of two >= the call's k; 0: the count alone, no list at all).
template <uint32_t K>
__global__ __launch_bounds__(64 * QUERY_WAVES) void instance_multihit_walk_kernel(InstanceMultiHitArgs a) {
	__shared__ float list_distance[K > 1u ? K * MULTIHIT_LANES : 1u];
	__shared__ uint32_t list_instance[K > 1u ? K * MULTIHIT_LANES : 1u];
	__shared__ uint32_t list_leaf[K > 1u ? K * MULTIHIT_LANES : 1u];
	const uint32_t t = threadIdx.x;
	bool live;
	uint32_t idx;
	const Ray ray = packet_ray(a, blockIdx.x * MULTIHIT_LANES + t, live, idx);
	uint32_t accepted = 0u, filled = 0u;
	float bound_d = __builtin_inff();  // (+inf, NONE, NONE): every key precedes it
	uint32_t bound_instance = NONE, bound_leaf = NONE;
	instance_walk<true>(a.set, a.nodes_ptr, a.node_count, a.tris_ptr, ray, a.max_distance, live, InstanceTriEval{},
	                    [&](uint32_t instance, uint32_t leaf, const TriResult &, float r) {
		                    ++accepted;
		                    if (K == 0u)
			                    return;
		                    // the candidate's record is the WORLD ray's (instance_candidate)
		                    const float px = ray.ox + r * ray.dx, py = ray.oy + r * ray.dy, pz = ray.oz + r * ray.dz;
		                    const float cd = reported_distance(length3(px - ray.ox, py - ray.oy, pz - ray.oz));
		                    if (!instance_key_before(cd, instance, leaf, bound_d, bound_instance, bound_leaf))
			                    return;
		                    if (K == 1u) {
			                    bound_d = cd;
			                    bound_instance = instance;
			                    bound_leaf = leaf;
			                    filled = 1u;
			                    return;
		                    }
		                    uint32_t j = filled < K ? filled : K - 1u;  // the slot that opens: the end of the list, or its last key's
		                    while (j > 0u) {
			                    const float pd = list_distance[(j - 1u) * MULTIHIT_LANES + t];
			                    const uint32_t pi = list_instance[(j - 1u) * MULTIHIT_LANES + t];
			                    const uint32_t pl = list_leaf[(j - 1u) * MULTIHIT_LANES + t];
			                    if (!instance_key_before(cd, instance, leaf, pd, pi, pl))
				                    break;
			                    list_distance[j * MULTIHIT_LANES + t] = pd;
			                    list_instance[j * MULTIHIT_LANES + t] = pi;
			                    list_leaf[j * MULTIHIT_LANES + t] = pl;
			                    --j;
		                    }
		                    list_distance[j * MULTIHIT_LANES + t] = cd;
		                    list_instance[j * MULTIHIT_LANES + t] = instance;
		                    list_leaf[j * MULTIHIT_LANES + t] = leaf;
		                    if (filled < K)
			                    ++filled;
		                    if (filled == K) {
			                    bound_d = list_distance[(K - 1u) * MULTIHIT_LANES + t];
			                    bound_instance = list_instance[(K - 1u) * MULTIHIT_LANES + t];
			                    bound_leaf = list_leaf[(K - 1u) * MULTIHIT_LANES + t];
		                    }
	                    });
	if (!live)
		return;
	if (a.count)
		a.count[idx] = accepted;
	if (K == 0u)
		return;
	// the first a.k keys of the lane (a.k <= K), the rest of the ray's slots unused
	uint32_t *mine_out = a.list + 3u * (size_t) idx * a.k;
	for (uint32_t j = 0; j < a.k; ++j) {
		uint32_t key_d = __float_as_uint(__builtin_inff()), key_instance = NONE, key_leaf = NONE;
		if (j < filled) {
			if (K == 1u) {
				key_d = __float_as_uint(bound_d);
				key_instance = bound_instance;
				key_leaf = bound_leaf;
			} else {
				key_d = __float_as_uint(list_distance[j * MULTIHIT_LANES + t]);
				key_instance = list_instance[j * MULTIHIT_LANES + t];
				key_leaf = list_leaf[j * MULTIHIT_LANES + t];
			}
		}
		mine_out[3u * j + 0u] = key_d;
		mine_out[3u * j + 1u] = key_instance;
		mine_out[3u * j + 2u] = key_leaf;
	}
}

// One thread per (ray, slot): the record of the slot's (instance, leaf) -- the object ray from the instance's rows, the
// triangle test by the function the walk ran on the same inputs (the same bits), position and barycentrics as
// instance_candidate and instance_record_store make them, the normal by instance_normal; a member whose distance is not
// below +inf keeps the entry values beside its own instance and leaf, and so does an unused slot beside 0xFFFFFFFF.
__global__ __launch_bounds__(256) void instance_multihit_resolve_kernel(InstanceMultiHitArgs a) {
	const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
	const uint32_t total = a.n * a.k;  // (<= RT_QUERY_MAX_RAYS: checked at the boundary)
	if (slot >= total)
		return;
	const uint32_t key_d = a.list[3u * (size_t) slot + 0u], instance = a.list[3u * (size_t) slot + 1u], leaf = a.list[3u * (size_t) slot + 2u];
	const bool used = leaf != NONE;
	const bool wants_record = a.out.barycentric || a.out.position || a.out.normal;
	bool kept = false;
	float b0 = 0.0f, b1 = 0.0f, b2 = 0.0f, px = 0.0f, py = 0.0f, pz = 0.0f;
	if (used && wants_record && __uint_as_float(key_d) < __builtin_inff()) {
		const uint32_t i = slot / a.k;
		const float4 o = a.origins[i], d = a.directions[i];
		const float4 *rows = a.set.inverses + 3u * (size_t) instance;
		const float4 m0 = rows[0], m1 = rows[1], m2 = rows[2];
		Ray object;
		object.ox = ((m0.x * o.x + m0.y * o.y) + m0.z * o.z) + m0.w;
		object.oy = ((m1.x * o.x + m1.y * o.y) + m1.z * o.z) + m1.w;
		object.oz = ((m2.x * o.x + m2.y * o.y) + m2.z * o.z) + m2.w;
		object.dx = (m0.x * d.x + m0.y * d.y) + m0.z * d.z;
		object.dy = (m1.x * d.x + m1.y * d.y) + m1.z * d.z;
		object.dz = (m2.x * d.x + m2.y * d.y) + m2.z * d.z;
		object.ix = object.iy = object.iz = 0.0f;  // (the triangle test reads no reciprocal)
		const float4 *tri = a.tris_ptr + LEAF_F4 * leaf + LEAF_TRI_F4;
		float r;
		const TriResult tr = instance_tri_eval(tri[0], tri[1], tri[2], tri[3], object, r);
		kept = true;
		b0 = 1.0f - tr.s - tr.t;
		b1 = tr.s;
		b2 = tr.t;
		px = o.x + r * d.x;
		py = o.y + r * d.y;
		pz = o.z + r * d.z;
	}
	if (a.out.distance)
		a.out.distance[slot] = __uint_as_float(key_d);
	if (a.out.leaf)
		a.out.leaf[slot] = leaf;
	if (a.instance)
		a.instance[slot] = instance;
	if (a.out.barycentric) {
		a.out.barycentric[3u * (size_t) slot + 0u] = b0;
		a.out.barycentric[3u * (size_t) slot + 1u] = b1;
		a.out.barycentric[3u * (size_t) slot + 2u] = b2;
	}
	if (a.out.position) {
		a.out.position[3u * (size_t) slot + 0u] = px;
		a.out.position[3u * (size_t) slot + 1u] = py;
		a.out.position[3u * (size_t) slot + 2u] = pz;
	}
	if (a.out.normal) {
		float wx = 0.0f, wy = 0.0f, wz = 0.0f;
		if (kept)
			instance_normal(a.shade, a.set.inverses, leaf, instance, b0, b1, b2, wx, wy, wz);
		a.out.normal[3u * (size_t) slot + 0u] = wx;
		a.out.normal[3u * (size_t) slot + 1u] = wy;
		a.out.normal[3u * (size_t) slot + 2u] = wz;
	}
}

}  // namespace ocrt
