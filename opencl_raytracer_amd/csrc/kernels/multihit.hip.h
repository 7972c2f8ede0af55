// kernels/multihit.hip.h -- multi-hit ray queries: the number of triangles a ray's walk accepts and the first K of them
// (include/rt_hip_multihit.h)
// (part of the one translation unit kernels.hip; see its head for the passes and the arithmetic contract)
//
// The reference's scene_intersect (src/intersect_kernel.cl:184-213) does not prune on the running nearest distance: it
// tests every leaf whose chain of boxes passes aabb_intersect with the call's max_distance.  The triangles it accepts
// for a ray are therefore a set that depends on the scene arrays, the ray and max_distance alone -- not on the order of
// the walk.  multihit_walk_kernel<K> is the exact form of the shared walk (walk.hip.h, exact_walk) with a leaf step
// that counts the members of that set and keeps the K first of them by (reported distance, leaf index);
// multihit_resolve_kernel, one thread per (ray, slot), runs the triangle test on each kept leaf again and writes the
// whole record.  The rays are ordered by query.hip.h's sort kernels, unchanged.
//
// The list of a lane: K keys (float distance, uint32 leaf) in ascending order, in LDS, lane-strided -- slot j of lane l
// at word [j * 256 + l] of a distance array and of a leaf array, so the 32 lanes one LDS cycle serves (4-byte accesses:
// bank = word % 32) fall on 32 different banks whatever slot each of them is at.  256 lanes x K slots x 8 bytes: 32 KiB
// per workgroup at K = 16 (5 workgroups per CU in 160 KiB), 2 KiB at K = 1.  The K-th key is also held in registers
// (`bound`: until the list is full, a key every candidate precedes): a candidate that does not precede it -- the common
// case once the list is full -- costs one comparison and no LDS access.  The insertion shifts the keys behind the
// candidate's place up by one slot, addressed in LDS by a loop counter: no per-thread array, no scratch.
#pragma once
#include "query.hip.h"

namespace ocrt {

struct MultiHitArgs : RayQueryArgs {  // (`order`: the walk's; `out`: slot j of ray i at i * k + j)
	uint32_t k;
	uint2 *list;      // [n * k] scratch: the keys (distance bits, leaf) of ray i at i * k; unused: (+inf, NONE)
	uint32_t *count;  // [n], or null: not written
};

constexpr uint32_t MULTIHIT_MAX_K = 16u;  // include/rt_hip_multihit.h: RT_MULTIHIT_MAX_K
constexpr uint32_t MULTIHIT_LANES = 64u * QUERY_WAVES;

namespace {

// The order of the slots: reported distance ascending (never NaN), then leaf index ascending.
__device__ __forceinline__ bool key_before(float d, uint32_t leaf, float than_d, uint32_t than_leaf) {
	return d < than_d || (d == than_d && leaf < than_leaf);
}

// What a member of the accepted set reports as its distance: the record's, which triangle_intersect replaces only where
// the computed distance is below the +inf it holds on entry (`rec->distance > distance`, false for +inf and NaN).
__device__ __forceinline__ float reported_distance(float computed) { return computed < __builtin_inff() ? computed : __builtin_inff(); }

}  // namespace

// K: the slots kept per lane (a power of two >= the call's k; 0: the count alone, no list at all).
template <uint32_t K>
__global__ __launch_bounds__(64 * QUERY_WAVES) void multihit_walk_kernel(MultiHitArgs a) {
	__shared__ float list_distance[K > 1u ? K * MULTIHIT_LANES : 1u];
	__shared__ uint32_t list_leaf[K > 1u ? K * MULTIHIT_LANES : 1u];
	const uint32_t t = threadIdx.x;
	bool live;
	uint32_t idx;
	const Ray ray = packet_ray(a, blockIdx.x * MULTIHIT_LANES + t, live, idx);
	uint32_t accepted = 0u, filled = 0u;
	float bound_d = __builtin_inff();  // (+inf, NONE): every key precedes it
	uint32_t bound_leaf = NONE;
	exact_walk(a.nodes_ptr, a.node_count, ray, a.max_distance, live, [&](uint32_t leaf, bool box) {
		const float4 *tri = a.tris_ptr + LEAF_F4 * leaf + LEAF_TRI_F4;
		const float4 q0 = tri[0], q1 = tri[1], q2 = tri[2], q3 = tri[3];
		if (box) {
			const TriResult tr = tri_eval<(K > 0u)>(q0, q1, q2, q3, ray);
			if (tr.accepted) {
				++accepted;
				if (K > 0u) {
					const float cd = reported_distance(tr.distance);
					if (key_before(cd, leaf, bound_d, bound_leaf)) {
						if (K == 1u) {
							bound_d = cd;
							bound_leaf = leaf;
							filled = 1u;
						} else {
							uint32_t j = filled < K ? filled : K - 1u;  // the slot that opens: the end of the list, or its last key's
							while (j > 0u) {
								const float pd = list_distance[(j - 1u) * MULTIHIT_LANES + t];
								const uint32_t pl = list_leaf[(j - 1u) * MULTIHIT_LANES + t];
								if (!key_before(cd, leaf, pd, pl))
									break;
								list_distance[j * MULTIHIT_LANES + t] = pd;
								list_leaf[j * MULTIHIT_LANES + t] = pl;
								--j;
							}
							list_distance[j * MULTIHIT_LANES + t] = cd;
							list_leaf[j * MULTIHIT_LANES + t] = leaf;
							if (filled < K)
								++filled;
							if (filled == K) {
								bound_d = list_distance[(K - 1u) * MULTIHIT_LANES + t];
								bound_leaf = list_leaf[(K - 1u) * MULTIHIT_LANES + t];
							}
						}
					}
				}
			}
		}
		return false;  // (no lane ever leaves: the reference walks on)
	});
	if (!live)
		return;
	if (a.count)
		a.count[idx] = accepted;
	if (K == 0u)
		return;
	// the first a.k keys of the lane (a.k <= K), the rest of the ray's slots unused
	uint2 *mine_out = a.list + (size_t) idx * a.k;
	for (uint32_t j = 0; j < a.k; ++j) {
		uint2 key = make_uint2(__float_as_uint(__builtin_inff()), NONE);
		if (j < filled) {
			if (K == 1u)
				key = make_uint2(__float_as_uint(bound_d), bound_leaf);
			else
				key = make_uint2(__float_as_uint(list_distance[j * MULTIHIT_LANES + t]), list_leaf[j * MULTIHIT_LANES + t]);
		}
		mine_out[j] = key;
	}
}

// One thread per (ray, slot): the record of the slot's leaf -- triangle_intersect on a record with distance = INFINITY
// and the other fields 0 on entry, by the function the walk ran on the same inputs (the same bits) -- and its smooth
// normal (store_record, query.hip.h); a member whose distance is not below +inf keeps the entry values beside its own
// leaf index, and so does an unused slot beside the leaf 0xFFFFFFFF.
__global__ __launch_bounds__(256) void multihit_resolve_kernel(MultiHitArgs a) {
	const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
	const uint32_t total = a.n * a.k;  // (<= RT_QUERY_MAX_RAYS: checked at the boundary)
	if (slot >= total)
		return;
	const uint2 key = a.list[slot];
	const uint32_t leaf = key.y;
	const bool used = leaf != NONE;
	const bool wants_record = a.out.barycentric || a.out.position || a.out.normal;
	bool kept = false;
	float b0 = 0.0f, b1 = 0.0f, b2 = 0.0f, px = 0.0f, py = 0.0f, pz = 0.0f;
	if (used && wants_record && __uint_as_float(key.x) < __builtin_inff()) {
		const uint32_t i = slot / a.k;
		const float4 o = a.origins[i], d = a.directions[i];
		const Ray ray = make_ray(o.x, o.y, o.z, d.x, d.y, d.z);
		const float4 *tri = a.tris_ptr + LEAF_F4 * leaf + LEAF_TRI_F4;
		const TriResult tr = tri_eval<true>(tri[0], tri[1], tri[2], tri[3], ray);
		kept = true;
		b0 = 1.0f - tr.s - tr.t;
		b1 = tr.s;
		b2 = tr.t;
		px = tr.px; py = tr.py; pz = tr.pz;
	}
	if (a.out.distance)
		a.out.distance[slot] = __uint_as_float(key.x);
	if (a.out.leaf)
		a.out.leaf[slot] = leaf;
	store_record(a.out, slot, a.shade, leaf, kept, b0, b1, b2, px, py, pz);
}

}  // namespace ocrt
