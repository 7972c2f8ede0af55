// kernels/multihit.hip.h -- multi-hit ray queries: the number of triangles a ray's walk accepts and the first K of them
// (include/rt_hip_multihit.h), and what the instanced form (kernels/instance_multihit.hip.h) shares with them: the key of a
// slot and its order, a lane's list, the scratch list and the resolve pass
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
// The list of a lane (MultiHitList): K keys in ascending order, in LDS, lane-strided -- slot j of lane l at word
// [j * 256 + l] of a distance array, a leaf array and, where the keys carry one, an instance array, so the 32 lanes one LDS
// cycle serves (4-byte accesses: bank = word % 32) fall on 32 different banks whatever slot each of them is at.  256 lanes x
// K slots x 8 bytes: 32 KiB per workgroup at K = 16 (5 workgroups per CU in 160 KiB); x 12 bytes with the instance: 48 KiB
// (3 workgroups); none at K <= 1, where the one key lives in registers.  The K-th key is also held in registers (`bound`:
// until the list is full, a key every candidate precedes): a candidate that does not precede it -- the common case once
// the list is full -- costs its comparisons and no LDS access.  The insertion shifts the keys behind the candidate's
// place up by one slot, addressed in LDS by a loop counter: no per-thread array, no scratch.
#pragma once
#include "query.hip.h"

namespace ocrt {

struct MultiHitArgs : RayQueryArgs {  // (`order`: the walk's; `out`: slot j of ray i at i * k + j)
	uint32_t k;
	uint32_t *list;   // scratch: the key of slot j of ray i at slot i * k + j (multihit_scratch_store); unused: (+inf, NONE, NONE)
	uint32_t *count;  // [n], or null: not written
};

constexpr uint32_t MULTIHIT_MAX_K = 16u;  // include/rt_hip_multihit.h: RT_MULTIHIT_MAX_K
constexpr uint32_t MULTIHIT_LANES = 64u * QUERY_WAVES;

// The key of a slot; the plain form's keys carry no instance (the field is not read).
struct MultiHitKey {
	float distance;
	uint32_t instance, leaf;
};

namespace {

// The order of the slots: reported distance ascending (never NaN), then -- INSTANCED -- instance, then leaf index ascending.
template <bool INSTANCED>
__device__ __forceinline__ bool key_before(const MultiHitKey &key, const MultiHitKey &than) {
	const bool lower = INSTANCED ? key.instance < than.instance || (key.instance == than.instance && key.leaf < than.leaf) : key.leaf < than.leaf;
	return key.distance < than.distance || (key.distance == than.distance && lower);
}

// What a member of the accepted set reports as its distance: the record's, which triangle_intersect replaces only where
// the computed distance is below the +inf it holds on entry (`rec->distance > distance`, false for +inf and NaN).
__device__ __forceinline__ float reported_distance(float computed) { return computed < __builtin_inff() ? computed : __builtin_inff(); }

// The scratch list between the two passes: a uint2 (distance bits, leaf) per slot, or -- INSTANCED -- three words
// (distance bits, instance, leaf).
template <bool INSTANCED>
__device__ __forceinline__ void multihit_scratch_store(uint32_t *list, size_t slot, const MultiHitKey &key) {
	if (INSTANCED) {
		list[3u * slot + 0u] = __float_as_uint(key.distance);
		list[3u * slot + 1u] = key.instance;
		list[3u * slot + 2u] = key.leaf;
	} else {
		((uint2 *) list)[slot] = make_uint2(__float_as_uint(key.distance), key.leaf);
	}
}
template <bool INSTANCED>
__device__ __forceinline__ MultiHitKey multihit_scratch_load(const uint32_t *list, size_t slot) {
	if (INSTANCED)
		return MultiHitKey{__uint_as_float(list[3u * slot + 0u]), list[3u * slot + 1u], list[3u * slot + 2u]};
	const uint2 key = ((const uint2 *) list)[slot];
	return MultiHitKey{__uint_as_float(key.x), NONE, key.y};
}

}  // namespace

// One lane's list: the K first keys offered so far, ascending.  K: a power of two >= the call's k (0: no list at all);
// the arrays: the kernel's __shared__ ones, K * MULTIHIT_LANES words each (`instance`: null unless INSTANCED; none is
// touched at K <= 1).
template <uint32_t K, bool INSTANCED>
struct MultiHitList {
	float *distance;
	uint32_t *instance, *leaf;
	uint32_t lane;
	uint32_t filled = 0u;
	MultiHitKey bound = MultiHitKey{__builtin_inff(), NONE, NONE};  // the K-th key; until there is one, a key every candidate precedes

	__device__ __forceinline__ uint32_t word(uint32_t j) const { return j * MULTIHIT_LANES + lane; }  // slot j's, in each array
	__device__ __forceinline__ MultiHitKey get(uint32_t w) const { return MultiHitKey{distance[w], INSTANCED ? instance[w] : NONE, leaf[w]}; }
	__device__ __forceinline__ void put(uint32_t w, const MultiHitKey &key) {
		distance[w] = key.distance;
		if (INSTANCED)
			instance[w] = key.instance;
		leaf[w] = key.leaf;
	}

	__device__ __forceinline__ void offer(const MultiHitKey &key) {
		if (K == 0u || !key_before<INSTANCED>(key, bound))
			return;
		if (K == 1u) {
			bound = key;
			filled = 1u;
			return;
		}
		uint32_t j = filled < K ? filled : K - 1u;  // the slot that opens: the end of the list, or its last key's
		while (j > 0u) {
			const uint32_t at = word(j);
			const MultiHitKey previous = get(at - MULTIHIT_LANES);
			if (!key_before<INSTANCED>(key, previous))
				break;
			put(at, previous);
			--j;
		}
		put(word(j), key);
		if (filled < K)
			++filled;
		if (filled == K)
			bound = get(word(K - 1u));
	}

	// Slot j as the scratch list gets it: the j-th key, or the unused slot's (+inf, NONE, NONE).
	__device__ __forceinline__ MultiHitKey key(uint32_t j) const {
		MultiHitKey key{__builtin_inff(), NONE, NONE};
		if (j < filled)
			key = K == 1u ? bound : get(word(j));
		return key;
	}
};

// The walk kernels' tail: the count, and the first a.k keys of the lane (a.k <= K), the rest of the ray's slots unused.
template <uint32_t K, bool INSTANCED>
__device__ __forceinline__ void multihit_walk_store(const MultiHitArgs &a, uint32_t idx, uint32_t accepted, const MultiHitList<K, INSTANCED> &list) {
	if (a.count)
		a.count[idx] = accepted;
	if (K == 0u)
		return;
	uint32_t *mine = a.list + (INSTANCED ? 3u : 2u) * (size_t) idx * a.k;
	for (uint32_t j = 0; j < a.k; ++j)
		multihit_scratch_store<INSTANCED>(mine, j, list.key(j));
}

// K: the slots kept per lane (a power of two >= the call's k; 0: the count alone, no list at all).
template <uint32_t K>
__global__ __launch_bounds__(64 * QUERY_WAVES) void multihit_walk_kernel(MultiHitArgs a) {
	__shared__ float list_distance[K > 1u ? K * MULTIHIT_LANES : 1u];
	__shared__ uint32_t list_leaf[K > 1u ? K * MULTIHIT_LANES : 1u];
	bool live;
	uint32_t idx;
	const Ray ray = packet_ray(a, blockIdx.x * MULTIHIT_LANES + threadIdx.x, live, idx);
	uint32_t accepted = 0u;
	MultiHitList<K, false> list{list_distance, nullptr, list_leaf, threadIdx.x};
	exact_walk(a.nodes_ptr, a.node_count, ray, a.max_distance, live, [&](uint32_t leaf, bool box) {
		const float4 *tri = a.tris_ptr + LEAF_F4 * leaf + LEAF_TRI_F4;
		const float4 q0 = tri[0], q1 = tri[1], q2 = tri[2], q3 = tri[3];
		if (box) {
			const TriResult tr = tri_eval<(K > 0u)>(q0, q1, q2, q3, ray);
			if (tr.accepted) {
				++accepted;
				if (K > 0u)
					list.offer(MultiHitKey{reported_distance(tr.distance), NONE, leaf});
			}
		}
		return false;  // (no lane ever leaves: the reference walks on)
	});
	if (live)
		multihit_walk_store(a, idx, accepted, list);
}

// The resolve kernels' body, one thread per (ray, slot): the slot's key, its record where one is asked for and the key
// has a distance below +inf -- record(o, d, key): the triangle test on the kept leaf again, by the function the walk ran
// on the same inputs (the same bits), its s, t and position --, and the stores.  A member whose distance is not below
// +inf keeps the entry values (distance +inf, the other fields 0) beside its own leaf (and instance), and so does an
// unused slot beside 0xFFFFFFFF.  normal(key, b0, b1, b2, nx, ny, nz): the record's, called for kept records only.
template <bool INSTANCED, class Record, class Normal>
__device__ __forceinline__ void multihit_resolve(const MultiHitArgs &a, uint32_t *instance, Record &&record, Normal &&normal) {
	const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
	const uint32_t total = a.n * a.k;  // (<= RT_QUERY_MAX_RAYS: checked at the boundary)
	if (slot >= total)
		return;
	const MultiHitKey key = multihit_scratch_load<INSTANCED>(a.list, slot);
	const bool used = key.leaf != NONE;
	const bool wants_record = a.out.barycentric || a.out.position || a.out.normal;
	bool kept = false;
	float b0 = 0.0f, b1 = 0.0f, b2 = 0.0f, px = 0.0f, py = 0.0f, pz = 0.0f;
	if (used && wants_record && key.distance < __builtin_inff()) {
		const uint32_t i = slot / a.k;
		const TriResult tr = record(a.origins[i], a.directions[i], key);
		kept = true;
		b0 = 1.0f - tr.s - tr.t;
		b1 = tr.s;
		b2 = tr.t;
		px = tr.px; py = tr.py; pz = tr.pz;
	}
	if (a.out.distance)
		a.out.distance[slot] = key.distance;
	if (a.out.leaf)
		a.out.leaf[slot] = key.leaf;
	if (INSTANCED && instance)
		instance[slot] = key.instance;
	store_record(a.out, slot, kept, b0, b1, b2, px, py, pz, [&](float &nx, float &ny, float &nz) { normal(key, b0, b1, b2, nx, ny, nz); });
}

// The record: triangle_intersect on a record with distance = INFINITY and the other fields 0 on entry, and its smooth normal.
__global__ __launch_bounds__(256) void multihit_resolve_kernel(MultiHitArgs a) {
	multihit_resolve<false>(
	    a, nullptr,
	    [&](const float4 o, const float4 d, const MultiHitKey &key) {
		    const float4 *tri = a.tris_ptr + LEAF_F4 * key.leaf + LEAF_TRI_F4;
		    return tri_eval<true>(tri[0], tri[1], tri[2], tri[3], make_ray(o.x, o.y, o.z, d.x, d.y, d.z));
	    },
	    [&](const MultiHitKey &key, float b0, float b1, float b2, float &nx, float &ny, float &nz) {
		    smooth_normal(a.shade, key.leaf, b0, b1, b2, nx, ny, nz);
	    });
}

}  // namespace ocrt
