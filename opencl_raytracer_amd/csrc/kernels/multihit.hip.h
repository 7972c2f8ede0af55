// kernels/multihit.hip.h -- multi-hit ray queries: the number of triangles a ray's walk accepts and the first K of them
// (include/rt_hip_multihit.h)
// (part of the one translation unit kernels.hip; see its head for the passes and the arithmetic contract)
//
// The reference's scene_intersect (src/intersect_kernel.cl:184-213) does not prune on the running nearest distance: it
// tests every leaf whose chain of boxes passes aabb_intersect with the call's max_distance.  The triangles it accepts
// for a ray are therefore a set that depends on the scene arrays, the ray and max_distance alone -- not on the order of
// the walk.  multihit_walk_kernel<K> is query_kernel<true>'s walk (the exact form of the shared walk, query.hip.h)
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

struct MultiHitArgs {
	const float4 *nodes_ptr;  // SceneBuffers::nodes: exact boxes, builder order (NodeRec)
	const float4 *tris_ptr;   // TriRec by leaf
	const float4 *shade;      // ShadeRec by leaf
	const float4 *origins, *directions;  // float4[n]
	const uint32_t *order;    // [n] ray of packet lane k, or null: ray k (walk)
	uint32_t n, node_count, k;
	float max_distance;
	uint2 *list;              // [n * k] scratch: the keys (distance bits, leaf) of ray i at i * k; unused: (+inf, NONE)
	// outputs; null: not written
	uint32_t *count;          // [n]
	float *distance;          // [n * k]
	uint32_t *leaf;           // [n * k]
	float *barycentric, *position, *normal;  // [3 * n * k]
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
	const uint32_t k = blockIdx.x * MULTIHIT_LANES + t;
	const bool live = k < a.n;  // (a partial last packet: its dead lanes walk nothing and write nothing)
	uint32_t idx = k;
	if (live && a.order)
		idx = a.order[k];
	float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f), d = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
	if (live) {
		o = a.origins[idx];
		d = a.directions[idx];
	}
	const Ray ray = make_ray(o.x, o.y, o.z, d.x, d.y, d.z);
	const float max_distance = a.max_distance;
	uint32_t accepted = 0u, filled = 0u;
	float bound_d = __builtin_inff();  // (+inf, NONE): every key precedes it
	uint32_t bound_leaf = NONE;
	// the exact form of the shared walk, as in query_kernel: one wave-uniform node index `at`, each lane's own walk in `mine`
	const uint32_t count = a.node_count;
	uint32_t mine = 0u, at = 0u;
	while (at < count) {
		const u32x8 node = scalar_load_node(a.nodes_ptr, at);
		const float4 lo = make_float4(__uint_as_float(node[0]), __uint_as_float(node[1]), __uint_as_float(node[2]), 0.0f);
		const float4 hi = make_float4(__uint_as_float(node[4]), __uint_as_float(node[5]), __uint_as_float(node[6]), 0.0f);
		const uint32_t skip = node[3], leaf = node[7];
		const bool box = exact_box(lo, hi, ray, max_distance, live, at, skip, mine);
		const unsigned long long hit_mask = wave_ballot(box);
		if (hit_mask != 0ull && leaf != NONE) {
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
		}
		at = (uint32_t) __builtin_amdgcn_readfirstlane((int) (at + (hit_mask != 0ull ? 1u : skip)));
	}
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
// normal as query_kernel computes it; a member whose distance is not below +inf keeps the entry values beside its own
// leaf index, and so does an unused slot beside the leaf 0xFFFFFFFF.
__global__ __launch_bounds__(256) void multihit_resolve_kernel(MultiHitArgs a) {
	const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
	const uint32_t total = a.n * a.k;  // (<= RT_QUERY_MAX_RAYS: checked at the boundary)
	if (slot >= total)
		return;
	const uint2 key = a.list[slot];
	const uint32_t leaf = key.y;
	const bool used = leaf != NONE;
	const bool wants_record = a.barycentric || a.position || a.normal;
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
	if (a.distance)
		a.distance[slot] = __uint_as_float(key.x);
	if (a.leaf)
		a.leaf[slot] = leaf;
	if (a.barycentric) {
		a.barycentric[3u * (size_t) slot + 0u] = b0;
		a.barycentric[3u * (size_t) slot + 1u] = b1;
		a.barycentric[3u * (size_t) slot + 2u] = b2;
	}
	if (a.position) {
		a.position[3u * (size_t) slot + 0u] = px;
		a.position[3u * (size_t) slot + 1u] = py;
		a.position[3u * (size_t) slot + 2u] = pz;
	}
	if (a.normal) {
		float nx = 0.0f, ny = 0.0f, nz = 0.0f;
		if (kept) {
			const float4 n0 = a.shade[3 * (size_t) leaf + 0];
			const float4 n1 = a.shade[3 * (size_t) leaf + 1];
			const float4 n2 = a.shade[3 * (size_t) leaf + 2];
			nx = (n0.x * b0 + n1.x * b1) + n2.x * b2;
			ny = (n0.y * b0 + n1.y * b1) + n2.y * b2;
			nz = (n0.z * b0 + n1.z * b1) + n2.z * b2;
			normalize3(nx, ny, nz);
		}
		a.normal[3u * (size_t) slot + 0u] = nx;
		a.normal[3u * (size_t) slot + 1u] = ny;
		a.normal[3u * (size_t) slot + 2u] = nz;
	}
}

}  // namespace ocrt
