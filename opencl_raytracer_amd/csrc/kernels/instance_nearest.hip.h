// kernels/instance_nearest.hip.h -- instanced closest-point queries: the nearest point of the surface among the posed copies
// of the uploaded scene, in world space (include/rt_hip_instance_nearest.h; the arithmetic is instance_nearest.h's and
// nearest_point.h's, the files the tests' oracle compiles)
// (part of the one translation unit kernels.hip; see its head for the passes and the arithmetic contract)
//
// The answer is the minimum of (d2, instance, leaf) over ALL pairs of a copy and a leaf, each pair's d2 np_nearest's for the
// copy's WORLD triangle: a distance does not survive an affine map, so -- unlike instance_walk's rays -- nothing can be
// measured in a copy's object space.  Only the LOOKING is done there: the walk holds the object-space point q' = O q against
// the scene's own boxes, and inp_object_limit2 (proof in instance_nearest.h) turns the lane's world reach into the object
// distance beyond which no triangle of a box can matter.  Nothing the walk does changes a bit of the answer.
//
// nearest_kernel's two parts, nested like instance_walk:
//   1. instance_nearest_descend: each lane goes down the top-level tree into the nearest child's box, then down that copy's
//      scene tree with its own q', and tests the one leaf it arrives at -- gathers, divergent, for a starting bound.
//   2. the shared walk: a wave-uniform top-level index, the record by one scalar load, np_box_d2 of q against the world box;
//      at a top-level leaf some lane needs, the rows of O and W and the copy's bounds arrive by scalar loads into SGPRs and
//      nearest_kernel's loop runs over the scene's records with q'.  At a scene leaf the lanes that need it form the world
//      triangle out of the SGPR rows and call np_nearest; a lane's reach falls as it finds nearer triangles, across copies.
// No stack, no LDS.  Scenes whose boxes promise nothing (NearestArgs::walk without NEAREST_PRUNE, or the coordinates flag: the
// top-level boxes are made from the scene's root box and promise no more than it does) are walked pair by pair.
#pragma once
#include "instances.hip.h"
#include "nearest.hip.h"

namespace ocrt {

struct InstanceNearestArgs : NearestArgs {  // (nodes_ptr, tris_ptr, shade, node_count, tri_count: the scene's own)
	InstanceSet set;
	const float4 *world;   // world_from_object as given, three float4 rows per instance
	const float4 *bounds;  // inp_bounds, one float4 per instance
	uint32_t *instance;    // by point index, or null
};

__device__ __forceinline__ inp_rows instance_rows(const float4 m0, const float4 m1, const float4 m2) {
	inp_rows r;
	r.m[0][0] = m0.x; r.m[0][1] = m0.y; r.m[0][2] = m0.z; r.m[0][3] = m0.w;
	r.m[1][0] = m1.x; r.m[1][1] = m1.y; r.m[1][2] = m1.z; r.m[1][3] = m1.w;
	r.m[2][0] = m2.x; r.m[2][1] = m2.y; r.m[2][2] = m2.z; r.m[2][3] = m2.w;
	return r;
}

// Instance k's bounds by one scalar load (scalar_load_rows' form).  `k` is wave-uniform.
__device__ __forceinline__ inp_bounds scalar_load_bounds(const float4 *bounds, uint32_t k) {
	u32x4s r;
	const uint32_t offset = (uint32_t) __builtin_amdgcn_readfirstlane((int) (k * 16u));
	asm volatile("s_load_dwordx4 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=&s"(r) : "s"(bounds), "s"(offset));
	inp_bounds b;
	b.scale = __uint_as_float(r[0]);
	b.per_q = __uint_as_float(r[1]);
	b.fixed = __uint_as_float(r[2]);
	b.world = __uint_as_float(r[3]);
	return b;
}

// Pair (instance, leaf) against the lane's record; returns whether it replaced it.
__device__ __forceinline__ bool instance_nearest_take(Nearest &best, uint32_t &best_instance, const inp_rows &world, const np_tri &object,
                                                      uint32_t instance, uint32_t leaf, float qx, float qy, float qz) {
	const np_point r = np_nearest(inp_world_tri(world, object), qx, qy, qz);
	if (!inp_better(r.d2, instance, leaf, best.d2, best_instance, best.leaf))
		return false;
	best.d2 = r.d2;
	best.leaf = leaf;
	best.s = r.s; best.t = r.t;
	best.px = r.px; best.py = r.py; best.pz = r.pz;
	best_instance = instance;
	return true;
}

// A lane's own way down one tree, nearest_descend's: at every inner node into the child whose box is nearest.  Returns the
// `leaf` word of the record it ends at, NONE where an inner node has no children.  Records by buffer loads (out of range
// reads 0, which ends the descent).
template <bool COUNT>
__device__ __forceinline__ uint32_t instance_nearest_down(__amdgpu_buffer_rsrc_t nodes, float qx, float qy, float qz, uint32_t &node_tests) {
	uint32_t at = 0u;
	float4 lo = load_f4(nodes, 0u), hi = load_f4(nodes, 16u);
	while (__float_as_uint(hi.w) == NONE) {
		const uint32_t end = at + __float_as_uint(lo.w);
		uint32_t c = at + 1u, pick = NONE;
		float pick_d2 = 0.0f;
		while (c < end) {
			const float4 clo = load_f4(nodes, c * 32u), chi = load_f4(nodes, c * 32u + 16u);
			const float d2 = np_box_d2(clo.x, clo.y, clo.z, chi.x, chi.y, chi.z, qx, qy, qz);
			if (COUNT)
				++node_tests;
			if (pick == NONE || d2 < pick_d2) {
				pick = c;
				pick_d2 = d2;
				lo = clo;
				hi = chi;
			}
			const uint32_t size = __float_as_uint(clo.w);
			c += size ? size : 1u;
		}
		if (pick == NONE)
			return NONE;
		at = pick;
	}
	return __float_as_uint(hi.w);
}

// Part 1: down the top-level tree with q, down that copy's scene tree with q', and the leaf it ends at.
template <bool COUNT>
__device__ __forceinline__ void instance_nearest_descend(const InstanceNearestArgs &a, float qx, float qy, float qz, bool active, Nearest &best,
                                                         uint32_t &best_instance, uint32_t &node_tests, uint32_t &tri_tests) {
	if (!active)
		return;
	const __amdgpu_buffer_rsrc_t top = __builtin_amdgcn_make_buffer_rsrc((void *) a.set.top_ptr, 0, (int) (a.set.top_count * 32u), 0x00020000);
	const uint32_t k = instance_nearest_down<COUNT>(top, qx, qy, qz, node_tests);
	if (k >= (a.set.top_count + 1u) / 2u)
		return;
	const float4 *o = a.set.inverses + 3u * (size_t) k, *w = a.world + 3u * (size_t) k;
	float ox, oy, oz;
	inp_object_point(instance_rows(o[0], o[1], o[2]), qx, qy, qz, &ox, &oy, &oz);
	const SceneViews scene = make_views(a.nodes_ptr, a.tris_ptr, a.node_count, a.tri_count);
	const uint32_t leaf = instance_nearest_down<COUNT>(scene.nodes, ox, oy, oz, node_tests);
	if (leaf >= a.tri_count)
		return;
	const uint32_t rec = leaf * LEAF_BYTES + LEAF_TRI_OFFSET;
	const float4 q0 = load_f4(scene.tris, rec), q1 = load_f4(scene.tris, rec + 16u), q2 = load_f4(scene.tris, rec + 32u),
	             q3 = load_f4(scene.tris, rec + 48u);
	if (COUNT)
		++tri_tests;
	(void) instance_nearest_take(best, best_instance, instance_rows(w[0], w[1], w[2]), nearest_tri(q0, q1, q2, q3), k, leaf, qx, qy, qz);
}

// COUNT: the counted form for tools/instance_distance_bench.py (rt_debug_set_nearest_walk); the product's host code never
// launches it.  (amdgpu_waves_per_eu: two trees' records, the rows of W and the bounds are SGPRs' work, and left to itself the
// compiler takes 102 of them -- 7 waves per SIMD.  Held to nearest_kernel's 8 it keeps 78 and parks 22 words the scene loop
// never touches -- output pointers, mostly -- in the lanes of one VGPR: four v_readlane per copy entered, none per record.)
template <bool COUNT>
__global__ __launch_bounds__(64 * NEAREST_WAVES) __attribute__((amdgpu_waves_per_eu(8, 8))) void instance_nearest_kernel(InstanceNearestArgs a) {
	const uint32_t lane = blockIdx.x * (64u * NEAREST_WAVES) + threadIdx.x;
	const bool live = lane < a.n;
	uint32_t idx = lane;
	if (live && a.order)
		idx = a.order[lane];
	float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	if (live)
		q = a.points[idx];
	const bool alive = live && np_point_ok(q.x, q.y, q.z) && np_radius_ok(a.max_distance);
	Nearest best;
	best.d2 = __builtin_inff();
	best.leaf = NONE;
	best.s = best.t = 0.0f;
	best.px = best.py = best.pz = 0.0f;
	uint32_t best_instance = NONE;
	uint32_t node_tests = 0u, tri_tests = 0u;
	const uint32_t walk = (a.coords_flag && *a.coords_flag != 0u) ? 0u : a.walk;  // (wave-uniform)
	const bool prune = (walk & NEAREST_PRUNE) != 0u && a.set.top_count != 0u;
	// the lane's reach in world space (inp_reach): +inf where nothing may be passed by
	float magnitude = 0.0f, reach = __builtin_inff(), radius_reach = __builtin_inff();
	const float q_max = fmaxf(fmaxf(fabsf(q.x), fabsf(q.y)), fabsf(q.z));
	if (prune) {
		const u32x8 root = scalar_load_node(a.set.top_ptr, 0u);
		magnitude = np_magnitude(__uint_as_float(root[0]), __uint_as_float(root[1]), __uint_as_float(root[2]), __uint_as_float(root[4]),
		                         __uint_as_float(root[5]), __uint_as_float(root[6]), q.x, q.y, q.z);
		radius_reach = inp_reach_of_distance(a.max_distance, magnitude);
		reach = radius_reach;
	}
	if ((walk & NEAREST_START) != 0u && prune && a.node_count != 0u) {
		instance_nearest_descend<COUNT>(a, q.x, q.y, q.z, alive, best, best_instance, node_tests, tri_tests);
		reach = fminf(radius_reach, inp_reach(best.d2, magnitude));
	}
	uint32_t top = 0u;
	while (top < a.set.top_count) {
		const u32x8 record = scalar_load_node(a.set.top_ptr, top);
		const uint32_t top_size = record[3], k = record[7];
		const float top_d2 = np_box_d2(__uint_as_float(record[0]), __uint_as_float(record[1]), __uint_as_float(record[2]),
		                               __uint_as_float(record[4]), __uint_as_float(record[5]), __uint_as_float(record[6]), q.x, q.y, q.z);
		const bool enter = alive && !np_prune(top_d2, reach * reach);
		const bool any_enter = wave_ballot(enter) != 0ull;
		if (COUNT && alive)
			++node_tests;
		if (any_enter && k != NONE) {
			// (k comes out of a scalar register: the rows and the bounds arrive by scalar loads, into SGPRs)
			float4 o0, o1, o2, w0, w1, w2;
			scalar_load_rows(a.set.inverses, k, o0, o1, o2);
			scalar_load_rows(a.world, k, w0, w1, w2);
			const inp_bounds bounds = scalar_load_bounds(a.bounds, k);
			const inp_rows world = instance_rows(w0, w1, w2);
			float ox, oy, oz;
			inp_object_point(instance_rows(o0, o1, o2), q.x, q.y, q.z, &ox, &oy, &oz);
			const float slack = inp_slack(bounds, q_max);
			float limit2 = inp_object_limit2(reach, bounds, slack);  // (+inf for a reach of +inf)
			uint32_t at = 0u;
			while (at < a.node_count) {
				const u32x8 node = scalar_load_node(a.nodes_ptr, at);
				const uint32_t size = node[3], leaf = node[7];
				const float box_d2 = np_box_d2(__uint_as_float(node[0]), __uint_as_float(node[1]), __uint_as_float(node[2]),
				                               __uint_as_float(node[4]), __uint_as_float(node[5]), __uint_as_float(node[6]), ox, oy, oz);
				const bool need = enter && !np_prune(box_d2, limit2);
				const bool any = wave_ballot(need) != 0ull;
				if (COUNT && alive)
					++node_tests;
				if (any && leaf != NONE) {
					const float4 *tri = a.tris_ptr + LEAF_F4 * leaf + LEAF_TRI_F4;
					const float4 q0 = tri[0], q1 = tri[1], q2 = tri[2], q3 = tri[3];
					if (need) {
						if (COUNT)
							++tri_tests;
						if (instance_nearest_take(best, best_instance, world, nearest_tri(q0, q1, q2, q3), k, leaf, q.x, q.y, q.z) && prune) {
							reach = fminf(radius_reach, inp_reach(best.d2, magnitude));
							limit2 = inp_object_limit2(reach, bounds, slack);
						}
					}
				}
				const uint32_t step = any ? 1u : (size ? size : 1u);
				at = (uint32_t) __builtin_amdgcn_readfirstlane((int) (at + step));
			}
		}
		const uint32_t top_step = any_enter ? 1u : (top_size ? top_size : 1u);
		top = (uint32_t) __builtin_amdgcn_readfirstlane((int) (top + top_step));
	}
	if (COUNT) {
		// (one atomic pair per wave: the lanes' counts summed across the wave first)
		unsigned long long nodes = node_tests, tris = tri_tests;
		for (int offset = 32; offset > 0; offset >>= 1) {
			nodes += __shfl_down(nodes, offset);
			tris += __shfl_down(tris, offset);
		}
		if ((threadIdx.x & 63u) == 0u) {
			atomicAdd(&a.counts[0], nodes);
			atomicAdd(&a.counts[1], tris);
		}
	}
	if (!live)
		return;
	const float distance = sqrtf(best.d2);
	const bool found = alive && best.d2 < __builtin_inff() && distance <= a.max_distance;
	if (a.hit)
		a.hit[idx] = found ? 1u : 0u;
	if (a.instance)
		a.instance[idx] = found ? best_instance : NONE;
	if (a.out.distance)
		a.out.distance[idx] = found ? distance : __builtin_inff();
	if (a.out.leaf)
		a.out.leaf[idx] = found ? best.leaf : NONE;
	instance_store_record(a.out, idx, a.shade, a.set.inverses, best.leaf, best_instance, found, found ? 1.0f - best.s - best.t : 0.0f,
	                      found ? best.s : 0.0f, found ? best.t : 0.0f, found ? best.px : 0.0f, found ? best.py : 0.0f, found ? best.pz : 0.0f);
}

}  // namespace ocrt
