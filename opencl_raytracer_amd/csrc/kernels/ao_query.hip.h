// kernels/ao_query.hip.h -- ambient-occlusion queries: the reference's ambient_occlusion() at points the caller supplies
// (include/rt_hip_ao.h)
// (part of the one translation unit kernels.hip; see its head for the passes and the arithmetic contract)
//
// The rays of a call are the flattened list r = slot * rays_per_point + k: direction k of the point in slot `slot` (the
// point's own index, or -- sorted calls -- the entry of the counting sort's order, kernels/query.hip.h, keyed by point and
// normal).  ao_query_kernel<MODE> casts one packet of 64 CONSECUTIVE rays per wave: a run of directions from one point
// or from a few neighbouring ones, all within the AO reach of each other -- what the shared walk wants -- and no ray is
// ever read: every lane makes its own from its point, its normal and the direction table (UNIFORM) or the point's
// generator (RANDOM), with the arithmetic of the frame's own pass (reference src/intersect_kernel.cl:215-248 and
// :153-183): the tangent frame is tangent_frame (kernels/common.hip.h), the RANDOM sample random_sample (kernels/ao.hip.h).
//
// The walk is the EXACT form (walk.hip.h, exact_walk) over the uploaded scene's exact node records, any-hit:
// lane by lane the reference's scene_intersect whatever the point and the normal hold.  The padded records of the fast
// form are not used: their margins are proven for the frame's own hit points, not for points from anywhere.
//
// Counting: hits are integers, so the order of the additions is free.  Per packet the hit flags are balloted and the
// first lane of each point's run of lanes adds the run's popcount to count[point] -- one vector atomic per (packet, point),
// none where nothing was hit.  ao_query_finish_kernel then writes 1 - count / n per point.
#pragma once
#include "ao.hip.h"
#include "query.hip.h"

namespace ocrt {

struct AoQueryArgs {
	const float4 *nodes_ptr;  // SceneBuffers::nodes: exact boxes, builder order (NodeRec)
	const float4 *tris_ptr;   // TriRec by leaf
	const float4 *ao_table;   // float4[rays] (UNIFORM)
	const float4 *points, *normals;  // float4[n]
	const uint32_t *seeds;    // [n] the reference's `index` of a point (RANDOM), or null: the point's own index
	const uint32_t *order;    // [n] point of slot j, or null: point j
	uint32_t *count;          // [n] occluded rays by point index, zeroed before the launch
	uint32_t n, rays;         // points, rays per point
	uint32_t total;           // n * rays
	uint32_t node_count;
	float max_distance;
};

// Ray `r` of the flattened list, made in registers: direction r % rays of the point in slot r / rays (ao_query_kernel and
// its instanced form, kernels/instance_views.hip.h).  MODE is AO_UNIFORM or AO_RANDOM, as for ao_kernel: the sampler's code
// and registers stay out of the default path.
template <int MODE>
__device__ __forceinline__ Ray ao_query_ray(const AoQueryArgs &a, uint32_t r, bool &live, uint32_t &slot, uint32_t &idx) {
	live = r < a.total;  // (a partial last packet: its dead lanes walk nothing and count nothing)
	slot = 0u;
	idx = 0u;
	float ox = 0.0f, oy = 0.0f, oz = 0.0f, rx = 1.0f, ry = 1.0f, rz = 1.0f;
	if (live) {
		slot = r / a.rays;
		const uint32_t k = r - slot * a.rays;
		idx = a.order ? a.order[slot] : slot;
		const float4 p = a.points[idx], q = a.normals[idx];
		float nx = q.x, ny = q.y, nz = q.z;
		// p = point + normal * (1.0f / 100000.0f), reference :215
		const float eps = 1.0f / 100000.0f;
		ox = p.x + nx * eps;
		oy = p.y + ny * eps;
		oz = p.z + nz * eps;
		if (MODE == AO_RANDOM)
			normalize3(nx, ny, nz);  // hemisphere_sampler normalises once more, reference :155
		float bxx, bxy, bxz, bzx, bzy, bzz;
		tangent_frame(nx, ny, nz, bxx, bxy, bxz, bzx, bzy, bzz);
		float xs, ys, zs;
		if (MODE == AO_UNIFORM) {
			const float4 dir = a.ao_table[k];
			xs = dir.x; ys = dir.y; zs = dir.z;
		} else {
			// RANDOM: ray 0 goes along the normal (below), ray k >= 1 is sample k of the point's generator
			random_sample(a.seeds ? a.seeds[idx] : idx, k, xs, ys, zs);
		}
		// ray_dir = basis_x * xs + basis_y * ys + basis_z * zs
		rx = (bxx * xs + nx * ys) + bzx * zs;
		ry = (bxy * xs + ny * ys) + bzy * zs;
		rz = (bxz * xs + nz * ys) + bzz * zs;
		if (MODE == AO_RANDOM) {
			normalize3(rx, ry, rz);
			if (k == 0u) {  // the un-normalised normal itself (:263)
				rx = q.x; ry = q.y; rz = q.z;
			}
		}
	}
	return make_ray(ox, oy, oz, rx, ry, rz);
}

// The packet's hits by point: the first lane of a point's run adds the run's share of the ballot.
__device__ __forceinline__ void ao_query_count(const AoQueryArgs &a, uint32_t r, bool live, uint32_t slot, uint32_t idx, bool hit) {
	const unsigned long long hits = wave_ballot(hit);
	if (!live)
		return;
	const uint32_t lane = threadIdx.x & 63u, packet = r - lane;  // (the packet's first ray)
	const uint32_t run = slot * a.rays;                          // (the point's first ray)
	const uint32_t first = run > packet ? run - packet : 0u;
	if (lane != first)
		return;
	const uint32_t end = run + a.rays - packet;  // (> first: ray r is the point's; may lie beyond the packet)
	const unsigned long long below_end = end >= 64u ? ~0ull : (1ull << end) - 1ull;
	const uint32_t occluded = (uint32_t) __popcll(hits & below_end & ~((1ull << first) - 1ull));
	if (occluded)
		atomicAdd(&a.count[idx], occluded);
}

template <int MODE>
__global__ __launch_bounds__(64 * QUERY_WAVES) void ao_query_kernel(AoQueryArgs a) {
	const uint32_t r = blockIdx.x * (64u * QUERY_WAVES) + threadIdx.x;
	bool live;
	uint32_t slot, idx;
	const Ray ray = ao_query_ray<MODE>(a, r, live, slot, idx);
	bool alive = live, hit = false;
	// a lane leaves at its first accepted triangle
	exact_walk(a.nodes_ptr, a.node_count, ray, a.max_distance, alive, [&](uint32_t leaf, bool box) {
		const float4 *tri = a.tris_ptr + LEAF_F4 * leaf + LEAF_TRI_F4;
		const float4 q0 = tri[0], q1 = tri[1], q2 = tri[2], q3 = tri[3];
		if (box) {
			const TriResult tr = tri_eval<false>(q0, q1, q2, q3, ray);
			if (tr.accepted) {
				hit = true;
				alive = false;
			}
		}
		return wave_ballot(alive) == 0ull;
	});
	ao_query_count(a, r, live, slot, idx, hit);
}

// ao[i] = 1.0f - ((float) hits / (float) n), reference :256 / :275 (as the frame's finishing sweep resolves a sub-pixel).
__global__ __launch_bounds__(256) void ao_query_finish_kernel(const uint32_t *__restrict__ count, float *__restrict__ ao, uint32_t n,
                                                              uint32_t ao_divisor) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n)
		return;
	const float divisor = (float) ao_divisor;
	ao[i] = 1.0f - ((float) count[i] / divisor);
}

}  // namespace ocrt
