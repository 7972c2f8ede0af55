// kernels/instance_views.hip.h -- the instance set seen and shaded: ambient occlusion at world-space points against the
// posed copies, and the frame's own rays of many views against them (include/rt_hip_instance_views.h)
// (part of the one translation unit kernels.hip; see its head for the passes and the arithmetic contract)
//
// Both kernels go through instance_walk<CLOSEST> with instance_tri_eval at the leaf (kernels/instances.hip.h has the walk
// and its rules).
//
// instance_ao_kernel<MODE>: ao_query_kernel's packet (ao_query_ray: 64 consecutive rays of the flattened (slot, direction)
// list, each made in registers), the nested walk in its occlusion form, and ao_query_kernel's tail (ao_query_count: ballot,
// one vector atomic per (packet, point), none where nothing was hit).  `order` and `seeds` are that kernel's, so the views
// path hands it the list of a chunk's hit sub-pixels unchanged.
//
// instance_layers_kernel: layers_kernel<true, true>'s tiling and ray -- one wave per 8 x 8 tile, blockIdx.y the view, the
// pose by scalar loads from the chunk's poses, camera_ray<true> --, the nested walk in its closest form with
// instance_candidate, and an epilogue that writes the instanced record as instance_kernel writes it (the normal:
// instance_normal), the direction, the head-light term on that normal, and -- views always
// list -- the flag, seed, point and normal entries of the ambient-occlusion step with the missed sub-pixels' ao = 1 and
// value = 0.  What follows it (kernels/views.hip.h) runs as it is.
#pragma once
#include "ao_query.hip.h"
#include "instances.hip.h"
#include "layers.hip.h"

namespace ocrt {

struct InstanceAoArgs : AoQueryArgs {  // (nodes_ptr, tris_ptr, node_count: the scene's own; max_distance: in both spaces)
	InstanceSet set;
};

// MODE is AO_UNIFORM or AO_RANDOM, as for ao_query_kernel, whose ray and tail these are.
template <int MODE>
__global__ __launch_bounds__(64 * QUERY_WAVES) void instance_ao_kernel(InstanceAoArgs a) {
	const uint32_t r = blockIdx.x * (64u * QUERY_WAVES) + threadIdx.x;
	bool live;
	uint32_t slot, idx;
	const Ray ray = ao_query_ray<MODE>(a, r, live, slot, idx);
	const bool hit = instance_walk<false>(a.set, a.nodes_ptr, a.node_count, a.tris_ptr, ray, a.max_distance, live, InstanceTriEval{}, NoCandidate{});
	ao_query_count(a, r, live, slot, idx, hit);
}

struct InstanceLayersArgs : LayersArgs {  // (ARRAY and listing: `poses` is read; flags, seeds, points, normals where the step follows)
	InstanceSet set;
	uint32_t *instance;  // by sub-pixel index, the first view's block, or null
};

__global__ __launch_bounds__(64 * LAYERS_WAVES) void instance_layers_kernel(InstanceLayersArgs a) {
	// (wave-uniform by construction; read through the first lane so that the compiler keeps the tile in SGPRs, as the view is)
	const uint32_t tile = (uint32_t) __builtin_amdgcn_readfirstlane((int) (blockIdx.x * LAYERS_WAVES + (threadIdx.x >> 6)));
	const uint32_t view = blockIdx.y, lane = threadIdx.x & 63u;
	if (tile >= a.tiles)  // (the spare waves of a view's last workgroup)
		return;
	a.pose = a.poses[view];
	const uint32_t tile_y = tile / a.tiles_x, tile_x = tile - tile_y * a.tiles_x;
	const uint32_t x = tile_x * TILE_W + (lane & 7u), y = tile_y * TILE_H + (lane >> 3);
	// (a partial tile on the right or bottom edge: its lanes outside the image walk nothing and write nothing)
	const bool live = x < a.width && y < a.height;
	const Ray ray = camera_ray<true>(a, x, y);
	Hit best = closest_entry();
	uint32_t best_instance = 0u;
	const bool hit = instance_walk<true>(a.set, a.nodes_ptr, a.node_count, a.tris_ptr, ray, LAYERS_MAX_DISTANCE, live, InstanceTriEval{},
	                                     [&](uint32_t k, uint32_t leaf, const TriResult &tr, float r) {
		                                     instance_candidate(ray, k, leaf, tr, r, best, best_instance);
	                                     });
	if (!live)
		return;
	const uint32_t seed = y * a.width + x;          // the sub-pixel's index within its view
	const size_t idx = (size_t) view * a.n + seed;  // ... and within the launch: view v's block of every layer
	// the record, as instance_kernel<true> writes it (not through instance_store_record: the normal also feeds the head-light term and the list)
	if (a.hit)
		a.hit[idx] = hit ? 1u : 0u;
	const bool kept = hit && best.distance < __builtin_inff();  // (the record was replaced at least once)
	if (a.instance)
		a.instance[idx] = hit ? best_instance : NONE;
	if (a.out.distance)
		a.out.distance[idx] = best.distance;
	if (a.out.leaf)
		a.out.leaf[idx] = hit ? best.leaf : NONE;
	const float b0 = kept ? 1.0f - best.s - best.t : 0.0f, b1 = kept ? best.s : 0.0f, b2 = kept ? best.t : 0.0f;
	const float px = kept ? best.px : 0.0f, py = kept ? best.py : 0.0f, pz = kept ? best.pz : 0.0f;
	if (a.out.barycentric) {
		a.out.barycentric[3u * idx + 0u] = b0;
		a.out.barycentric[3u * idx + 1u] = b1;
		a.out.barycentric[3u * idx + 2u] = b2;
	}
	if (a.out.position) {
		a.out.position[3u * idx + 0u] = px;
		a.out.position[3u * idx + 1u] = py;
		a.out.position[3u * idx + 2u] = pz;
	}
	if (a.direction) {
		a.direction[3u * idx + 0u] = ray.dx;
		a.direction[3u * idx + 1u] = ray.dy;
		a.direction[3u * idx + 2u] = ray.dz;
	}
	if (!a.out.normal && !a.shade && !a.value && !a.points)
		return;
	// the record's normal, and the head-light term (reference :296-304) on those words
	float value = 0.0f;
	float wx = 0.0f, wy = 0.0f, wz = 0.0f;
	if (hit) {
		instance_normal(a.shade_recs, a.set.inverses, best.leaf, best_instance, b0, b1, b2, wx, wy, wz);
		value = 1.0f;
		if (a.shading)
			value = fminf(fmaxf(-dot3(wx, wy, wz, ray.dx, ray.dy, ray.dz), 0.0f), 1.0f);
	}
	if (a.out.normal) {
		a.out.normal[3u * idx + 0u] = wx;
		a.out.normal[3u * idx + 1u] = wy;
		a.out.normal[3u * idx + 2u] = wz;
	}
	if (a.shade)
		a.shade[idx] = value;
	if (a.value)
		a.value[idx] = value;
	if (!a.points)
		return;
	// the ambient-occlusion step follows: a missed sub-pixel is final, a hit one goes onto the list
	if (!hit) {
		if (a.ao)
			a.ao[idx] = 1.0f;
		if (a.product)
			a.product[idx] = 0.0f;
	}
	a.flags[idx] = hit ? 1u : 0u;
	if (hit) {
		a.seeds[idx] = seed;
		a.points[idx] = make_float4(px, py, pz, 1.0f);
		a.normals[idx] = make_float4(wx, wy, wz, value);
	}
}

}  // namespace ocrt
