// kernels/layers.hip.h -- the frame's own rays: the closest-hit record of every sub-pixel of one pose or of many, and what
// the frame makes of it (include/rt_hip_layers.h, include/rt_hip_views.h)
// (part of the one translation unit kernels.hip; see its head for the passes and the arithmetic contract)
//
// layers_kernel<POSED, ARRAY> packs its rays as the primary pass does -- one wave per 8 x 8 tile of sub-pixels, lane & 7 across,
// lane >> 3 down, four waves per workgroup -- and makes each ray in registers with the primary pass's arithmetic
// (camera_ray below restates primary_tile's lines: a helper of its own, so that the frame kernels' code, registers and
// hand-scheduled loop stay exactly as they are); no ray array exists.  The grid is tiles by views -- blockIdx.y is the
// view, so no wave divides to find it --: a wave's view is a scalar, and its pose comes by scalar loads from the call's array of poses on the device or, where there is none (a
// layers call: one view), from the kernel arguments.  From there on it is query_kernel<true>: the EXACT form of the
// shared walk (walk.hip.h, exact_walk) over the uploaded scene's exact node records with the frame's max_distance,
// tri_eval<true>, nearer and take at a leaf, and closest_entry and closest_store (kernels/query.hip.h) for the record --
// so the answer is the query contract's for any pose, non-finite eyes and eyes the fast walk's margins do not cover included.  The epilogue adds the
// ray's direction and the head-light term (the primary epilogue's dot3, max and min).  Everything is written into view
// v's block of every layer, at view * N + index.
//
// With the ambient-occlusion step to follow, the kernel leaves a sub-pixel's point and normal as float4 (normal.w: the
// head-light term) at the sub-pixel's index, for ao_query_kernel to run over and views_scatter_kernel (kernels/views.hip.h)
// to write `ao` and `value` from.  Two modes, a uniform branch on `flags`:
//   not listing (a layers call)  every live lane writes its entry, and the step runs over all N sub-pixels in index order
//       -- point i gets seed i = y * W + x, the reference's `index`.  A sub-pixel without a hit leaves a NaN point and a
//       zero normal: its ambient-occlusion rays fail the slab test at the root and walk nothing, so its count stays 0 and
//       the tail's own arithmetic gives ao = 1 - 0 / n = 1 and value = 0 * 1 = +0.  Nothing is read back: the call only enqueues.
//   listing (a views call)  the sub-pixels that were HIT -- and only they -- are listed for the step.  Every live lane leaves
//       its hit flag, a hit one also its entry and the reference's `index` of the sub-pixel WITHIN ITS VIEW (the RANDOM
//       sampler's seed); a missed one gets its ao = 1, value = 0 here.  kernels/views.hip.h makes the list's order.
#pragma once
#include "query.hip.h"

namespace ocrt {

struct LayersArgs {
	const float4 *nodes_ptr;  // SceneBuffers::nodes: exact boxes, builder order (NodeRec)
	const float4 *tris_ptr;   // TriRec by leaf
	const float4 *shade_recs; // ShadeRec by leaf
	uint32_t width, height;   // sub-pixels
	uint32_t tiles_x, tiles;  // tiles per row, tiles per view
	uint32_t node_count;
	int32_t shading;
	float a, half_w, half_h;  // KernelParams: the camera-space terms of a sub-pixel
	CameraPose pose;          // (POSED, not ARRAY) the pose of the one view
	const CameraPose *poses;  // (ARRAY) [views] on the device
	uint32_t n;               // sub-pixels per view
	uint8_t *hit;             // by sub-pixel index, the first view's block; every output: null = not written
	RecordOutputs out;
	float *direction;         // float[3 n] per view
	float *shade;             // float[n]: the head-light term
	float *value;             // float[n]: the same once more -- `value` of a host without ambient occlusion
	float4 *points, *normals; // [views * n] the entries of the ambient-occlusion step; null: no such step follows
	uint8_t *flags;           // [views * n] 1 = hit: listed; null: not listing
	uint32_t *seeds;          // [views * n] (listing)
	float *ao, *product;      // [views * n] or null (listing): the missed sub-pixels' 1.0f and 0.0f
};

constexpr uint32_t LAYERS_WAVES = 4u;
constexpr float LAYERS_MAX_DISTANCE = 100000.0f;  // the primary rays' (reference src/intersect_kernel.cl:295)

// The ray the frame casts for sub-pixel (x, y): reference src/intersect_kernel.cl:279-295, and for a posed host
// include/rt_hip_camera.h -- direction = normalize(((right * cx) + (up * cy)) + forward), every product and sum rounded
// on its own (this file is compiled without contraction).  The default form keeps the reference's camera folded in:
// the direction is normalize((cx, cy, -1)) itself, so a cy of -0 stays -0.  The same operations in the same order as
// primary_tile's.
template <bool POSED>
__device__ __forceinline__ Ray camera_ray(const LayersArgs &a, uint32_t x, uint32_t y) {
	float dx = ((float) x + 0.5f) / a.a - a.half_w;
	float dy = -(((float) y + 0.5f) / a.a - a.half_h);
	float dz = -1.0f;
	if (POSED) {
		const float cx = dx, cy = dy;
		dx = (a.pose.right[0] * cx + a.pose.up[0] * cy) + a.pose.forward[0];
		dy = (a.pose.right[1] * cx + a.pose.up[1] * cy) + a.pose.forward[1];
		dz = (a.pose.right[2] * cx + a.pose.up[2] * cy) + a.pose.forward[2];
	}
	normalize3(dx, dy, dz);
	return POSED ? make_ray(a.pose.eye[0], a.pose.eye[1], a.pose.eye[2], dx, dy, dz) : make_ray(0.0f, 0.0f, 2.0f, dx, dy, dz);
}

// POSED: a pose is read at all; ARRAY: from `poses` (then POSED), else from the arguments.  Where the pose comes from is a
// template parameter because as a run-time branch it cost the posed layers call 1 to 1.5 %.
template <bool POSED, bool ARRAY>
__global__ __launch_bounds__(64 * LAYERS_WAVES) void layers_kernel(LayersArgs a) {
	// (wave-uniform by construction; read through the first lane so that the compiler keeps the tile in SGPRs, as the view is)
	const uint32_t tile = (uint32_t) __builtin_amdgcn_readfirstlane((int) (blockIdx.x * LAYERS_WAVES + (threadIdx.x >> 6)));
	const uint32_t view = blockIdx.y, lane = threadIdx.x & 63u;
	if (tile >= a.tiles)  // (the spare waves of a view's last workgroup)
		return;
	if (ARRAY)
		a.pose = a.poses[view];
	const uint32_t tile_y = tile / a.tiles_x, tile_x = tile - tile_y * a.tiles_x;
	const uint32_t x = tile_x * TILE_W + (lane & 7u), y = tile_y * TILE_H + (lane >> 3);
	// (a partial tile on the right or bottom edge: its lanes outside the image walk nothing and write nothing)
	const bool live = x < a.width && y < a.height;
	const Ray ray = camera_ray<POSED>(a, x, y);
	bool hit = false;
	Hit best = closest_entry();
	exact_walk(a.nodes_ptr, a.node_count, ray, LAYERS_MAX_DISTANCE, live, [&](uint32_t leaf, bool box) {
		const float4 *tri = a.tris_ptr + LEAF_F4 * leaf + LEAF_TRI_F4;
		const float4 q0 = tri[0], q1 = tri[1], q2 = tri[2], q3 = tri[3];
		if (box) {
			const TriResult tr = tri_eval<true>(q0, q1, q2, q3, ray);
			if (tr.accepted) {
				hit = true;
				if (nearer(tr.distance, leaf, best))
					take(best, tr, leaf);
			}
		}
		return false;  // (closest hit: nobody leaves the walk)
	});
	if (!live)
		return;
	const uint32_t seed = y * a.width + x;          // the sub-pixel's index within its view
	const size_t idx = (size_t) view * a.n + seed;  // ... and within the launch: view v's block of every layer
	const ClosestRecord rec = closest_store(a.hit, a.out, idx, a.shade_recs, hit, best);
	if (a.direction) {
		a.direction[3u * idx + 0u] = ray.dx;
		a.direction[3u * idx + 1u] = ray.dy;
		a.direction[3u * idx + 2u] = ray.dz;
	}
	if (!a.shade && !a.value && !a.points)
		return;
	// smooth normal and head-light term, reference :296-304, on the record's barycentrics
	float value = 0.0f;
	float nx = 0.0f, ny = 0.0f, nz = 0.0f;
	if (hit) {
		smooth_normal(a.shade_recs, best.leaf, rec.b0, rec.b1, rec.b2, nx, ny, nz);
		value = 1.0f;
		if (a.shading)
			value = fminf(fmaxf(-dot3(nx, ny, nz, ray.dx, ray.dy, ray.dz), 0.0f), 1.0f);
	}
	if (a.shade)
		a.shade[idx] = value;
	if (a.value)
		a.value[idx] = value;
	if (!a.points)
		return;
	// the ambient-occlusion step follows
	if (a.flags) {
		// listing: a missed sub-pixel is final, a hit one goes onto the list
		if (!hit) {
			if (a.ao)
				a.ao[idx] = 1.0f;
			if (a.product)
				a.product[idx] = 0.0f;
		}
		a.flags[idx] = hit ? 1u : 0u;
		if (hit)
			a.seeds[idx] = seed;
	}
	if (hit || !a.flags) {
		const float none = __builtin_nanf("");
		a.points[idx] = hit ? make_float4(rec.px, rec.py, rec.pz, 1.0f) : make_float4(none, none, none, 0.0f);
		a.normals[idx] = make_float4(nx, ny, nz, value);
	}
}

}  // namespace ocrt
