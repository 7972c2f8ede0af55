// kernels/layers.hip.h -- frame layers: the closest-hit record of every sub-pixel's own ray and what the frame makes of
// it (include/rt_hip_layers.h)
// (part of the one translation unit kernels.hip; see its head for the passes and the arithmetic contract)
//
// layers_kernel<POSED> packs its rays as the primary pass does -- one wave per 8 x 8 tile of sub-pixels, lane & 7 across,
// lane >> 3 down, four waves per workgroup -- and makes each ray in registers with the primary pass's arithmetic
// (camera_ray below restates primary_tile's lines: a helper of its own, so that the frame kernels' code, registers and
// hand-scheduled loop stay exactly as they are); no ray array exists.  From there on it is query_kernel<true>: the
// EXACT form of the shared walk (walk.hip.h, exact_walk) over the uploaded scene's exact node records with the frame's
// max_distance, tri_eval<true>, nearer, take, and store_record for the record -- so the answer is the query contract's
// for any pose, non-finite eyes and eyes the fast walk's margins do not cover included.  The epilogue adds the ray's
// direction and the head-light term (the primary epilogue's dot3, max and min).
//
// With ambient occlusion asked for, the kernel also leaves every sub-pixel's point and normal as float4 in scratch
// (point.w: the hit flag, normal.w: the head-light term) for ao_query_kernel to run over in index order -- point i gets
// seed i = y * W + x, the reference's `index` --, and layers_combine_kernel writes `ao` and `value` from its factors.  A
// sub-pixel without a hit leaves a NaN point: its ambient-occlusion rays fail the slab test at the root and walk
// nothing, and the combine step writes ao = 1, value = 0 for it whatever the factor says.
#pragma once
#include "query.hip.h"

namespace ocrt {

struct LayersArgs {
	const float4 *nodes_ptr;  // SceneBuffers::nodes: exact boxes, builder order (NodeRec)
	const float4 *tris_ptr;   // TriRec by leaf
	const float4 *shade_recs; // ShadeRec by leaf
	uint32_t width, height;   // sub-pixels
	uint32_t tiles_x, tiles;  // tiles per row, tiles in all
	uint32_t node_count;
	int32_t shading;
	float a, half_w, half_h;  // KernelParams: the camera-space terms of a sub-pixel
	CameraPose pose;          // (POSED only)
	uint8_t *hit;             // by sub-pixel index; every output: null = not written
	RecordOutputs out;
	float *direction;         // float[3 n]
	float *shade;             // float[n]: the head-light term
	float *value;             // float[n]: the same once more -- `value` of a host without ambient occlusion
	float4 *points, *normals; // float4[n] scratch for the ambient-occlusion step, or null
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

template <bool POSED>
__global__ __launch_bounds__(64 * LAYERS_WAVES) void layers_kernel(LayersArgs a) {
	const uint32_t tile = blockIdx.x * LAYERS_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
	if (tile >= a.tiles)  // (the last workgroup's spare waves)
		return;
	const uint32_t tile_y = tile / a.tiles_x, tile_x = tile - tile_y * a.tiles_x;
	const uint32_t x = tile_x * TILE_W + (lane & 7u), y = tile_y * TILE_H + (lane >> 3);
	// (a partial tile on the right or bottom edge: its lanes outside the image walk nothing and write nothing)
	const bool live = x < a.width && y < a.height;
	const Ray ray = camera_ray<POSED>(a, x, y);
	bool hit = false;
	Hit best;
	best.distance = __builtin_inff();
	best.leaf = 0u;
	best.s = best.t = 0.0f;
	best.px = best.py = best.pz = 0.0f;
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
	const size_t idx = (size_t) y * a.width + x;
	// the record, as query_kernel<true> writes it
	if (a.hit)
		a.hit[idx] = hit ? 1u : 0u;
	const bool kept = hit && best.distance < __builtin_inff();  // (the record was replaced at least once)
	const float b0 = kept ? 1.0f - best.s - best.t : 0.0f, b1 = kept ? best.s : 0.0f, b2 = kept ? best.t : 0.0f;
	const float px = kept ? best.px : 0.0f, py = kept ? best.py : 0.0f, pz = kept ? best.pz : 0.0f;
	if (a.out.distance)
		a.out.distance[idx] = best.distance;
	if (a.out.leaf)
		a.out.leaf[idx] = hit ? best.leaf : NONE;
	store_record(a.out, idx, a.shade_recs, best.leaf, hit, b0, b1, b2, px, py, pz);
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
		smooth_normal(a.shade_recs, best.leaf, b0, b1, b2, nx, ny, nz);
		value = 1.0f;
		if (a.shading)
			value = fminf(fmaxf(-dot3(nx, ny, nz, ray.dx, ray.dy, ray.dz), 0.0f), 1.0f);
	}
	if (a.shade)
		a.shade[idx] = value;
	if (a.value)
		a.value[idx] = value;
	if (a.points) {
		const float none = __builtin_nanf("");
		a.points[idx] = hit ? make_float4(px, py, pz, 1.0f) : make_float4(none, none, none, 0.0f);
		a.normals[idx] = make_float4(nx, ny, nz, value);
	}
}

// ao[i] and value[i] = shade * ao of sub-pixel i from the factors of the ambient-occlusion step over layers_kernel's
// points (`factor` may be `ao` itself); without a hit: ao = 1, value = 0.  The product is the frame's finishing sweep's.
__global__ __launch_bounds__(256) void layers_combine_kernel(const float4 *__restrict__ points, const float4 *__restrict__ normals,
                                                             const float *factor, float *ao, float *value, uint32_t n) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n)
		return;
	const bool hit = points[i].w != 0.0f;
	const float f = hit ? factor[i] : 1.0f;
	if (ao)
		ao[i] = f;
	if (value)
		value[i] = hit ? normals[i].w * f : 0.0f;
}

}  // namespace ocrt
