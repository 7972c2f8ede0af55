// kernels/views.hip.h -- multi-view rendering: the frame layers and the 8-bit image of many camera poses against one
// uploaded scene (include/rt_hip_views.h)
// (part of the one translation unit kernels.hip; see its head for the passes and the arithmetic contract)
//
// views_kernel is layers_kernel<true> once per view of a chunk: one wave per (view, 8 x 8 tile), four waves per
// workgroup, the grid covers chunk views x tiles.  A wave's view is a scalar; its pose comes by scalar loads from the
// chunk's array of poses on the device -- not from the kernel arguments, which are the same for every view -- and the
// ray is camera_ray<true> itself (kernels/layers.hip.h).  The walk (exact_walk, the EXACT form), the triangle test, the
// record (nearer, take, store_record) and the epilogue (smooth_normal, the head-light term) are layers_kernel's, through the
// same helpers; the lines that join them are restated here -- layers_kernel's own code stays as it is, as the frame
// kernels' did when it was written -- and write into view v's block of every layer.
//
// With the ambient-occlusion step to follow, the sub-pixels that were HIT -- and only they -- are listed for it.  Every
// live lane leaves its hit flag, a hit one also its point, its normal with the head-light term in .w and the reference's
// `index` of the sub-pixel WITHIN ITS VIEW (y * W + x: the RANDOM sampler's seed), all at the sub-pixel's index within
// the chunk, view * N + index; a missed one gets its ao = 1, value = 0 here.  views_count_kernel counts the flags by
// blocks of 1024 sub-pixels, views_scan_sums_kernel makes the counts' exclusive prefix sums -- the last one is the number
// of hit sub-pixels of the chunk, which sizes the ambient-occlusion launch --, and views_order_kernel writes the order
// array ao_query_kernel accepts: slot j of its ray list is the j-th hit sub-pixel in index order, view by view, row by
// row.  ao_query_kernel then runs UNCHANGED over exactly the hit sub-pixels, in the order layersDevice runs it over all
// of them, and views_scatter_kernel writes factor and product.  No atomic, and nothing depends on how waves are scheduled.
// (Two earlier forms, measured at 1920 x 1080 with 1.56 M of 2.07 M sub-pixels hit, DESIGN.md section 15.  A ballot-ranked
// append with one returning atomic per wave on one counter, entries in the order the atomics landed: the 24 000 atomics
// on one address doubled views_kernel, 0.25 -> 0.49 ms, and ao_query_kernel took 7.78 ms over the list against 7.13 ms
// over all sub-pixels in index order.  Ranked writes to 64 places per wave and a scan, entries tile by tile: 0.25 ms and
// 7.46 ms.  The order of the points is worth more to that kernel than the lanes compaction saves.)
//
// views_resize_kernel is resize_kernel's arithmetic for every view of the chunk in one launch.
#pragma once
#include "layers.hip.h"

namespace ocrt {

struct ViewsArgs {
	LayersArgs layers;         // every output: the chunk's first view's block; `pose`, `points`, `normals` unset
	const CameraPose *poses;   // [views] the chunk's poses
	uint32_t views, n;         // views in the chunk; sub-pixels per view
	float *ao, *product;       // [views * n] or null: the missed sub-pixels' 1.0f and 0.0f (the hit ones: views_scatter_kernel)
	uint8_t *flags;            // [views * n] 1 = hit: listed
	float4 *points, *normals;  // [views * n] the hit sub-pixels' entries; null: no ambient-occlusion step follows
	uint32_t *seeds;           // [views * n]
};

__global__ __launch_bounds__(64 * LAYERS_WAVES) void views_kernel(ViewsArgs v) {
	// (wave-uniform by construction; read through the first lane so that the compiler keeps view and tile in SGPRs)
	const uint32_t wave = (uint32_t) __builtin_amdgcn_readfirstlane((int) (blockIdx.x * LAYERS_WAVES + (threadIdx.x >> 6)));
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t view = wave / v.layers.tiles, tile = wave - view * v.layers.tiles;
	if (view >= v.views)  // (the last workgroup's spare waves)
		return;
	LayersArgs a = v.layers;
	a.pose = v.poses[view];
	const uint32_t tile_y = tile / a.tiles_x, tile_x = tile - tile_y * a.tiles_x;
	const uint32_t x = tile_x * TILE_W + (lane & 7u), y = tile_y * TILE_H + (lane >> 3);
	const bool live = x < a.width && y < a.height;
	const Ray ray = camera_ray<true>(a, x, y);
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
	const uint32_t seed = y * a.width + x;                // the sub-pixel's index within its view
	const size_t idx = (size_t) view * v.n + seed;        // ... and within the chunk: view v's block of every layer
	// the record and the epilogue, as layers_kernel writes them
	if (a.hit)
		a.hit[idx] = hit ? 1u : 0u;
	const bool kept = hit && best.distance < __builtin_inff();
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
	if (!a.shade && !a.value && !v.points)
		return;
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
	if (!v.points)
		return;
	// the ambient-occlusion step follows: a missed sub-pixel is final, a hit one goes onto the list
	if (!hit) {
		if (v.ao)
			v.ao[idx] = 1.0f;
		if (v.product)
			v.product[idx] = 0.0f;
	}
	v.flags[idx] = hit ? 1u : 0u;
	if (hit) {
		v.points[idx] = make_float4(px, py, pz, 1.0f);
		v.normals[idx] = make_float4(nx, ny, nz, value);
		v.seeds[idx] = seed;
	}
}

// The hit sub-pixels in index order.  views_count_kernel: sums[b] = the flags set among the 1024 sub-pixels of block b;
// views_scan_sums_kernel (ONE workgroup): sums[] becomes its exclusive prefix sums, *total the grand total;
// views_order_kernel: order[sums[b] + rank within the block] = the sub-pixel, for every flag set.
constexpr uint32_t VIEWS_SCAN = 1024u, VIEWS_SUMS = 1024u;

// This thread's rank among the workgroup's (VIEWS_SCAN threads) flagged ones, and -- for every thread -- their number.
__device__ __forceinline__ uint32_t block_rank(bool flag, uint32_t &total) {
	__shared__ uint32_t waves[VIEWS_SCAN / 64u];
	const unsigned long long set = wave_ballot(flag);
	const uint32_t wave = threadIdx.x >> 6;
	if ((threadIdx.x & 63u) == 0u)
		waves[wave] = (uint32_t) __popcll(set);
	__syncthreads();
	uint32_t before = 0u;
	total = 0u;
	for (uint32_t w = 0; w < VIEWS_SCAN / 64u; ++w) {
		before += w < wave ? waves[w] : 0u;
		total += waves[w];
	}
	return before + rank_in(set);
}

__global__ __launch_bounds__(VIEWS_SCAN) void views_count_kernel(const uint8_t *__restrict__ flags, uint32_t *__restrict__ sums, uint32_t m) {
	const uint32_t i = blockIdx.x * VIEWS_SCAN + threadIdx.x;
	uint32_t total;
	(void) block_rank(i < m && flags[i] != 0u, total);
	if (threadIdx.x == 0u)
		sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(VIEWS_SUMS) void views_scan_sums_kernel(uint32_t *__restrict__ sums, uint32_t blocks, uint32_t *__restrict__ total) {
	__shared__ uint32_t part[VIEWS_SUMS];
	const uint32_t t = threadIdx.x;
	uint32_t carry = 0u;
	for (uint32_t first = 0u; first < blocks; first += VIEWS_SUMS) {  // (uniform: every thread takes every turn)
		const uint32_t i = first + t, mine = i < blocks ? sums[i] : 0u;
		part[t] = mine;
		__syncthreads();
		for (uint32_t step = 1u; step < VIEWS_SUMS; step <<= 1) {
			const uint32_t add = t >= step ? part[t - step] : 0u;
			__syncthreads();
			part[t] += add;
			__syncthreads();
		}
		if (i < blocks)
			sums[i] = carry + part[t] - mine;
		carry += part[VIEWS_SUMS - 1u];
		__syncthreads();
	}
	if (t == 0u)
		*total = carry;
}

__global__ __launch_bounds__(VIEWS_SCAN) void views_order_kernel(const uint8_t *__restrict__ flags, const uint32_t *__restrict__ sums,
                                                                 uint32_t *__restrict__ order, uint32_t m) {
	const uint32_t i = blockIdx.x * VIEWS_SCAN + threadIdx.x;
	const bool flag = i < m && flags[i] != 0u;
	uint32_t total;
	const uint32_t rank = block_rank(flag, total);
	if (flag)
		order[sums[blockIdx.x] + rank] = i;  // (< the grand total <= m: the sums count exactly these)
}

// ao = 1.0f - ((float) hits / (float) n) -- ao_query_finish_kernel's expression, reference :256 / :275 -- and value =
// head-light term * ao of the `listed` entries, each where its sub-pixel lies (either output may be null).  The product is
// layers_combine_kernel's, the frame's finishing sweep's.
__global__ __launch_bounds__(256) void views_scatter_kernel(const float4 *__restrict__ normals, const uint32_t *__restrict__ count,
                                                            const uint32_t *__restrict__ order, float *ao, float *product, uint32_t listed,
                                                            uint32_t ao_divisor) {
	const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= listed)
		return;
	const uint32_t idx = order[j];
	const float divisor = (float) ao_divisor;
	const float f = 1.0f - ((float) count[idx] / divisor);
	if (ao)
		ao[idx] = f;
	if (product)
		product[idx] = normals[idx].w * f;
}

// Supersample box filter + 8-bit quantisation of every view of a chunk: resize_kernel's sum (ssY-major, ssX-minor) and
// truncating store, reference src/ray_tracer.cc:3-16; blockIdx.y: the output row, blockIdx.z: the view.
__global__ __launch_bounds__(256) void views_resize_kernel(const float *__restrict__ value, unsigned char *__restrict__ image, uint32_t width,
                                                           uint32_t height, uint32_t total_width, uint32_t n, uint32_t per_view) {
	const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t y = blockIdx.y, view = blockIdx.z;
	if (x >= width)
		return;
	const float *tmp = value + (size_t) view * per_view;
	float total = 0.0f;
	for (uint32_t sy = 0; sy < n; ++sy) {
		const float *row = tmp + (size_t) (y * n + sy) * total_width + (size_t) x * n;
		for (uint32_t sx = 0; sx < n; ++sx)
			total += row[sx];
	}
	image[((size_t) view * height + y) * width + x] = (unsigned char) ((total / (float) (n * n)) * 255.0f);
}

}  // namespace ocrt
