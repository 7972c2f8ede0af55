// kernels/views.hip.h -- what follows layers_kernel (kernels/layers.hip.h) where the ambient-occlusion step or the 8-bit
// images are asked for: the list of a chunk's hit sub-pixels, the step's tail, and the images of many views
// (include/rt_hip_layers.h, include/rt_hip_views.h)
// (part of the one translation unit kernels.hip; see its head for the passes and the arithmetic contract)
//
// The list (views calls).  layers_kernel leaves a flag per sub-pixel of the chunk, at view * N + index.
// views_count_kernel counts the flags by blocks of 1024 sub-pixels, views_scan_sums_kernel makes the counts' exclusive
// prefix sums -- the last one is the number of hit sub-pixels of the chunk, which sizes the ambient-occlusion launch --,
// and views_order_kernel writes the order array ao_query_kernel accepts: slot j of its ray list is the j-th hit sub-pixel
// in index order, view by view, row by row.  ao_query_kernel then runs UNCHANGED over exactly the hit sub-pixels, in the
// order a layers call runs it over all of them.  No atomic, and nothing depends on how waves are scheduled.
// (Two earlier forms, measured at 1920 x 1080 with 1.56 M of 2.07 M sub-pixels hit, DESIGN.md section 15.  A ballot-ranked
// append with one returning atomic per wave on one counter, entries in the order the atomics landed: the 24 000 atomics
// on one address doubled the ray kernel, 0.25 -> 0.49 ms, and ao_query_kernel took 7.78 ms over the list against 7.13 ms
// over all sub-pixels in index order.  Ranked writes to 64 places per wave and a scan, entries tile by tile: 0.25 ms and
// 7.46 ms.  The order of the points is worth more to that kernel than the lanes compaction saves.)
//
// The tail (layers and views calls alike).  views_scatter_kernel writes factor and product of the step's entries from
// its counts: the listed ones through the order array, or -- no order array: a layers call -- all of them, entry j being
// sub-pixel j.
//
// views_resize_kernel is resize_kernel's arithmetic for every view of the chunk in one launch.
#pragma once
#include "layers.hip.h"

namespace ocrt {

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
// head-light term * ao (the frame's finishing sweep's product) of the `listed` entries of the ambient-occlusion step, each
// where its sub-pixel lies: order[j], or j where `order` is null (either output may be null).  An entry of a missed
// sub-pixel -- only a layers call has them -- has count 0 and normals.w = 0: ao = 1 - 0 = 1, value = 0 * 1 = +0.
__global__ __launch_bounds__(256) void views_scatter_kernel(const float4 *__restrict__ normals, const uint32_t *__restrict__ count,
                                                            const uint32_t *__restrict__ order, float *ao, float *product, uint32_t listed,
                                                            uint32_t ao_divisor) {
	const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= listed)
		return;
	const uint32_t idx = order ? order[j] : j;
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
