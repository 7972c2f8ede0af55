// kernels.hip -- gfx950 ray-casting kernels (the replacement for reference
// src/intersect_kernel.cl).
//
// Arithmetic contract: IEEE binary32 + - * / sqrt in the
// reference's operation order, NO fma contraction (this file is compiled with
// -ffp-contract=off), IEEE maxNum/minNum for max/min, double-literal
// comparisons folded to their exact float thresholds.  Anything else (data
// layout, traversal order, where a value is computed) is free and is chosen
// for the CDNA4 wave64 machine.
//
// Work decomposition: one 64-lane wavefront per 8x8 tile of sub-pixels, in two ray passes and a finishing sweep --
// three kernels per frame, captured once per host as a hipGraph and replayed.
//   primary_kernel  every lane casts its primary ray (closest hit) and computes
//                   the smooth normal and head-light term.  Sub-pixels that need
//                   no ambient occlusion are final; the tile's other hits leave a TAG in the image and
//                   are ballot-compacted into the tile's slots of the hit list (tile_base: sized by what is hit).
//                   The order the next pass takes the tiles in is made once per upload, on the host
//                   (DeviceRenderer::orderTiles: each XCD group's non-empty tiles, the costly blocks first).
//   ao_kernel       persistent workgroups claim runs of (tile, table direction) units in
//                   that order -- a tile at a time, whose directions the four waves take
//                   from a cursor in LDS.  A wave rebuilds the tile's tangent frames in its
//                   LDS slice and casts one packet of 64 any-hit rays per
//                   direction -- one table direction from the tile's neighbouring
//                   surface points -- that stop at the first accepted triangle and walk only
//                   the interval of the node array their segments can reach (entry_kernel, once per upload);
//                   occlusion counts are LDS atomics, flushed to a per-hit counter
//                   when the claim is done.
//   finish_kernel / finish_wide_kernel
//                   value * (1 - occluded / n) into the tagged sub-pixels and the supersample box filter +
//                   quantisation of the same sweep (n = 1: a thread per pixel; n >= 2: along the sub-pixel rows).
//   (queries)       query_key_kernel / query_scan_kernel / query_scatter_kernel order caller-supplied rays by a coherence
//                   key, query_kernel<CLOSEST> casts them (kernels/query.hip.h, include/rt_hip_query.h): not part of a frame.
//                   ao_query_kernel<MODE> makes, casts and counts the ambient-occlusion rays of caller-supplied points,
//                   ao_query_finish_kernel writes their 1 - hits / n (kernels/ao_query.hip.h, include/rt_hip_ao.h).
//                   ao_mask_kernel<MODE> casts the same rays and keeps their hit flags apart, a bit per ray,
//                   ao_directional_finish_kernel<MODE> writes a point's count, value and the sum of its open rays' directions,
//                   ao_rays_kernel<MODE> the rays themselves (kernels/directional.hip.h, include/rt_hip_directional.h).
//                   multihit_walk_kernel<K> counts every triangle a caller-supplied ray's walk accepts and keeps the first K,
//                   multihit_resolve_kernel writes their records (kernels/multihit.hip.h, include/rt_hip_multihit.h).
//                   nearest_key_kernel / nearest_scatter_kernel order caller-supplied POINTS by position, nearest_kernel finds
//                   the nearest point of the surface for each (kernels/nearest.hip.h, include/rt_hip_nearest.h);
//                   instance_nearest_kernel finds it among the posed copies of an instance set, measured in world space
//                   (kernels/instance_nearest.hip.h, include/rt_hip_instance_nearest.h);
//                   signed_kernel and signed_grid_kernel are nearest_kernel's walk with a signed tail -- for points, and for
//                   the voxels of a grid made in registers, a 4 x 4 x 4 brick per wave --, over the sign table that
//                   sign_keys_kernel, sign_heads_kernel, sign_sum_kernel and sign_leaf_kernel make around sign_sort.hip's
//                   sorts (kernels/signed.hip.h, include/rt_hip_signed.h).
//                   segment_kernel<CLOSEST> answers whether the line between two caller-supplied points is free, or where it is
//                   blocked first (segment_key_kernel / segment_scatter_kernel order the segments), visibility_mask_kernel
//                   does so for P points against T targets, a bit per pair, visibility_count_kernel counts a point's bits
//                   (kernels/segment.hip.h, include/rt_hip_segment.h).
//                   instance_kernel<CLOSEST> casts caller-supplied rays against posed copies of the scene: an exact walk over a
//                   top-level tree of instance boxes, and at each instance a packet enters the exact walk of the scene's own
//                   tree with the rays mapped into the object's frame -- the nested walk that the instanced kernels below
//                   share as instance_walk (kernels/instances.hip.h, include/rt_hip_instances.h).
//                   layers_kernel<POSED, ARRAY> casts the frame's own rays for one pose or for every pose of a chunk of views, a wave
//                   per (view, tile), and writes every sub-pixel's record, direction and head-light term (kernels/layers.hip.h,
//                   include/rt_hip_layers.h, include/rt_hip_views.h).  ao_query_kernel runs over its points -- all of them
//                   (a layers call) or the hit ones, listed (a views call: views_count_kernel, views_scan_sums_kernel,
//                   views_order_kernel make their number and order) --, views_scatter_kernel writes their factors and
//                   products, views_resize_kernel every view's 8-bit image (kernels/views.hip.h).
//                   instance_layers_kernel and instance_ao_kernel<MODE> are layers_kernel<true, true> and ao_query_kernel
//                   against the posed copies: the same rays, made in registers by the same functions, through instance_walk;
//                   the list, the tail and the images between and behind them are the views' own (kernels/instance_views.hip.h,
//                   include/rt_hip_instance_views.h).
//                   instance_segment_kernel<CLOSEST> and instance_visibility_kernel are segment_kernel and
//                   visibility_mask_kernel against the posed copies: the same packets and tails, shared functions, around
//                   instance_walk with the interval test on the object ray's plane parameter (kernels/instance_segments.hip.h,
//                   include/rt_hip_instance_segments.h).
//                   instance_multihit_walk_kernel<K> and instance_multihit_resolve_kernel are the multi-hit kernels against the
//                   posed copies: the lane's list keyed by (distance, instance, leaf), around instance_walk in its closest form
//                   (kernels/instance_multihit.hip.h, include/rt_hip_instance_multihit.h); instance_ao_mask_kernel<MODE> is
//                   ao_mask_kernel against them: the same rays and tail, shared functions, around instance_walk in its occlusion
//                   form (kernels/instance_directional.hip.h, include/rt_hip_instance_directional.h).
//   (scenes)        refit_leaves_kernel / refit_inner_kernel make the records and boxes of a scene again from new positions
//                   (kernels/refit.hip.h, include/rt_hip_update.h); build_boxes_kernel, build_root_kernel, build_keys_kernel,
//                   build_tree_kernel and build_layout_kernel make a scene's tree from triangles, around a sort that lives in
//                   build_sort.hip (kernels/build.hip.h, include/rt_hip_build.h); instance_inverse_kernel, instance_reach_kernel,
//                   instance_leaves_kernel, instance_root_kernel, instance_keys_kernel, instance_tree_kernel,
//                   instance_layout_kernel and instance_boxes_kernel make an instance set -- inverses, bounds, top-level tree --
//                   from transforms in device memory, around the same sort (kernels/instance_build.hip.h,
//                   include/rt_hip_instance_build.h).
//   (on demand)     entry_kernel: the walk intervals, once per upload; occluded_sum_kernel: the frame's occlusion
//                   total when the statistics are asked for; resize_kernel: a box filter on its own.
//   (tests)         node_test_forms_kernel: the any-hit node test against the form it replaced, on the caller's records and
//                   rays (kernels/node_test_forms.hip.h, include/rt_hip_debug.h).
// Why not one fused launch (it was, see profiles/r01_notes.md): cost per tile
// varies 30x (background vs model, 29 rays per hit sub-pixel), so the frame used
// to end on a long tail of half-empty CUs.  With the tiles' costs known from the
// upload's primary pass, claiming the costly blocks first packs them almost perfectly.
// (Round 5 put both ray passes into one persistent launch once more, the hit records handed from workgroup to workgroup
// inside it: bit-exact and 2-9 % slower than the two kernels, so it was taken out again -- profiles/r05_notes.md.)
//
// How rays walk the tree: the 64 rays of a wave share ONE node index ("shared
// walk", see walk_collect below) -- nodes and triangles arrive by
// scalar loads, boxes are tested out of SGPRs, nothing diverges and nothing is
// gathered.
//
// What bounds it: the scene (19 MB) is cache-resident, HBM traffic is negligible;
// the walk is bound by vector-instruction issue (11 to 17 per node and primary packet, 12 per any-hit packet) and the
// latency of the one scalar load per pair of nodes (scenes beyond the caches: by that latency alone) -- see DESIGN.md section 5 and
// profiles/r0*_notes.md for the counters and the microbenchmarks.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "device_types.h"
#include "exact_reciprocal.h"
#include "lbvh.h"
#include "instance_plan.h"
#include "nearest_point.h"
#include "signed_point.h"
#include "instance_nearest.h"
#include "tri_predicate.h"

#include "kernels/common.hip.h"
#include "kernels/walk.hip.h"
#include "kernels/primary.hip.h"
#include "kernels/ao.hip.h"
#include "kernels/entry.hip.h"
#include "kernels/finish.hip.h"
#include "kernels/query.hip.h"
#include "kernels/ao_query.hip.h"
#include "kernels/directional.hip.h"
#include "kernels/multihit.hip.h"
#include "kernels/layers.hip.h"
#include "kernels/views.hip.h"
#include "kernels/refit.hip.h"
#include "kernels/build.hip.h"
#include "kernels/instance_build.hip.h"
#include "kernels/node_test_forms.hip.h"
#include "kernels/nearest.hip.h"
#include "kernels/signed.hip.h"
#include "kernels/segment.hip.h"
#include "kernels/instances.hip.h"
#include "kernels/instance_views.hip.h"
#include "kernels/instance_segments.hip.h"
#include "kernels/instance_nearest.hip.h"
#include "kernels/instance_multihit.hip.h"
#include "kernels/instance_directional.hip.h"


namespace ocrt {

// ---- host-callable launchers (keeps the launch syntax inside this TU) ----
// Makes the runtime load this library's code object for the current device now (it is otherwise loaded at the first
// launch): called from a warm-up thread while the CPU still builds the scene.
void preload_kernels() {
	hipFuncAttributes attr;
	(void) hipFuncGetAttributes(&attr, (const void *) primary_kernel);
	(void) hipFuncGetAttributes(&attr, (const void *) ao_kernel<AO_UNIFORM, true>);
	(void) hipGetLastError();
}

#if defined(OCRT_STAMPS) || defined(OCRT_TAIL)
// (instrumented builds only: the debug stamps are sums and need zeroing; the frame's own counters do not -- device_types.h)
__global__ __launch_bounds__(256) void clear_stamps_kernel(FrameCounters *counters) {
	for (uint32_t i = threadIdx.x; i < sizeof(counters->stamp) / sizeof(counters->stamp[0]); i += blockDim.x)
		counters->stamp[i] = 0ull;
}
#endif

#ifdef OCRT_OCML_BUILTINS
// (test-only build: the UNIFORM direction table as the reference kernel computes it on the device -- per pixel, with the
// library's own float sin / cos / cospi / sinpi, src/intersect_kernel.cl:237-246 -- instead of the host's libm: the same
// expressions in the same order, one thread)
__global__ void ocml_ao_table_kernel(float4 *table, uint32_t *count, uint32_t rings, int alpha_min, int alpha_max, uint32_t capacity) {
	if (threadIdx.x != 0 || blockIdx.x != 0)
		return;
	uint32_t n = 0;
	const float degrees = (float) (M_PI / 180);
	const float amin = (float) alpha_min * degrees;
	const float amax = (float) alpha_max * degrees;
	for (uint32_t ring = 0; ring < rings; ++ring) {
		const float step = amax / rings;
		const float angle = (step * ring) + amin;
		const double rays_in_ring = (2.0f * M_PI * ocl_cos(angle)) / step;
		const uint32_t ray_count = rays_in_ring > 0.0 ? (uint32_t) rays_in_ring : 0u;  // (negative beyond 90 degrees: uniform_ao_table)
		const float theta = (float) (M_PI_2 - angle);
		for (uint32_t k = 0; k <= ray_count; ++k) {
			const float phi = (float) ((2.0f * M_PI * k) / ray_count);
			const float xs = ocl_sin(theta) * ocl_cospi(phi);
			const float ys = ocl_cos(theta);
			const float zs = ocl_sin(theta) * ocl_sinpi(phi);
			if (n < capacity)
				table[n] = make_float4(xs, ys, zs, 0.0f);
			++n;
		}
	}
	*count = n;
}
// Overwrites the `capacity` entries at `table` (device) with the device-made ones; returns how many the device counted.
uint32_t ocml_ao_table(void *table, uint32_t rings, int alpha_min, int alpha_max, uint32_t capacity) {
	uint32_t *d_count = nullptr, count = 0;
	if (hipMalloc(&d_count, sizeof(uint32_t)) != hipSuccess)
		return 0;
	hipLaunchKernelGGL(ocml_ao_table_kernel, dim3(1), dim3(64), 0, nullptr, (float4 *) table, d_count, rings, alpha_min, alpha_max, capacity);
	(void) hipDeviceSynchronize();
	(void) hipMemcpy(&count, d_count, sizeof count, hipMemcpyDeviceToHost);
	(void) hipFree(d_count);
	return count;
}
#endif

// The frame is three kernels (two without ambient occlusion): the primary pass, the ambient-occlusion pass, the
// finishing kernel (AO factor + box filter + quantisation).
#ifdef OCRT_PRIMARY_TICKS
extern void *primary_ticks_probe;
#endif
void launch_primary(const SceneBuffers &scene, float *image, void *hits, void *occluded_of, void *tile_hits,
                    const void *tile_base, void *counters, const KernelParams &P, void *stream, const void *blocks_by_cost) {
	hipStream_t s = (hipStream_t) stream;
#if defined(OCRT_STAMPS) || defined(OCRT_TAIL)
	hipLaunchKernelGGL(clear_stamps_kernel, dim3(1), dim3(256), 0, s, (FrameCounters *) counters);
#endif
	if (P.tiles_x * P.local_tile_rows == 0)
		return;
	const uint32_t strips = (P.tiles_x + P.strip_tiles - 1u) / P.strip_tiles, row_blocks = (P.local_tile_rows + PRIMARY_ROWS - 1u) / PRIMARY_ROWS;
	// (with a list -- DeviceRenderer::orderBlocksByCost -- every group's workgroups take its entries one by one)
	const uint32_t blocks = blocks_by_cost && P.primary_list_stride && PRIMARY_WAVES == 4u ? XCD_GROUPS * P.primary_list_stride
	                                                                                        : XCD_GROUPS * ((strips + XCD_GROUPS - 1u) >> 3) * row_blocks * (P.strip_tiles >> 1);
	auto launch = [&](auto kernel) {
		FrameArgs args{};
		args.walk_ptr = (const float4 *) scene.walk;
		args.tris_ptr = (const float4 *) scene.tris;
		args.nodes_ptr = (const float4 *) scene.nodes;
		args.shade = (const float4 *) scene.shade;
		args.image = image;
		args.hits = (HitRec *) hits;
		args.occluded_of = (uint32_t *) occluded_of;
		args.tile_hits = (uint32_t *) tile_hits;
		args.tile_base = (const uint32_t *) tile_base;
		args.counters = (FrameCounters *) counters;
		args.primary_order = P.primary_list_stride && PRIMARY_WAVES == 4u ? (const uint32_t *) blocks_by_cost : nullptr;  // (null: the spatial mapping)
#ifdef OCRT_PRIMARY_TICKS
		args.tile_cost = (uint32_t *) primary_ticks_probe;
#endif
		args.P = P;
		hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64 * PRIMARY_WAVES), 0, s, args);
	};
	// (a host with a camera pose: the kernel that reads the pose; the default one holds the reference's camera as constants)
	if (P.posed)
		return launch(primary_posed_kernel);
	launch(primary_kernel);
}

#ifdef OCRT_PRIMARY_TICKS
void *primary_ticks_probe = nullptr;  // (probe build: set by DeviceRenderer::measureTileCosts around its frames)
#endif

// Fills `tile_entry` (1 + ao_dirs intervals of two words per tile) for the frame whose hit list is in `hits`: once per
// upload (entry_kernel).
void launch_entries(const SceneBuffers &scene, const void *hits, const void *tile_hits, const void *tile_base, void *tile_entry,
                    const KernelParams &P, void *stream) {
	const uint32_t tiles = P.tiles_x * P.local_tile_rows;
	if (tiles == 0)
		return;
	hipLaunchKernelGGL(entry_kernel, dim3((tiles + ENTRY_WAVES - 1u) / ENTRY_WAVES), dim3(64 * ENTRY_WAVES), 0, (hipStream_t) stream,
	                   (const NodeRec *) ((const char *) scene.walk + P.walk_ce_bytes), (const HitRec *) hits, (const uint32_t *) tile_hits, (const uint32_t *) tile_base,
	                   (const float4 *) scene.ao_table, (uint2 *) tile_entry, tiles, P.entry_stride, P.ao_mode == AO_UNIFORM && scene.ao_table ? 1 : 0,
	                   P.ao_max_distance);
}

void launch_ao(const SceneBuffers &scene, void *hits, void *occluded_of, void *order, const void *tile_base, const void *tile_entry,
               void *counters, const KernelParams &params, uint32_t workgroups, bool prefetch, void *stream, void *event_before_ao,
               void *event_after_ao, void *tile_cost) {
	if (params.tiles_x * params.local_tile_rows == 0 || params.ao_mode == AO_NONE || params.ao_dirs == 0)
		return;
	hipStream_t s = (hipStream_t) stream;
	// persistent grid: what the chip holds, or one wave per (tile, direction) when the image is small
	const uint32_t tiles = params.tiles_x * params.local_tile_rows;
	const uint64_t units = (uint64_t) tiles * params.ao_dirs;
	uint32_t ao_blocks = workgroups;  // (DeviceRenderer::aoWorkgroups: 8 per CU for a host alone on its GPU)
	if ((units + AO_WAVES - 1) / AO_WAVES < ao_blocks)
		ao_blocks = (uint32_t) ((units + AO_WAVES - 1) / AO_WAVES);
	KernelParams P = params;
	const uint32_t waves_per_group = (ao_blocks * AO_WAVES + XCD_GROUPS - 1u) / XCD_GROUPS;
	P.ao_guide = P.ao_guide * (waves_per_group ? waves_per_group : 1u);
	P.ao_claim_div = waves_per_group ? waves_per_group : 1u;  // (the waves of a group, for ao_kernel's claim rule)
	auto launch = [&](auto kernel) {
		// (the events bracket the ao_kernel launch alone: its duration is the one the roofline is quoted for)
		if (event_before_ao)
			(void) hipEventRecord((hipEvent_t) event_before_ao, s);
		FrameArgs args{};
		args.walk_ptr = (const float4 *) scene.walk;
		args.tris_ptr = (const float4 *) scene.tris;
		args.nodes_ptr = (const float4 *) scene.nodes;
		args.ao_table = (const float4 *) scene.ao_table;
		args.hits = (HitRec *) hits;
		args.occluded_of = (uint32_t *) occluded_of;
		args.order = (const uint32_t *) order;
		args.tile_base = (const uint32_t *) tile_base;
		args.tile_entry = (const uint2 *) tile_entry;
		args.counters = (FrameCounters *) counters;
		args.tile_cost = (uint32_t *) tile_cost;
		args.P = P;
		hipLaunchKernelGGL(kernel, dim3(ao_blocks), dim3(64 * AO_WAVES), 0, s, args);
		if (event_after_ao)
			(void) hipEventRecord((hipEvent_t) event_after_ao, s);
	};
	if (P.ao_mode == AO_UNIFORM) {
		if (prefetch)
			launch(ao_kernel<AO_UNIFORM, true>);
		else
			launch(ao_kernel<AO_UNIFORM, false>);
	} else
		launch(ao_kernel<AO_RANDOM>);
}

// `out`: this rank's 8-bit bands (local_out_rows x out_width), or null for a frame without the device resize.
void launch_finish(float *image, const void *hits, const void *occluded_of, const void *tile_base, unsigned char *out,
                   const KernelParams &P, uint32_t out_width, uint32_t n, uint32_t local_out_rows, void *stream, void *counters) {
	if (local_out_rows == 0 || out_width == 0 || n == 0)
		return;
	const bool has_ao = P.ao_mode != AO_NONE && P.ao_dirs > 0;
	if (!has_ao && !out)
		return;  // (nothing pending, nothing to filter)
	const uint32_t rows_per_band = P.part.band_tile_rows * TILE_H / n;
	const uint32_t cells_per_pixel = (n * n) | 1u;
	if (n >= 2u && cells_per_pixel <= FINISH_CELL_FLOATS) {
		// supersampled: a workgroup per run of output pixels, swept along the sub-pixel rows (finish_wide_kernel)
		uint32_t pixels_per_block = FINISH_CELL_FLOATS / cells_per_pixel;
		pixels_per_block = pixels_per_block > 256u ? 256u : pixels_per_block > 16u ? pixels_per_block & ~15u : pixels_per_block;
		hipLaunchKernelGGL(finish_wide_kernel<true>, dim3((out_width + pixels_per_block - 1u) / pixels_per_block, local_out_rows), dim3(256), 0,
		                   (hipStream_t) stream, image, (const HitRec *) hits, (const uint32_t *) occluded_of, (const uint32_t *) tile_base,
		                   out, out_width, P.height / n, P.width, n, P.tiles_x, P.part, rows_per_band,
		                   P.ao_divisor ? P.ao_divisor : 1u, pixels_per_block, (FrameCounters *) counters);
		return;
	}
	hipLaunchKernelGGL(finish_kernel, dim3((out_width + 255) / 256, local_out_rows), dim3(256), 0, (hipStream_t) stream, image,
	                   (const HitRec *) hits, (const uint32_t *) occluded_of, (const uint32_t *) tile_base, out,
	                   out_width, P.height / n,
	                   P.width, n, P.tiles_x, P.part, rows_per_band, P.ao_divisor ? P.ao_divisor : 1u, (FrameCounters *) counters);
}

// counters->occluded = the sum of the hit list's `slots` occlusion counts (stream-ordered: after the frames enqueued so far).
void launch_occluded_sum(const void *occluded_of, size_t slots, void *counters, void *stream) {
	FrameCounters *const c = (FrameCounters *) counters;
	(void) hipMemsetAsync(&c->occluded, 0, sizeof c->occluded, (hipStream_t) stream);
	if (slots == 0)
		return;
	const size_t blocks = (slots + 4095) / 4096;  // (16 counts per thread at least)
	hipLaunchKernelGGL(occluded_sum_kernel, dim3((unsigned) (blocks < 256 ? blocks : 256)), dim3(256), 0, (hipStream_t) stream,
	                   (const uint32_t *) occluded_of, slots, c);
}

void launch_resize(const float *tmp, unsigned char *out, const KernelParams &P, uint32_t out_width, uint32_t n,
                   uint32_t local_out_rows, void *stream) {
	if (local_out_rows == 0 || out_width == 0 || n == 0)
		return;
	const uint32_t rows_per_band = P.part.band_tile_rows * TILE_H / n;
	const uint32_t cells_per_pixel = (n * n) | 1u;
	if (n >= 2u && cells_per_pixel <= FINISH_CELL_FLOATS) {
		// supersampled: along the sub-pixel rows, like the frame's own finishing sweep (no tags to resolve, nothing written back)
		uint32_t pixels_per_block = FINISH_CELL_FLOATS / cells_per_pixel;
		pixels_per_block = pixels_per_block > 256u ? 256u : pixels_per_block > 16u ? pixels_per_block & ~15u : pixels_per_block;
		hipLaunchKernelGGL(finish_wide_kernel<false>, dim3((out_width + pixels_per_block - 1u) / pixels_per_block, local_out_rows), dim3(256), 0,
		                   (hipStream_t) stream, const_cast<float *>(tmp), (const HitRec *) nullptr, (const uint32_t *) nullptr,
		                   (const uint32_t *) nullptr, out, out_width, P.height / n, P.width, n, P.tiles_x, P.part, rows_per_band, 1u,
		                   pixels_per_block, (FrameCounters *) nullptr);
		return;
	}
	hipLaunchKernelGGL(resize_kernel, dim3((out_width + 255) / 256, local_out_rows), dim3(256), 0,
	                   (hipStream_t) stream, tmp, out, out_width, P.height / n, P.width, n, P.part, rows_per_band);
}

// Ray queries (kernels/query.hip.h).  `count`: QUERY_BUCKETS words of scratch, `order`: n words; both on the device.
// `segments`: the two arrays are the ends (a, b) of segments, keyed as the rays (a, b - a) (kernels/segment.hip.h).
void launch_query_sort(const void *origins, const void *directions, uint32_t n, const float lo[3], const float scale[3], void *count,
                       void *order, void *stream, bool segments) {
	if (n == 0)
		return;
	hipStream_t s = (hipStream_t) stream;
	QueryKeyArgs a{};
	a.origins = (const float4 *) origins;
	a.directions = (const float4 *) directions;
	a.count = (uint32_t *) count;
	a.order = (uint32_t *) order;
	a.n = n;
	for (int k = 0; k < 3; ++k) {
		a.lo[k] = lo[k];
		a.scale[k] = scale[k];
	}
	(void) hipMemsetAsync(count, 0, QUERY_BUCKETS * sizeof(uint32_t), s);
	const uint32_t blocks = (n + 255u) / 256u;
	const auto key_kernel = segments ? segment_key_kernel : query_key_kernel;
	const auto scatter_kernel = segments ? segment_scatter_kernel : query_scatter_kernel;
	hipLaunchKernelGGL(key_kernel, dim3(blocks), dim3(256), 0, s, a);
	hipLaunchKernelGGL(query_scan_kernel, dim3(1), dim3(QUERY_SCAN_THREADS), 0, s, (uint32_t *) count);
	hipLaunchKernelGGL(scatter_kernel, dim3(blocks), dim3(256), 0, s, a);
}

// (the instance set as the kernels take it)
static InstanceSet instance_set(const InstanceBuffers &set) {
	return InstanceSet{ (const float4 *) set.top, (const float4 *) set.inverses, set.top_count };
}

// (what query_kernel, instance_kernel and the multi-hit kernels are launched with alike)
static void fill(RayQueryArgs &a, const SceneBuffers &scene, uint32_t node_count, const void *origins, const void *directions,
                 const void *order, uint32_t n, float max_distance, const RecordOutputs &out) {
	a.nodes_ptr = (const float4 *) scene.nodes;
	a.tris_ptr = (const float4 *) scene.tris;
	a.shade = (const float4 *) scene.shade;
	a.origins = (const float4 *) origins;
	a.directions = (const float4 *) directions;
	a.order = (const uint32_t *) order;
	a.n = n;
	a.node_count = node_count;
	a.max_distance = max_distance;
	a.out = out;
}

// `set`: null, or the instance set the rays are cast against (kernels/instances.hip.h), `instance` beside the closest form's
// record; the sort is then keyed over the top-level root box.  `closest` false: occlusion into out.hit alone.
void launch_query(const SceneBuffers &scene, uint32_t node_count, const InstanceBuffers *set, bool closest, const void *origins,
                  const void *directions, const void *order, uint32_t n, float max_distance, const QueryOutputs &out, uint32_t *instance,
                  void *stream) {
	if (n == 0 || (set && set->top_count == 0))
		return;
	const uint32_t blocks = (n + 64u * QUERY_WAVES - 1u) / (64u * QUERY_WAVES);
	if (set) {
		InstanceArgs a{};
		fill(a, scene, node_count, origins, directions, order, n, max_distance, out);
		a.set = instance_set(*set);
		a.hit = out.hit;
		a.instance = instance;
		if (closest)
			hipLaunchKernelGGL(instance_kernel<true>, dim3(blocks), dim3(64 * QUERY_WAVES), 0, (hipStream_t) stream, a);
		else
			hipLaunchKernelGGL(instance_kernel<false>, dim3(blocks), dim3(64 * QUERY_WAVES), 0, (hipStream_t) stream, a);
		return;
	}
	QueryArgs a{};
	fill(a, scene, node_count, origins, directions, order, n, max_distance, out);
	a.hit = out.hit;
	if (closest) {
		hipLaunchKernelGGL(query_kernel<true>, dim3(blocks), dim3(64 * QUERY_WAVES), 0, (hipStream_t) stream, a);
	} else {
		hipLaunchKernelGGL(query_kernel<false>, dim3(blocks), dim3(64 * QUERY_WAVES), 0, (hipStream_t) stream, a);
	}
}

// Closest-point queries (kernels/nearest.hip.h).  The sort: launch_query_sort's with a key of the position alone.
void launch_nearest_sort(const void *points, uint32_t n, const float lo[3], const float scale[3], void *count, void *order, void *stream) {
	if (n == 0)
		return;
	hipStream_t s = (hipStream_t) stream;
	NearestKeyArgs a{};
	a.points = (const float4 *) points;
	a.count = (uint32_t *) count;
	a.order = (uint32_t *) order;
	a.n = n;
	for (int k = 0; k < 3; ++k) {
		a.lo[k] = lo[k];
		a.scale[k] = scale[k];
	}
	(void) hipMemsetAsync(count, 0, QUERY_BUCKETS * sizeof(uint32_t), s);
	const uint32_t blocks = (n + 255u) / 256u;
	hipLaunchKernelGGL(nearest_key_kernel, dim3(blocks), dim3(256), 0, s, a);
	hipLaunchKernelGGL(query_scan_kernel, dim3(1), dim3(QUERY_SCAN_THREADS), 0, s, (uint32_t *) count);
	hipLaunchKernelGGL(nearest_scatter_kernel, dim3(blocks), dim3(256), 0, s, a);
}

// `flag`: one word on the device, set to 1 where a coordinate of `vertices4` (float4 each) is no number or beyond 1e37.
void launch_nearest_coordinates(const void *vertices4, uint32_t num_vertices, void *flag, void *stream) {
	(void) hipMemsetAsync(flag, 0, sizeof(uint32_t), (hipStream_t) stream);
	if (num_vertices == 0)
		return;
	hipLaunchKernelGGL(nearest_coordinates_kernel, dim3((num_vertices + 255u) / 256u), dim3(256), 0, (hipStream_t) stream,
	                   (const float4 *) vertices4, num_vertices, (uint32_t *) flag);
}

// `walk`: NEAREST_START | NEAREST_PRUNE as far as the scene allows them (ray_query.cc); `coords_flag`: that word, or null:
// the host has seen the scene's coordinates; `counts`: two 64-bit words on the device, zeroed here on the stream, for the
// counted form -- or null: the product's form.  `set`: null, or the instance set the points are held against
// (kernels/instance_nearest.hip.h), `instance` beside the record.
static void fill(NearestArgs &a, const SceneBuffers &scene, uint32_t node_count, uint32_t tri_count, const void *points, const void *order,
                 uint32_t n, float max_distance, uint32_t walk, const QueryOutputs &out, const void *coords_flag, void *counts) {
	a.coords_flag = (const uint32_t *) coords_flag;
	a.nodes_ptr = (const float4 *) scene.nodes;
	a.tris_ptr = (const float4 *) scene.tris;
	a.shade = (const float4 *) scene.shade;
	a.points = (const float4 *) points;
	a.order = (const uint32_t *) order;
	a.n = n;
	a.node_count = node_count;
	a.tri_count = tri_count;
	a.max_distance = max_distance;
	a.walk = walk;
	a.out = out;
	a.hit = out.hit;
	a.counts = (unsigned long long *) counts;
}

void launch_nearest(const SceneBuffers &scene, uint32_t node_count, uint32_t tri_count, const InstanceBuffers *set, const void *points,
                    const void *order, uint32_t n, float max_distance, uint32_t walk, const QueryOutputs &out, uint32_t *instance,
                    const void *coords_flag, void *counts, void *stream) {
	if (n == 0 || (set && set->top_count == 0))
		return;
	const uint32_t blocks = (n + 64u * NEAREST_WAVES - 1u) / (64u * NEAREST_WAVES);
	if (counts)
		(void) hipMemsetAsync(counts, 0, 2u * sizeof(unsigned long long), (hipStream_t) stream);
	if (set) {
		InstanceNearestArgs a{};
		fill(a, scene, node_count, tri_count, points, order, n, max_distance, walk, out, coords_flag, counts);
		a.set = instance_set(*set);
		a.world = (const float4 *) set->world;
		a.bounds = (const float4 *) set->bounds;
		a.instance = instance;
		if (counts)
			hipLaunchKernelGGL(instance_nearest_kernel<true>, dim3(blocks), dim3(64 * NEAREST_WAVES), 0, (hipStream_t) stream, a);
		else
			hipLaunchKernelGGL(instance_nearest_kernel<false>, dim3(blocks), dim3(64 * NEAREST_WAVES), 0, (hipStream_t) stream, a);
		return;
	}
	NearestArgs a{};
	fill(a, scene, node_count, tri_count, points, order, n, max_distance, walk, out, coords_flag, counts);
	if (counts) {
		hipLaunchKernelGGL(nearest_kernel<true>, dim3(blocks), dim3(64 * NEAREST_WAVES), 0, (hipStream_t) stream, a);
	} else {
		hipLaunchKernelGGL(nearest_kernel<false>, dim3(blocks), dim3(64 * NEAREST_WAVES), 0, (hipStream_t) stream, a);
	}
}

// Signed distance queries (kernels/signed.hip.h).  The table's pieces, in the order ray_query.cc runs them: the sorts' inputs
// of the 3 tri_count corners; (sign_sort.hip's sorts;) the kept incidence words out of a sort's result; the sums and the
// per-leaf words, which are all an update redoes.
void launch_sign_keys(const void *faces, uint32_t tri_count, void *vertex_keys, void *edge_keys, void *values, void *stream) {
	const uint32_t corners = 3u * tri_count;
	if (corners == 0)
		return;
	hipLaunchKernelGGL(sign_keys_kernel, dim3((corners + 255u) / 256u), dim3(256), 0, (hipStream_t) stream, (const uint32_t *) faces, corners,
	                   (uint32_t *) vertex_keys, (unsigned long long *) edge_keys, (uint32_t *) values);
}

void launch_sign_heads(bool wide, const void *sorted_keys, const void *sorted_values, uint32_t tri_count, void *kept, void *stream) {
	const uint32_t corners = 3u * tri_count;
	if (corners == 0)
		return;
	if (wide)
		hipLaunchKernelGGL(sign_heads_kernel<unsigned long long>, dim3((corners + 255u) / 256u), dim3(256), 0, (hipStream_t) stream,
		                   (const unsigned long long *) sorted_keys, (const uint32_t *) sorted_values, corners, (uint32_t *) kept);
	else
		hipLaunchKernelGGL(sign_heads_kernel<uint32_t>, dim3((corners + 255u) / 256u), dim3(256), 0, (hipStream_t) stream,
		                   (const uint32_t *) sorted_keys, (const uint32_t *) sorted_values, corners, (uint32_t *) kept);
}

void launch_sign_sums(const void *kept_vertices, const void *kept_edges, const SceneBuffers &scene, uint32_t tri_count, void *table, void *stream) {
	const uint32_t corners = 3u * tri_count;
	if (corners == 0)
		return;
	hipStream_t s = (hipStream_t) stream;
	hipLaunchKernelGGL(sign_leaf_kernel, dim3((tri_count + 255u) / 256u), dim3(256), 0, s, (const float4 *) scene.tris, tri_count, (float4 *) table);
	hipLaunchKernelGGL(sign_sum_kernel<false>, dim3((corners + 255u) / 256u), dim3(256), 0, s, (const uint32_t *) kept_vertices, corners,
	                   (const float4 *) scene.tris, tri_count, (float4 *) table);
	hipLaunchKernelGGL(sign_sum_kernel<true>, dim3((corners + 255u) / 256u), dim3(256), 0, s, (const uint32_t *) kept_edges, corners,
	                   (const float4 *) scene.tris, tri_count, (float4 *) table);
}

// The point form: launch_nearest's arguments, the table, and the two outputs of its own.
void launch_signed(const SceneBuffers &scene, uint32_t node_count, uint32_t tri_count, const void *points, const void *order, uint32_t n,
                   float max_distance, uint32_t walk, const QueryOutputs &out, uint8_t *feature, float *pseudonormal4, const void *table,
                   const void *coords_flag, void *stream) {
	if (n == 0)
		return;
	SignedArgs a{};
	fill(a.nearest, scene, node_count, tri_count, points, order, n, max_distance, walk, out, coords_flag, nullptr);
	a.table = (const float4 *) table;
	a.feature = feature;
	a.pseudonormal = (float4 *) pseudonormal4;
	const uint32_t blocks = (n + 64u * NEAREST_WAVES - 1u) / (64u * NEAREST_WAVES);
	hipLaunchKernelGGL(signed_kernel, dim3(blocks), dim3(64 * NEAREST_WAVES), 0, (hipStream_t) stream, a);
}

// The grid form over the slab of `nz` slices from `z_first` on: `distance`, `leaf` hold [nz][ny][nx] (either may be null).
void launch_signed_grid(const SceneBuffers &scene, uint32_t node_count, uint32_t tri_count, const float origin[3], const float spacing[3],
                        uint32_t nx, uint32_t ny, uint32_t nz, uint32_t z_first, float max_distance, uint32_t walk, float *distance,
                        uint32_t *leaf, const void *table, const void *coords_flag, void *stream) {
	if (nx == 0 || ny == 0 || nz == 0)
		return;
	SignedGridArgs a{};
	fill(a.nearest, scene, node_count, tri_count, nullptr, nullptr, 0u, max_distance, walk, QueryOutputs{}, coords_flag, nullptr);
	a.table = (const float4 *) table;
	for (int k = 0; k < 3; ++k) {
		a.origin[k] = origin[k];
		a.spacing[k] = spacing[k];
	}
	a.nx = nx; a.ny = ny; a.nz = nz; a.z_first = z_first;
	a.bricks_x = (nx + 3u) / 4u;
	a.bricks_y = (ny + 3u) / 4u;
	const uint64_t bricks = (uint64_t) a.bricks_x * a.bricks_y * ((nz + 3u) / 4u);  // (at most 2^31 voxels: fewer bricks than 2^31)
	a.bricks = (uint32_t) bricks;
	a.distance = distance;
	a.leaf = leaf;
	const uint32_t blocks = (a.bricks + NEAREST_WAVES - 1u) / NEAREST_WAVES;
	hipLaunchKernelGGL(signed_grid_kernel, dim3(blocks), dim3(64 * NEAREST_WAVES), 0, (hipStream_t) stream, a);
}

// Segment queries (kernels/segment.hip.h); their sort is launch_query_sort's with `segments`.  `set`, `instance`: as for
// launch_query (kernels/instance_segments.hip.h).  `closest` false: occlusion into out.hit alone.
void launch_segments(const SceneBuffers &scene, uint32_t node_count, const InstanceBuffers *set, bool closest, const void *from, const void *to,
                     const void *order, uint32_t n, float t_lo, float t_hi, const QueryOutputs &out, uint32_t *instance, void *stream) {
	if (n == 0 || (set && set->top_count == 0))
		return;
	InstanceSegmentArgs a{};
	a.nodes_ptr = (const float4 *) scene.nodes;
	a.tris_ptr = (const float4 *) scene.tris;
	a.shade = (const float4 *) scene.shade;
	a.from = (const float4 *) from;
	a.to = (const float4 *) to;
	a.order = (const uint32_t *) order;
	a.n = n;
	a.node_count = node_count;
	a.t_lo = t_lo;
	a.t_hi = t_hi;
	a.out = out;
	a.hit = out.hit;
	const SegmentArgs &plain = a;
	const dim3 blocks((n + 64u * QUERY_WAVES - 1u) / (64u * QUERY_WAVES)), lanes(64 * QUERY_WAVES);
	if (set) {
		a.set = instance_set(*set);
		a.instance = instance;
		if (closest)
			hipLaunchKernelGGL(instance_segment_kernel<true>, blocks, lanes, 0, (hipStream_t) stream, a);
		else
			hipLaunchKernelGGL(instance_segment_kernel<false>, blocks, lanes, 0, (hipStream_t) stream, a);
	} else if (closest) {
		hipLaunchKernelGGL(segment_kernel<true>, blocks, lanes, 0, (hipStream_t) stream, plain);
	} else {
		hipLaunchKernelGGL(segment_kernel<false>, blocks, lanes, 0, (hipStream_t) stream, plain);
	}
}

// The many-to-many form.  `mask`: np rows of ceil(nt / 32) words on the device (the caller's array or scratch), zeroed here
// on the stream; `order`: launch_nearest_sort's order of the POINTS or null; `count`: null = not written; `set`: null, or
// the instance set the segments are cast against.
void launch_visibility(const SceneBuffers &scene, uint32_t node_count, const InstanceBuffers *set, const void *points, uint32_t np,
                       const void *targets, uint32_t nt, const void *order, float t_lo, float t_hi, uint32_t *mask, uint32_t *count,
                       void *stream) {
	if (np == 0 || nt == 0 || (set && set->top_count == 0))
		return;
	hipStream_t s = (hipStream_t) stream;
	InstanceVisibilityArgs a{};
	a.nodes_ptr = (const float4 *) scene.nodes;
	a.tris_ptr = (const float4 *) scene.tris;
	a.points = (const float4 *) points;
	a.targets = (const float4 *) targets;
	a.order = (const uint32_t *) order;
	a.mask = mask;
	a.np = np;
	a.nt = nt;
	a.words = (nt + 31u) / 32u;
	a.total = np * nt;  // (<= RT_QUERY_MAX_RAYS: checked at the boundary)
	visibility_divisor(nt, a.magic, a.shift);
	a.node_count = node_count;
	a.t_lo = t_lo;
	a.t_hi = t_hi;
	(void) hipMemsetAsync(mask, 0, (size_t) np * a.words * sizeof(uint32_t), s);
	const uint32_t blocks = (a.total + 64u * QUERY_WAVES - 1u) / (64u * QUERY_WAVES);
	if (set) {
		a.set = instance_set(*set);
		hipLaunchKernelGGL(instance_visibility_kernel, dim3(blocks), dim3(64 * QUERY_WAVES), 0, s, a);
	} else {
		const VisibilityArgs &plain = a;
		hipLaunchKernelGGL(visibility_mask_kernel, dim3(blocks), dim3(64 * QUERY_WAVES), 0, s, plain);
	}
	if (count)
		hipLaunchKernelGGL(visibility_count_kernel, dim3((np + 255u) / 256u), dim3(256), 0, s, (const uint32_t *) mask, count, np, a.words);
}

// Ambient-occlusion queries (kernels/ao_query.hip.h).  `count`: n words on the device (the caller's `occluded` array or
// scratch), zeroed here on the stream; `order`: launch_query_sort's order of the POINTS or null; `ao`: null = not written;
// `set`: null, or the instance set the rays are cast against (kernels/instance_views.hip.h).
void launch_ao_query(const SceneBuffers &scene, uint32_t node_count, const InstanceBuffers *set, int ao_mode, uint32_t rays_per_point,
                     uint32_t divisor, float max_distance, const void *points, const void *normals, const uint32_t *seeds, const void *order,
                     uint32_t n, uint32_t *count, float *ao, void *stream) {
	if (n == 0 || rays_per_point == 0 || (set && set->top_count == 0))
		return;
	hipStream_t s = (hipStream_t) stream;
	InstanceAoArgs a{};
	a.nodes_ptr = (const float4 *) scene.nodes;
	a.tris_ptr = (const float4 *) scene.tris;
	a.ao_table = (const float4 *) scene.ao_table;
	a.points = (const float4 *) points;
	a.normals = (const float4 *) normals;
	a.seeds = seeds;
	a.order = (const uint32_t *) order;
	a.count = count;
	a.n = n;
	a.rays = rays_per_point;
	a.total = n * rays_per_point;  // (<= RT_QUERY_MAX_RAYS: checked at the boundary)
	a.node_count = node_count;
	a.max_distance = max_distance;
	const AoQueryArgs &plain = a;
	(void) hipMemsetAsync(count, 0, (size_t) n * sizeof(uint32_t), s);
	const dim3 blocks((a.total + 64u * QUERY_WAVES - 1u) / (64u * QUERY_WAVES)), lanes(64 * QUERY_WAVES);
	if (set) {
		a.set = instance_set(*set);
		if (ao_mode == AO_RANDOM)
			hipLaunchKernelGGL(instance_ao_kernel<AO_RANDOM>, blocks, lanes, 0, s, a);
		else
			hipLaunchKernelGGL(instance_ao_kernel<AO_UNIFORM>, blocks, lanes, 0, s, a);
	} else if (ao_mode == AO_RANDOM) {
		hipLaunchKernelGGL(ao_query_kernel<AO_RANDOM>, blocks, lanes, 0, s, plain);
	} else {
		hipLaunchKernelGGL(ao_query_kernel<AO_UNIFORM>, blocks, lanes, 0, s, plain);
	}
	if (ao)
		hipLaunchKernelGGL(ao_query_finish_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, (const uint32_t *) count, ao, n,
		                   divisor ? divisor : 1u);
}

// Directional occlusion queries (kernels/directional.hip.h).  `mask`: n rows of ceil(rays_per_point / 32) words on the
// device (the caller's array or scratch), zeroed here on the stream; `order`: launch_query_sort's order of the POINTS or
// null; `occluded`, `ao`, `bent`: null = not written -- with all three null the resolve is not launched; `set`: null, or the
// instance set the rays are cast against (kernels/instance_directional.hip.h).
void launch_ao_directional(const SceneBuffers &scene, uint32_t node_count, const InstanceBuffers *set, int ao_mode, uint32_t rays_per_point, uint32_t divisor,
                           float max_distance, const void *points, const void *normals, const uint32_t *seeds, const void *order, uint32_t n,
                           uint32_t *mask, uint32_t *occluded, float *ao, float *bent, void *stream) {
	if (n == 0 || rays_per_point == 0 || (set && set->top_count == 0))
		return;
	hipStream_t s = (hipStream_t) stream;
	InstanceAoMaskArgs a{};
	a.nodes_ptr = (const float4 *) scene.nodes;
	a.tris_ptr = (const float4 *) scene.tris;
	a.ao_table = (const float4 *) scene.ao_table;
	a.points = (const float4 *) points;
	a.normals = (const float4 *) normals;
	a.seeds = seeds;
	a.order = (const uint32_t *) order;
	a.mask = mask;
	a.n = n;
	a.rays = rays_per_point;
	a.words = (rays_per_point + 31u) / 32u;
	a.total = n * rays_per_point;  // (<= RT_QUERY_MAX_RAYS: checked at the boundary)
	a.node_count = node_count;
	a.max_distance = max_distance;
	(void) hipMemsetAsync(mask, 0, (size_t) n * a.words * sizeof(uint32_t), s);
	const AoMaskArgs &plain = a;
	const uint32_t blocks = (a.total + 64u * QUERY_WAVES - 1u) / (64u * QUERY_WAVES);
	if (set) {
		a.set = instance_set(*set);
		if (ao_mode == AO_RANDOM)
			hipLaunchKernelGGL(instance_ao_mask_kernel<AO_RANDOM>, dim3(blocks), dim3(64 * QUERY_WAVES), 0, s, a);
		else
			hipLaunchKernelGGL(instance_ao_mask_kernel<AO_UNIFORM>, dim3(blocks), dim3(64 * QUERY_WAVES), 0, s, a);
	} else if (ao_mode == AO_RANDOM) {
		hipLaunchKernelGGL(ao_mask_kernel<AO_RANDOM>, dim3(blocks), dim3(64 * QUERY_WAVES), 0, s, plain);
	} else {
		hipLaunchKernelGGL(ao_mask_kernel<AO_UNIFORM>, dim3(blocks), dim3(64 * QUERY_WAVES), 0, s, plain);
	}
	if (!occluded && !ao && !bent)
		return;
	AoResolveArgs f{};
	f.mask = mask;
	f.ao_table = a.ao_table;
	f.points = a.points;
	f.normals = a.normals;
	f.seeds = seeds;
	f.occluded = occluded;
	f.ao = ao;
	f.bent = bent;
	f.n = n;
	f.rays = rays_per_point;
	f.words = a.words;
	f.ao_divisor = divisor ? divisor : 1u;
	if (ao_mode == AO_RANDOM)
		hipLaunchKernelGGL(ao_directional_finish_kernel<AO_RANDOM>, dim3((n + 255u) / 256u), dim3(256), 0, s, f);
	else
		hipLaunchKernelGGL(ao_directional_finish_kernel<AO_UNIFORM>, dim3((n + 255u) / 256u), dim3(256), 0, s, f);
}

// The rays of an ambient-occlusion query, written out (kernels/directional.hip.h): `origins` float4[n], `directions`
// float4[n * rays_per_point]; null = not written.
void launch_ao_rays(const SceneBuffers &scene, int ao_mode, uint32_t rays_per_point, const void *points, const void *normals,
                    const uint32_t *seeds, uint32_t n, void *origins, void *directions, void *stream) {
	if (n == 0 || rays_per_point == 0 || (!origins && !directions))
		return;
	AoRaysArgs a{};
	a.ao_table = (const float4 *) scene.ao_table;
	a.points = (const float4 *) points;
	a.normals = (const float4 *) normals;
	a.seeds = seeds;
	a.origins = (float4 *) origins;
	a.directions = (float4 *) directions;
	a.rays = rays_per_point;
	a.total = n * rays_per_point;  // (<= RT_QUERY_MAX_RAYS: checked at the boundary)
	const uint32_t blocks = (a.total + 255u) / 256u;
	if (ao_mode == AO_RANDOM)
		hipLaunchKernelGGL(ao_rays_kernel<AO_RANDOM>, dim3(blocks), dim3(256), 0, (hipStream_t) stream, a);
	else
		hipLaunchKernelGGL(ao_rays_kernel<AO_UNIFORM>, dim3(blocks), dim3(256), 0, (hipStream_t) stream, a);
}

// Multi-hit queries (kernels/multihit.hip.h).  `k` <= MULTIHIT_MAX_K slots per ray (0: the count alone); `list`: n * k
// uint2 of scratch on the device; `count` and the slot arrays: null = not written.  The resolve pass is launched only if
// a slot array is given.  `set`: null, or the instance set the rays are cast against (kernels/instance_multihit.hip.h):
// `list` is then n * k * 3 words, and `instance` the slot array beside the record's.
template <uint32_t K>
static void launch_multihit_walk(const InstanceMultiHitArgs &a, bool instanced, dim3 blocks, dim3 lanes, hipStream_t s) {
	const MultiHitArgs &plain = a;
	if (instanced)
		hipLaunchKernelGGL(instance_multihit_walk_kernel<K>, blocks, lanes, 0, s, a);
	else
		hipLaunchKernelGGL(multihit_walk_kernel<K>, blocks, lanes, 0, s, plain);
}

void launch_multihit(const SceneBuffers &scene, uint32_t node_count, const InstanceBuffers *set, const void *origins, const void *directions,
                     const void *order, uint32_t n, float max_distance, uint32_t k, void *list, const MultiHitOutputs &out, uint32_t *instance,
                     void *stream) {
	if (n == 0 || k > MULTIHIT_MAX_K || (set && set->top_count == 0))
		return;
	hipStream_t s = (hipStream_t) stream;
	InstanceMultiHitArgs a{};
	fill(a, scene, node_count, origins, directions, order, n, max_distance, out);
	a.k = k;
	a.list = (uint32_t *) list;
	a.count = out.count;
	if (set) {
		a.set = instance_set(*set);
		a.instance = instance;
	}
	const bool instanced = set != nullptr;
	const dim3 blocks((n + MULTIHIT_LANES - 1u) / MULTIHIT_LANES), lanes(MULTIHIT_LANES);
	if (k == 0u)
		launch_multihit_walk<0u>(a, instanced, blocks, lanes, s);
	else if (k == 1u)
		launch_multihit_walk<1u>(a, instanced, blocks, lanes, s);
	else if (k <= 2u)
		launch_multihit_walk<2u>(a, instanced, blocks, lanes, s);
	else if (k <= 4u)
		launch_multihit_walk<4u>(a, instanced, blocks, lanes, s);
	else if (k <= 8u)
		launch_multihit_walk<8u>(a, instanced, blocks, lanes, s);
	else
		launch_multihit_walk<16u>(a, instanced, blocks, lanes, s);
	if (k == 0u || !(out.anySlot() || (set && instance)))
		return;
	const MultiHitArgs &plain = a;
	if (set)
		hipLaunchKernelGGL(instance_multihit_resolve_kernel, dim3((n * k + 255u) / 256u), dim3(256), 0, s, a);
	else
		hipLaunchKernelGGL(multihit_resolve_kernel, dim3((n * k + 255u) / 256u), dim3(256), 0, s, plain);
}

// The list of a chunk's hit sub-pixels from the flags its ray kernel left (kernels/views.hip.h): m = the chunk's sub-pixels.
static void launch_views_list(const ViewList &list, uint32_t m, hipStream_t s) {
	const uint32_t scans = (m + VIEWS_SCAN - 1u) / VIEWS_SCAN;  // (m <= RT_QUERY_MAX_RAYS: RayQueries::viewsPerChunk)
	hipLaunchKernelGGL(views_count_kernel, dim3(scans), dim3(VIEWS_SCAN), 0, s, (const uint8_t *) list.flags, list.sums, m);
	hipLaunchKernelGGL(views_scan_sums_kernel, dim3(1), dim3(VIEWS_SUMS), 0, s, list.sums, scans, list.listed);
	hipLaunchKernelGGL(views_order_kernel, dim3(scans), dim3(VIEWS_SCAN), 0, s, (const uint8_t *) list.flags, (const uint32_t *) list.sums,
	                   list.order, m);
}

// Frame layers and multi-view rendering (kernels/layers.hip.h, kernels/views.hip.h): the frame's own rays of `views`
// views.  `out`: the blocks of the first view.  The poses: `poses`, on the device, or -- null -- `pose` for every view (a
// layers call: one view), which only a `posed` host reads: without a pose the kernel holds the reference's camera as
// constants.  `value`: where the head-light term goes once more (no ambient-occlusion step) or null.  `list`: null = no
// such step follows; else its points and normals get the step's entries, and with list->flags -- listing -- only the hit
// sub-pixels do: their flags, seeds, order and, in *list->listed, their number, and `ao`, `product` the missed ones' 1 and 0.
// `set`: null, or the instance set the rays are cast against (kernels/instance_views.hip.h: `poses` on the device, always
// listing where `list` is given), `instance` its layer beside the others.
void launch_layers(const SceneBuffers &scene, const KernelParams &P, const InstanceBuffers *set, const void *poses, const CameraPose &pose,
                   bool posed, uint32_t views, const LayerOutputs &out, uint32_t *instance, float *value, float *ao, float *product,
                   const ViewList *list, void *stream) {
	InstanceLayersArgs a{};
	a.nodes_ptr = (const float4 *) scene.nodes;
	a.tris_ptr = (const float4 *) scene.tris;
	a.shade_recs = (const float4 *) scene.shade;
	a.width = P.width;
	a.height = P.height;
	a.tiles_x = (P.width + TILE_W - 1u) / TILE_W;
	a.tiles = a.tiles_x * ((P.height + TILE_H - 1u) / TILE_H);
	a.node_count = P.node_count;
	a.shading = P.shading;
	a.a = P.a;
	a.half_w = P.half_w;
	a.half_h = P.half_h;
	a.pose = pose;
	a.poses = (const CameraPose *) poses;
	a.n = P.width * P.height;
	a.hit = out.hit;
	a.out = out;
	a.direction = out.direction;
	a.shade = out.shade;
	a.value = value;
	if (views == 0 || a.tiles == 0 || (set && (set->top_count == 0 || !poses)))
		return;
	hipStream_t s = (hipStream_t) stream;
	if (list) {
		a.points = (float4 *) list->points;
		a.normals = (float4 *) list->normals;
		a.flags = list->flags;
		a.seeds = list->seeds;
		a.ao = ao;
		a.product = product;
	}
	const dim3 blocks((a.tiles + LAYERS_WAVES - 1u) / LAYERS_WAVES, views), lanes(64 * LAYERS_WAVES);  // (views <= 65535: RayQueries::viewsPerChunk)
	const LayersArgs &plain = a;
	if (set) {
		a.set = instance_set(*set);
		a.instance = instance;
		hipLaunchKernelGGL(instance_layers_kernel, blocks, lanes, 0, s, a);
	} else if (poses) {
		hipLaunchKernelGGL((layers_kernel<true, true>), blocks, lanes, 0, s, plain);
	} else if (posed) {
		hipLaunchKernelGGL((layers_kernel<true, false>), blocks, lanes, 0, s, plain);
	} else {
		hipLaunchKernelGGL((layers_kernel<false, false>), blocks, lanes, 0, s, plain);
	}
	if (list && list->flags)
		launch_views_list(*list, views * a.n, s);
}

// ... the factors of the step's `listed` entries, from its counts, to where they belong: list.order[j], or sub-pixel j
// itself where there is no order (`ao`, `product`: either may be null) ...
void launch_views_scatter(const ViewList &list, const uint32_t *count, uint32_t divisor, float *ao, float *product, uint32_t listed,
                          void *stream) {
	if (listed == 0 || (!ao && !product))
		return;
	hipLaunchKernelGGL(views_scatter_kernel, dim3((listed + 255u) / 256u), dim3(256), 0, (hipStream_t) stream, (const float4 *) list.normals,
	                   count, (const uint32_t *) list.order, ao, product, listed, divisor ? divisor : 1u);
}

// ... and the 8-bit images of `views` float images that lie back to back at `value`, n x n sub-pixels per pixel.
void launch_views_resize(const float *value, unsigned char *image, const KernelParams &P, uint32_t out_width, uint32_t out_height,
                         uint32_t n, uint32_t views, void *stream) {
	if (views == 0 || out_width == 0 || out_height == 0 || n == 0)
		return;
	hipLaunchKernelGGL(views_resize_kernel, dim3((out_width + 255u) / 256u, out_height, views), dim3(256), 0, (hipStream_t) stream, value,
	                   image, out_width, out_height, P.width, n, P.width * P.height);
}

// Vertex updates (kernels/refit.hip.h, include/rt_hip_update.h): the leaf records and leaf boxes of `leaves` leaves from
// the new positions (`vnormals4` null: the ShadeRecs stay) ...
void launch_refit_leaves(const void *faces, const void *leaf_nodes, const void *vertices4, const void *vnormals4, void *tris, void *shade,
                         void *nodes, uint32_t leaves, void *stream) {
	if (leaves == 0)
		return;
	RefitLeafArgs a{};
	a.faces = (const uint32_t *) faces;
	a.leaf_node = (const uint32_t *) leaf_nodes;
	a.vertices = (const float4 *) vertices4;
	a.vnormals = (const float4 *) vnormals4;
	a.tris = (float4 *) tris;
	a.shade = (float4 *) shade;
	a.nodes = (float *) nodes;
	a.leaves = leaves;
	hipLaunchKernelGGL(refit_leaves_kernel, dim3((leaves + REFIT_LEAF_LANES - 1u) / REFIT_LEAF_LANES), dim3(REFIT_LEAF_LANES), 0,
	                   (hipStream_t) stream, a);
}

// ... and one pass of the inner boxes: the schedule's groups first_group ... first_group + groups_in_pass - 1, a workgroup each.
void launch_refit_inner(const void *entries, const void *children, const void *groups, void *nodes, uint32_t first_group, uint32_t groups_in_pass,
                        void *stream) {
	if (groups_in_pass == 0)
		return;
	RefitInnerArgs a{};
	a.entries = (const uint4 *) entries;
	a.children = (const uint32_t *) children;
	a.groups = (const uint4 *) groups;
	a.nodes = (float *) nodes;
	a.first_group = first_group;
	hipLaunchKernelGGL(refit_inner_kernel, dim3(groups_in_pass), dim3(REFIT_INNER_LANES), 0, (hipStream_t) stream, a);
}

// Device-side scene builds (kernels/build.hip.h, include/rt_hip_build.h): the keys of `b.num_faces` faces and their ids, the
// pairs the sort takes (build_sort.hip) ...
namespace {
BuildArgs build_args(const BuildBuffers &b) {
	BuildArgs a{};
	a.faces = (const uint32_t *) b.faces;
	a.vertices = (const float4 *) b.vertices;
	a.num_faces = b.num_faces;
	a.num_vertices = b.num_vertices;
	a.centres = (float4 *) b.centres;
	a.partials = (float4 *) b.partials;
	a.root = (float4 *) b.root;
	a.flag = (uint32_t *) b.flag;
	a.keys = (uint32_t *) b.keys;
	a.ids = (uint32_t *) b.ids;
	a.sorted_keys = (const uint32_t *) b.sorted_keys;
	a.sorted_ids = (const uint32_t *) b.sorted_ids;
	a.leaf_faces = (uint32_t *) b.leaf_faces;
	a.ranges = (uint2 *) b.ranges;
	a.inner_links = (uint32_t *) b.inner_links;
	a.leaf_links = (uint32_t *) b.leaf_links;
	a.nodes = (uint4 *) b.nodes;
	a.skips = (uint32_t *) b.skips;
	a.leaf_node = (uint32_t *) b.leaf_node;
	return a;
}
}  // namespace

uint32_t build_partials(uint32_t faces) { return (faces + BUILD_LANES - 1u) / BUILD_LANES; }

void launch_build_keys(const BuildBuffers &b, void *stream) {
	if (b.num_faces == 0 || b.num_vertices == 0)
		return;
	const BuildArgs a = build_args(b);
	const uint32_t groups = build_partials(b.num_faces);
	hipLaunchKernelGGL(build_boxes_kernel, dim3(groups), dim3(BUILD_LANES), 0, (hipStream_t) stream, a);
	hipLaunchKernelGGL(build_root_kernel, dim3(1), dim3(BUILD_LANES), 0, (hipStream_t) stream, a, groups);
	hipLaunchKernelGGL(build_keys_kernel, dim3(groups), dim3(BUILD_LANES), 0, (hipStream_t) stream, a);
}

// ... and, of the sorted pairs, the faces in leaf order, the tree's shape and its pre-order layout: `skip` and `leaf` words of
// every node record, the leaf -> node map, the skips alone.
void launch_build_tree(const BuildBuffers &b, void *stream) {
	if (b.num_faces == 0 || b.num_vertices == 0)
		return;
	const BuildArgs a = build_args(b);
	hipLaunchKernelGGL(build_tree_kernel, dim3(build_partials(b.num_faces)), dim3(BUILD_LANES), 0, (hipStream_t) stream, a);
	const uint32_t nodes = 2u * b.num_faces - 1u;
	hipLaunchKernelGGL(build_layout_kernel, dim3((nodes + BUILD_LANES - 1u) / BUILD_LANES), dim3(BUILD_LANES), 0, (hipStream_t) stream, a);
}

// Device-side instance sets (kernels/instance_build.hip.h, include/rt_hip_instance_build.h): inverses, leaf boxes, bounds and
// the keys of `b.n` instances with their indices, the pairs the sort takes (build_sort.hip) -- one instance: its leaf record,
// the whole tree ...
namespace {
InstanceBuildArgs instance_build_args(const InstancePlanBuffers &b) {
	InstanceBuildArgs a{};
	const uint32_t groups = build_partials(b.n);
	const bool fused = groups <= INSTANCE_FUSED_PARTIALS;
	a.world = (const float4 *) b.world;
	a.inverse = (float4 *) b.inverse;
	a.n = b.n;
	a.scene_root = (const float4 *) b.scene_root;
	a.flag = (uint32_t *) b.flag;
	a.reach_partials = (double *) b.reach_partials;
	a.reach = (const double *) (fused ? b.reach_partials : b.reach);
	a.reach_count = fused ? groups : 1u;
	a.leaves = (float4 *) b.leaves;
	a.bounds = (float4 *) b.bounds;
	a.box_partials = (float4 *) b.box_partials;
	a.box = (const float4 *) (fused ? b.box_partials : b.box);
	a.box_count = fused ? groups : 1u;
	a.keys = (uint32_t *) b.keys;
	a.ids = (uint32_t *) b.ids;
	a.sorted_keys = (const uint32_t *) b.sorted_keys;
	a.sorted_ids = (const uint32_t *) b.sorted_ids;
	a.ranges = (uint2 *) b.ranges;
	a.inner_links = (uint32_t *) b.inner_links;
	a.leaf_links = (uint32_t *) b.leaf_links;
	a.counters = (uint32_t *) b.counters;
	a.inner_at = (uint32_t *) b.inner_at;
	a.leaf_at = (uint32_t *) b.leaf_at;
	a.nodes = (uint4 *) b.nodes;
	return a;
}
}  // namespace

void launch_instance_keys(const InstancePlanBuffers &b, void *stream) {
	if (b.n == 0)
		return;
	const InstanceBuildArgs a = instance_build_args(b);
	const uint32_t groups = build_partials(b.n);
	const bool fused = groups <= INSTANCE_FUSED_PARTIALS;
	hipLaunchKernelGGL(instance_inverse_kernel, dim3(groups), dim3(BUILD_LANES), 0, (hipStream_t) stream, a);
	if (!fused)
		hipLaunchKernelGGL(instance_reach_kernel, dim3(1), dim3(BUILD_LANES), 0, (hipStream_t) stream, (const double *) b.reach_partials, groups,
		                   (double *) b.reach);
	hipLaunchKernelGGL(instance_leaves_kernel, dim3(groups), dim3(BUILD_LANES), 0, (hipStream_t) stream, a);
	if (b.n == 1u)
		return;
	if (!fused)
		hipLaunchKernelGGL(instance_root_kernel, dim3(1), dim3(BUILD_LANES), 0, (hipStream_t) stream, (const float4 *) b.box_partials, groups,
		                   (float4 *) b.box);
	hipLaunchKernelGGL(instance_keys_kernel, dim3(groups), dim3(BUILD_LANES), 0, (hipStream_t) stream, a);
}

// ... and, of the sorted pairs of two instances or more, the tree's shape, its pre-order layout with the leaf records, and the
// inner boxes.
void launch_instance_tree(const InstancePlanBuffers &b, void *stream) {
	if (b.n < 2u)
		return;
	const InstanceBuildArgs a = instance_build_args(b);
	const uint32_t groups = build_partials(b.n), nodes = 2u * b.n - 1u;
	hipLaunchKernelGGL(instance_tree_kernel, dim3(groups), dim3(BUILD_LANES), 0, (hipStream_t) stream, a);
	hipLaunchKernelGGL(instance_layout_kernel, dim3((nodes + BUILD_LANES - 1u) / BUILD_LANES), dim3(BUILD_LANES), 0, (hipStream_t) stream, a);
	hipLaunchKernelGGL(instance_boxes_kernel, dim3(groups), dim3(BUILD_LANES), 0, (hipStream_t) stream, a);
}

// Test aid (kernels/node_test_forms.hip.h, include/rt_hip_debug.h): the any-hit node test in both forms, `rays` (a multiple of
// 64) walk rays against `boxes` centre / half-extent records, nine words per pair into `out`.
void launch_node_test_forms(const void *records, uint32_t boxes, const void *rays6, uint32_t rays, void *out, void *stream) {
	if (boxes == 0 || rays == 0)
		return;
	hipLaunchKernelGGL(node_test_forms_kernel, dim3(rays / 64u), dim3(64), 0, (hipStream_t) stream, (const float4 *) records, boxes,
	                   (const float *) rays6, (uint32_t *) out);
}

}  // namespace ocrt
