// kernels/build.hip.h -- device-side scene builds (include/rt_hip_build.h): the topology of the tree lbvh.h defines, from
// faces and vertices in device memory.  The arithmetic of a key, the search for a node's leaves and the count that places a
// node are lbvh.h's functions, the ones rt_scene_build_lbvh runs on the host.  The records and the boxes are then made by
// kernels/refit.hip.h as for a vertex update.
//
//   build_boxes_kernel    a lane per face: every index checked BEFORE anything is read through it (a bad face is built from
//                         vertex 0 and raises the flag), the centre of the face's box by the refit rule, the workgroup's
//                         share of the root box as a partial.
//   build_root_kernel     one workgroup: the root box of the partials.
//   build_keys_kernel     a lane per face: its key and its id, the pairs the sort takes (build_sort.hip).
//   build_tree_kernel     a lane per leaf of the sorted order: the leaf's face gathered, checked again, into leaf order, and
//                         inner node i's leaves and children -- its own search, no lane waits for another --; every child
//                         is left a link to its parent.
//   build_layout_kernel   a lane per node: the links, written by the launch BEFORE, walked up to the root (62 steps at most)
//                         give the node's place in pre-order; `skip` and `leaf` words, the leaf -> node map, the skips alone
//                         for the host.
// No workgroup waits for another; whatever one launch hands to lanes of other workgroups, a later launch reads.
#pragma once

namespace ocrt {

constexpr uint32_t BUILD_LANES = 256u;

struct BuildArgs {
	const uint32_t *faces;     // three vertex ids per face, as given
	const float4 *vertices;
	uint32_t num_faces, num_vertices;
	float4 *centres;           // [faces] the centre of every face's box
	float4 *partials;          // [workgroups of build_boxes_kernel][2] lo, hi
	float4 *root;              // [2] lo, hi
	uint32_t *flag;            // raised by a face with an index out of range
	uint32_t *keys, *ids;      // [faces] the sort's input
	const uint32_t *sorted_keys, *sorted_ids;  // ... and output: the face of every leaf
	uint32_t *leaf_faces;      // [3 * faces] the faces in leaf order
	uint2 *ranges;             // [faces - 1] the leaves of every inner node
	uint32_t *inner_links, *leaf_links;  // [faces - 1], [faces]: lbvh.h, lbvh_first_child_turns
	uint4 *nodes;              // NodeRec[2 * faces - 1] as two uint4
	uint32_t *skips;           // [2 * faces - 1]
	uint32_t *leaf_node;       // [faces]
};

// (comparison and select, as the refit rule has it: not v_min_f32 / v_max_f32)
__device__ __forceinline__ float build_wave_min(float v) {
#pragma unroll
	for (int m = 32; m >= 1; m >>= 1) {
		const float other = __shfl_xor(v, m, 64);
		v = other < v ? other : v;
	}
	return v;
}
__device__ __forceinline__ float build_wave_max(float v) {
#pragma unroll
	for (int m = 32; m >= 1; m >>= 1) {
		const float other = __shfl_xor(v, m, 64);
		v = v < other ? other : v;
	}
	return v;
}

// The workgroup's minimum of lo[] and maximum of hi[] per axis, in lane 0 of wave 0.
__device__ __forceinline__ void build_group_box(float lo[3], float hi[3]) {
	__shared__ float part[BUILD_LANES / 64u][6];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
	for (uint32_t k = 0; k < 3u; ++k) {
		lo[k] = build_wave_min(lo[k]);
		hi[k] = build_wave_max(hi[k]);
	}
	if (lane == 0u) {
#pragma unroll
		for (uint32_t k = 0; k < 3u; ++k) {
			part[wave][k] = lo[k];
			part[wave][3u + k] = hi[k];
		}
	}
	__syncthreads();
	if (threadIdx.x == 0u) {
		for (uint32_t w = 1; w < BUILD_LANES / 64u; ++w) {
#pragma unroll
			for (uint32_t k = 0; k < 3u; ++k) {
				lo[k] = part[w][k] < lo[k] ? part[w][k] : lo[k];
				hi[k] = hi[k] < part[w][3u + k] ? part[w][3u + k] : hi[k];
			}
		}
	}
}

__global__ __launch_bounds__(BUILD_LANES) void build_boxes_kernel(const BuildArgs a) {
	const uint32_t face = blockIdx.x * BUILD_LANES + threadIdx.x;
	const float inf = __builtin_inff();
	float lo[3] = { inf, inf, inf }, hi[3] = { -inf, -inf, -inf };
	if (face < a.num_faces) {
		uint32_t i0 = a.faces[3ull * face], i1 = a.faces[3ull * face + 1u], i2 = a.faces[3ull * face + 2u];
		if (i0 >= a.num_vertices || i1 >= a.num_vertices || i2 >= a.num_vertices) {
			i0 = i1 = i2 = 0u;
			atomicOr(a.flag, 1u);
		}
		const float4 va = a.vertices[i0], vb = a.vertices[i1], vc = a.vertices[i2];
		lo[0] = refit_min3(va.x, vb.x, vc.x); lo[1] = refit_min3(va.y, vb.y, vc.y); lo[2] = refit_min3(va.z, vb.z, vc.z);
		hi[0] = refit_max3(va.x, vb.x, vc.x); hi[1] = refit_max3(va.y, vb.y, vc.y); hi[2] = refit_max3(va.z, vb.z, vc.z);
		a.centres[face] = make_float4(lbvh_centre(lo[0], hi[0]), lbvh_centre(lo[1], hi[1]), lbvh_centre(lo[2], hi[2]), 0.0f);
	}
	build_group_box(lo, hi);
	if (threadIdx.x == 0u) {
		a.partials[2ull * blockIdx.x] = make_float4(lo[0], lo[1], lo[2], 0.0f);
		a.partials[2ull * blockIdx.x + 1u] = make_float4(hi[0], hi[1], hi[2], 0.0f);
	}
}

// (one workgroup; `partials`: the grid of build_boxes_kernel)
__global__ __launch_bounds__(BUILD_LANES) void build_root_kernel(const BuildArgs a, const uint32_t partials) {
	const float inf = __builtin_inff();
	float lo[3] = { inf, inf, inf }, hi[3] = { -inf, -inf, -inf };
	for (uint32_t p = threadIdx.x; p < partials; p += BUILD_LANES) {
		const float4 l = a.partials[2ull * p], h = a.partials[2ull * p + 1u];
		lo[0] = l.x < lo[0] ? l.x : lo[0]; lo[1] = l.y < lo[1] ? l.y : lo[1]; lo[2] = l.z < lo[2] ? l.z : lo[2];
		hi[0] = hi[0] < h.x ? h.x : hi[0]; hi[1] = hi[1] < h.y ? h.y : hi[1]; hi[2] = hi[2] < h.z ? h.z : hi[2];
	}
	build_group_box(lo, hi);
	if (threadIdx.x == 0u) {
		a.root[0] = make_float4(lo[0], lo[1], lo[2], 0.0f);
		a.root[1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
	}
}

__global__ __launch_bounds__(BUILD_LANES) void build_keys_kernel(const BuildArgs a) {
	const uint32_t face = blockIdx.x * BUILD_LANES + threadIdx.x;
	if (face >= a.num_faces)
		return;
	const float4 lo = a.root[0], hi = a.root[1], c = a.centres[face];
	a.keys[face] = lbvh_key(lbvh_cell(c.x, lo.x, hi.x), lbvh_cell(c.y, lo.y, hi.y), lbvh_cell(c.z, lo.z, hi.z));
	a.ids[face] = face;
}

__global__ __launch_bounds__(BUILD_LANES) void build_tree_kernel(const BuildArgs a) {
	const uint32_t i = blockIdx.x * BUILD_LANES + threadIdx.x;
	if (i >= a.num_faces)
		return;
	{
		uint32_t face = a.sorted_ids[i];
		face = face < a.num_faces ? face : 0u;  // (the sort's own output: a permutation)
		uint32_t i0 = a.faces[3ull * face], i1 = a.faces[3ull * face + 1u], i2 = a.faces[3ull * face + 2u];
		if (i0 >= a.num_vertices || i1 >= a.num_vertices || i2 >= a.num_vertices)
			i0 = i1 = i2 = 0u;  // (as build_boxes_kernel built it; the flag is up already)
		a.leaf_faces[3ull * i] = i0;
		a.leaf_faces[3ull * i + 1u] = i1;
		a.leaf_faces[3ull * i + 2u] = i2;
	}
	if (i == 0u)
		(a.num_faces == 1u ? a.leaf_links : a.inner_links)[0] = LBVH_NONE;
	if (i + 1u >= a.num_faces)
		return;
	uint32_t first, last, split;
	lbvh_node(a.sorted_keys, a.num_faces, i, &first, &last, &split);
	// (first <= split < last <= num_faces - 1 for rising keys; held to it whatever the keys are)
	last = last < a.num_faces ? last : a.num_faces - 1u;
	last = last ? last : 1u;
	split = split < last ? split : last - 1u;
	first = first <= split ? first : split;
	a.ranges[i] = make_uint2(first, last);
	(first == split ? a.leaf_links : a.inner_links)[split] = i | LBVH_FIRST;
	(last == split + 1u ? a.leaf_links : a.inner_links)[split + 1u] = i;
}

__global__ __launch_bounds__(BUILD_LANES) void build_layout_kernel(const BuildArgs a) {
	const uint32_t t = blockIdx.x * BUILD_LANES + threadIdx.x;
	const uint32_t inner = a.num_faces - 1u, count = 2u * a.num_faces - 1u;
	if (t >= count)
		return;
	const bool is_leaf = t >= inner;
	const uint32_t leaf = t - inner;
	const uint2 range = is_leaf ? make_uint2(leaf, leaf) : a.ranges[t];
	const uint32_t turns = lbvh_first_child_turns(a.inner_links, inner, is_leaf ? a.leaf_links[leaf] : a.inner_links[t]);
	const uint32_t at = 2u * range.x + turns;
	if (at >= count)
		return;  // (no tree of rising keys puts a node there)
	const uint32_t skip = 2u * (range.y - range.x + 1u) - 1u;
	// (the boxes come with the records: refit_leaves_kernel, refit_inner_kernel)
	a.nodes[2ull * at] = make_uint4(0u, 0u, 0u, skip);
	a.nodes[2ull * at + 1u] = make_uint4(0u, 0u, 0u, is_leaf ? leaf : LBVH_NONE);
	a.skips[at] = skip;
	if (is_leaf)
		a.leaf_node[leaf] = at;
}

}  // namespace ocrt
