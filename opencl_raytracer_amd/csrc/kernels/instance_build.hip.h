// kernels/instance_build.hip.h -- device-side instance sets (include/rt_hip_instance_build.h): from transforms in device
// memory to the inverses, the closest-point bounds and the top-level tree, the host never seeing any of them.  The arithmetic
// of one instance is instance_plan.h's (the functions instances.cc runs on the host), keys, shape and layout are lbvh.h's
// (the functions of a device-side scene build): rt_instance_plan_lbvh restates the whole on the host by the same calls.
//
//   instance_inverse_kernel  a lane per instance: the transform checked by instance_inverse's rules (a refused one raises
//                            the flag and gets a zero inverse), the inverse, the instance's reach; the workgroup's largest
//                            reach as a partial.
//   instance_reach_kernel    one workgroup: the largest of the partials (sets of more than INSTANCE_FUSED_PARTIALS
//                            workgroups; below that every workgroup of the next kernel reduces them for itself).
//   instance_leaves_kernel   a lane per instance: the set's reach, the leaf box, the bounds; the workgroup's share of the
//                            tree's root box as a partial.  One instance: its leaf record, and nothing else is launched.
//   instance_root_kernel     one workgroup: the root box of the partials (large sets, as above).
//   instance_keys_kernel     a lane per instance: the root box, the key of the leaf box's centre, the instance's index.
//   (build_sort.hip)         the pairs by key, stable.
//   instance_tree_kernel     a lane per rank of the sorted order: inner node i's leaves and children by its own search, a
//                            link to the parent in every child, the node's arrival counter cleared.
//   instance_layout_kernel   a lane per node: its place in pre-order from the links of the launch before; a leaf's whole
//                            record (box, skip 1, the INSTANCE's index), an inner node's skip and leaf words.
//   instance_boxes_kernel    a lane per leaf climbs towards the root.  At every parent it adds one to the node's counter: the
//                            first to arrive leaves -- its subtree's box lies in its record --, the second reads its
//                            sibling's record, writes the parent's box (first child's value where two compare equal) and
//                            goes on.  No lane waits for another.  What one lane hands to another in this launch goes
//                            through agent-scope atomic stores and loads with a release in front of the counter's add and
//                            an acquire behind it; everything else a lane reads was written by an earlier launch.
#pragma once

namespace ocrt {

constexpr uint32_t INSTANCE_FUSED_PARTIALS = BUILD_LANES;  // up to this many workgroups the reductions ride in the next kernel

struct InstanceBuildArgs {
	const float4 *world;        // [3 n] the library's copy of the transforms
	float4 *inverse;            // [3 n]
	uint32_t n;
	const float4 *scene_root;   // node 0 of the scene as it lies on the device (lo, skip | hi, leaf), or null: no scene yet
	uint32_t *flag;             // raised by a refused transform
	double *reach_partials;     // [workgroups]
	const double *reach;        // what instance_leaves_kernel reduces: reach_count values
	uint32_t reach_count;
	float4 *leaves;             // [2 n] lo, hi by instance
	float4 *bounds;             // [n]
	float4 *box_partials;       // [workgroups][2]
	const float4 *box;          // what instance_keys_kernel reduces: box_count pairs
	uint32_t box_count;
	uint32_t *keys, *ids;
	const uint32_t *sorted_keys, *sorted_ids;
	uint2 *ranges;              // [n - 1]
	uint32_t *inner_links, *leaf_links;  // [n - 1], [n]
	uint32_t *counters;         // [n - 1]
	uint32_t *inner_at, *leaf_at;  // [n - 1], [n]: the record of every inner node and of every rank
	uint4 *nodes;               // NodeRec[2 n - 1] as two uint4
};

// The scene's root box; one that is not finite where there is no scene yet.
__device__ __forceinline__ void instance_scene_root(const InstanceBuildArgs &a, float lo[3], float hi[3]) {
	if (a.scene_root) {
		const float4 l = a.scene_root[0], h = a.scene_root[1];
		lo[0] = l.x, lo[1] = l.y, lo[2] = l.z;
		hi[0] = h.x, hi[1] = h.y, hi[2] = h.z;
	} else {
		for (int k = 0; k < 3; ++k)
			lo[k] = -__builtin_inff(), hi[k] = __builtin_inff();
	}
}

__device__ __forceinline__ void instance_rows(const float4 *rows, uint32_t k, float M[12]) {
#pragma unroll
	for (uint32_t r = 0; r < 3u; ++r) {
		const float4 v = rows[3ull * k + r];
		M[4u * r] = v.x, M[4u * r + 1u] = v.y, M[4u * r + 2u] = v.z, M[4u * r + 3u] = v.w;
	}
}

// The workgroup's largest v, in every lane (the maximum of doubles is exact: the order is free).
__device__ __forceinline__ double instance_group_max(double v) {
	__shared__ double part[BUILD_LANES];
	part[threadIdx.x] = v;
	__syncthreads();
	for (uint32_t step = BUILD_LANES / 2u; step >= 1u; step >>= 1) {
		if (threadIdx.x < step)
			part[threadIdx.x] = instance_max(part[threadIdx.x], part[threadIdx.x + step]);
		__syncthreads();
	}
	const double all = part[0];
	__syncthreads();
	return all;
}

__device__ __forceinline__ double instance_reach_of(const double *values, uint32_t count) {
	double v = 0.0;
	for (uint32_t p = threadIdx.x; p < count; p += BUILD_LANES)
		v = instance_max(v, values[p]);
	return instance_group_max(v);
}

// The per-axis minimum of lo and maximum of hi over `count` pairs, in every lane.
__device__ __forceinline__ void instance_box_of(const float4 *pairs, uint32_t count, float lo[3], float hi[3]) {
	__shared__ float all[6];
	const float inf = __builtin_inff();
	for (int k = 0; k < 3; ++k)
		lo[k] = inf, hi[k] = -inf;
	for (uint32_t p = threadIdx.x; p < count; p += BUILD_LANES) {
		const float4 l = pairs[2ull * p], h = pairs[2ull * p + 1u];
		lo[0] = l.x < lo[0] ? l.x : lo[0]; lo[1] = l.y < lo[1] ? l.y : lo[1]; lo[2] = l.z < lo[2] ? l.z : lo[2];
		hi[0] = hi[0] < h.x ? h.x : hi[0]; hi[1] = hi[1] < h.y ? h.y : hi[1]; hi[2] = hi[2] < h.z ? h.z : hi[2];
	}
	build_group_box(lo, hi);
	if (threadIdx.x == 0u) {
		for (int k = 0; k < 3; ++k)
			all[k] = lo[k], all[3 + k] = hi[k];
	}
	__syncthreads();
	for (int k = 0; k < 3; ++k)
		lo[k] = all[k], hi[k] = all[3 + k];
	__syncthreads();
}

__global__ __launch_bounds__(BUILD_LANES) void instance_inverse_kernel(const InstanceBuildArgs a) {
	const uint32_t k = blockIdx.x * BUILD_LANES + threadIdx.x;
	double reach = 0.0;
	if (k < a.n) {
		float W[12], O[12];
		instance_rows(a.world, k, W);
		for (int j = 0; j < 12; ++j)
			O[j] = 0.0f;
		if (!instance_inverse(W, O))
			atomicOr(a.flag, 1u);
#pragma unroll
		for (uint32_t r = 0; r < 3u; ++r)
			a.inverse[3ull * k + r] = make_float4(O[4u * r], O[4u * r + 1u], O[4u * r + 2u], O[4u * r + 3u]);
		float root_lo[3], root_hi[3];
		instance_scene_root(a, root_lo, root_hi);
		reach = instance_max(0.0, instance_reach(root_lo, root_hi, W));  // (a reach that is no number counts as the host counts it: not at all)
	}
	reach = instance_group_max(reach);
	if (threadIdx.x == 0u)
		a.reach_partials[blockIdx.x] = reach;
}

// (one workgroup; the result lies in out[0])
__global__ __launch_bounds__(BUILD_LANES) void instance_reach_kernel(const double *partials, uint32_t count, double *out) {
	const double reach = instance_reach_of(partials, count);
	if (threadIdx.x == 0u)
		out[0] = reach;
}

__global__ __launch_bounds__(BUILD_LANES) void instance_leaves_kernel(const InstanceBuildArgs a) {
	const uint32_t k = blockIdx.x * BUILD_LANES + threadIdx.x;
	const double reach = instance_reach_of(a.reach, a.reach_count);
	const float inf = __builtin_inff();
	float lo[3] = { inf, inf, inf }, hi[3] = { -inf, -inf, -inf };
	if (k < a.n) {
		float W[12], O[12], root_lo[3], root_hi[3], bound[4];
		instance_rows(a.world, k, W);
		instance_rows(a.inverse, k, O);
		instance_scene_root(a, root_lo, root_hi);
		instance_box(root_lo, root_hi, W, O, 4.0 * reach, lo, hi);
		instance_bound(root_lo, root_hi, W, O, bound);
		a.leaves[2ull * k] = make_float4(lo[0], lo[1], lo[2], 0.0f);
		a.leaves[2ull * k + 1u] = make_float4(hi[0], hi[1], hi[2], 0.0f);
		a.bounds[k] = make_float4(bound[0], bound[1], bound[2], bound[3]);
		if (a.n == 1u) {  // (the whole tree)
			a.nodes[0] = make_uint4(__float_as_uint(lo[0]), __float_as_uint(lo[1]), __float_as_uint(lo[2]), 1u);
			a.nodes[1] = make_uint4(__float_as_uint(hi[0]), __float_as_uint(hi[1]), __float_as_uint(hi[2]), 0u);
		}
	}
	build_group_box(lo, hi);
	if (threadIdx.x == 0u) {
		a.box_partials[2ull * blockIdx.x] = make_float4(lo[0], lo[1], lo[2], 0.0f);
		a.box_partials[2ull * blockIdx.x + 1u] = make_float4(hi[0], hi[1], hi[2], 0.0f);
	}
}

// (one workgroup; the result lies in out[0], out[1])
__global__ __launch_bounds__(BUILD_LANES) void instance_root_kernel(const float4 *partials, uint32_t count, float4 *out) {
	float lo[3], hi[3];
	instance_box_of(partials, count, lo, hi);
	if (threadIdx.x == 0u) {
		out[0] = make_float4(lo[0], lo[1], lo[2], 0.0f);
		out[1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
	}
}

__global__ __launch_bounds__(BUILD_LANES) void instance_keys_kernel(const InstanceBuildArgs a) {
	const uint32_t k = blockIdx.x * BUILD_LANES + threadIdx.x;
	float lo[3], hi[3];
	instance_box_of(a.box, a.box_count, lo, hi);
	if (k >= a.n)
		return;
	const float4 l = a.leaves[2ull * k], h = a.leaves[2ull * k + 1u];
	a.keys[k] = lbvh_key(lbvh_cell(lbvh_centre(l.x, h.x), lo[0], hi[0]), lbvh_cell(lbvh_centre(l.y, h.y), lo[1], hi[1]),
	                     lbvh_cell(lbvh_centre(l.z, h.z), lo[2], hi[2]));
	a.ids[k] = k;
}

// (n >= 2)
__global__ __launch_bounds__(BUILD_LANES) void instance_tree_kernel(const InstanceBuildArgs a) {
	const uint32_t i = blockIdx.x * BUILD_LANES + threadIdx.x;
	if (i >= a.n)
		return;
	if (i == 0u)
		a.inner_links[0] = LBVH_NONE;
	if (i + 1u >= a.n)
		return;
	a.counters[i] = 0u;
	uint32_t first, last, split;
	lbvh_node(a.sorted_keys, a.n, i, &first, &last, &split);
	// (first <= split < last <= n - 1 for rising keys; held to it whatever the keys are)
	last = last < a.n ? last : a.n - 1u;
	last = last ? last : 1u;
	split = split < last ? split : last - 1u;
	first = first <= split ? first : split;
	a.ranges[i] = make_uint2(first, last);
	(first == split ? a.leaf_links : a.inner_links)[split] = i | LBVH_FIRST;
	(last == split + 1u ? a.leaf_links : a.inner_links)[split + 1u] = i;
}

// (n >= 2)
__global__ __launch_bounds__(BUILD_LANES) void instance_layout_kernel(const InstanceBuildArgs a) {
	const uint32_t t = blockIdx.x * BUILD_LANES + threadIdx.x;
	const uint32_t inner = a.n - 1u, count = 2u * a.n - 1u;
	if (t >= count)
		return;
	const bool is_leaf = t >= inner;
	const uint32_t rank = t - inner;
	const uint2 range = is_leaf ? make_uint2(rank, rank) : a.ranges[t];
	const uint32_t turns = lbvh_first_child_turns(a.inner_links, inner, is_leaf ? a.leaf_links[rank] : a.inner_links[t]);
	uint32_t at = 2u * range.x + turns;
	at = at < count ? at : count - 1u;  // (no tree of rising keys puts a node beyond the array)
	if (is_leaf) {
		uint32_t instance = a.sorted_ids[rank];
		instance = instance < a.n ? instance : 0u;  // (the sort's own output: a permutation)
		const float4 l = a.leaves[2ull * instance], h = a.leaves[2ull * instance + 1u];
		a.nodes[2ull * at] = make_uint4(__float_as_uint(l.x), __float_as_uint(l.y), __float_as_uint(l.z), 1u);
		a.nodes[2ull * at + 1u] = make_uint4(__float_as_uint(h.x), __float_as_uint(h.y), __float_as_uint(h.z), instance);
		a.leaf_at[rank] = at;
	} else {
		a.nodes[2ull * at] = make_uint4(0u, 0u, 0u, 2u * (range.y - range.x + 1u) - 1u);
		a.nodes[2ull * at + 1u] = make_uint4(0u, 0u, 0u, LBVH_NONE);
		a.inner_at[t] = at;
	}
}

// One box word handed between lanes of this launch: written through and read past the compute unit's cache.
__device__ __forceinline__ void instance_publish(uint32_t *word, float v) {
	__hip_atomic_store(word, __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float instance_observe(uint32_t *word) {
	return __uint_as_float(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// (n >= 2)
__global__ __launch_bounds__(BUILD_LANES) void instance_boxes_kernel(const InstanceBuildArgs a) {
	const uint32_t rank = blockIdx.x * BUILD_LANES + threadIdx.x;
	const uint32_t inner = a.n - 1u, count = 2u * a.n - 1u;
	if (rank >= a.n)
		return;
	uint32_t *const words = (uint32_t *) a.nodes;  // eight per record: lo[3], skip, hi[3], leaf
	uint32_t at = a.leaf_at[rank], skip = 1u, link = a.leaf_links[rank];
	if (at >= count)
		return;
	float lo[3], hi[3];
	{
		const uint4 l = a.nodes[2ull * at], h = a.nodes[2ull * at + 1u];  // (the launch before wrote it)
		lo[0] = __uint_as_float(l.x), lo[1] = __uint_as_float(l.y), lo[2] = __uint_as_float(l.z);
		hi[0] = __uint_as_float(h.x), hi[1] = __uint_as_float(h.y), hi[2] = __uint_as_float(h.z);
	}
	for (uint32_t step = 0; step < 64u && link != LBVH_NONE; ++step) {
		const uint32_t parent = link & ~LBVH_FIRST;
		const bool am_first = (link & LBVH_FIRST) != 0u;
		if (parent >= inner)
			return;  // (damaged links lead nowhere)
		const uint32_t parent_at = a.inner_at[parent];
		if (parent_at >= count)
			return;
		// everything this lane published lies in memory before the counter moves; what the other lane published is read
		// only behind the counter's answer
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
		const uint32_t arrived = __hip_atomic_fetch_add(a.counters + parent, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
		if (arrived != 1u)
			return;  // the first to arrive (or, on damaged links, one too many)
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
		const uint32_t sibling = am_first ? at + skip : parent_at + 1u;
		if (sibling >= count)
			return;
		float other_lo[3], other_hi[3];
#pragma unroll
		for (uint32_t k = 0; k < 3u; ++k) {
			other_lo[k] = instance_observe(words + 8ull * sibling + k);
			other_hi[k] = instance_observe(words + 8ull * sibling + 4u + k);
		}
#pragma unroll
		for (uint32_t k = 0; k < 3u; ++k) {  // (first child a, second b: lo = b < a ? b : a, hi = a < b ? b : a)
			const float a_lo = am_first ? lo[k] : other_lo[k], b_lo = am_first ? other_lo[k] : lo[k];
			const float a_hi = am_first ? hi[k] : other_hi[k], b_hi = am_first ? other_hi[k] : hi[k];
			lo[k] = b_lo < a_lo ? b_lo : a_lo;
			hi[k] = a_hi < b_hi ? b_hi : a_hi;
			instance_publish(words + 8ull * parent_at + k, lo[k]);
			instance_publish(words + 8ull * parent_at + 4u + k, hi[k]);
		}
		skip = 2u * (a.ranges[parent].y - a.ranges[parent].x + 1u) - 1u;
		at = parent_at;
		link = a.inner_links[parent];
	}
}

}  // namespace ocrt
