// kernels/nearest.hip.h -- closest-point queries: the nearest point of the surface for points the caller supplies
// (include/rt_hip_nearest.h; the arithmetic is nearest_point.h's, the same file the tests' oracle compiles)
// (part of the one translation unit kernels.hip; see its head for the passes and the arithmetic contract)
//
// One point per lane, a packet of 64 per wave.  The answer is the minimum of (d2, leaf) over ALL leaves, so nothing the walk
// does can change a bit of it: the walk only decides which leaves it may leave out, and the margin of np_limit2 (proof in
// nearest_point.h) is what makes leaving them out safe.
//
// The walk has two parts.
//   1. nearest_descend: each lane goes down the tree on its own, at every inner node into the child whose box is nearest,
//      and tests the one leaf it arrives at.  That is a few dozen gathered node records per lane (two per level: the
//      children of the node at i sit at i + 1 and behind the first child's subtree), divergent and unshared -- and it
//      is what makes the second part prune: the skip-pointer order is fixed, depth first, first child first, and under
//      a bound that starts at +inf a lane would enter every subtree ahead of the one that holds its answer.
//   2. the shared walk of exact_walk's shape: one wave-uniform node index, the record by ONE scalar load, the box distance
//      out of SGPRs, a subtree skipped when no live lane needs it (np_prune against the lane's own limit, which falls as the
//      lane finds nearer triangles).  No stack: a wave-uniform "nearer child first" order needs both children's records
//      before it can move -- a second, dependent scalar load per inner node, the latency the walks are bound by -- and an
//      order that suits the packet's mean suits its lanes only as far as they agree; the descent gives every lane ITS bound
//      for the price of gathers that hit the L2.  No LDS, few registers held across the loop: the launch keeps 8 waves per
//      SIMD, which is what hides the scalar load's latency.
// Boxes nest, and np_box_d2 is monotone in the box: a lane that does not need a node needs none below it, so the walk
// keeps no per-lane position (exact_walk's `mine`) -- the test itself says no again.  Lanes that need a leaf test it; the
// others sit out (divergence inside a leaf step only).
// Scenes whose boxes promise nothing (NearestArgs::walk without NEAREST_PRUNE: damaged uploads) are walked leaf by leaf.
#pragma once
#include "query.hip.h"

namespace ocrt {

// ---- coherence key: position only ------------------------------------------------------------------------------------
// 15 bits of Morton code, 32 cells per axis over the root box (the ray key's 8 cells and its direction bits, constant
// here, would leave 512 buckets); points outside are clamped to the border cells, points that are no numbers take the
// last bucket.  The counting sort around it is query.hip.h's (wave_groups, query_scan_kernel).
struct NearestKeyArgs {
	const float4 *points;
	uint32_t *count;  // [QUERY_BUCKETS]
	uint32_t *order;  // [n]
	uint32_t n;
	float lo[3], scale[3];  // QueryKeyArgs': 8 cells per axis inside the scene box (a quarter of a cell here)
};

namespace {

__device__ __forceinline__ uint32_t nearest_key(const float4 p, const NearestKeyArgs &a) {
	if (!np_point_ok(p.x, p.y, p.z))
		return QUERY_BUCKETS - 1u;
	const float cx = (p.x - a.lo[0]) * a.scale[0] * 4.0f, cy = (p.y - a.lo[1]) * a.scale[1] * 4.0f, cz = (p.z - a.lo[2]) * a.scale[2] * 4.0f;
	// (fmaxf drops the NaN of an overflow)
	const uint32_t qx = (uint32_t) fminf(fmaxf(cx, 0.0f), 31.0f), qy = (uint32_t) fminf(fmaxf(cy, 0.0f), 31.0f);
	const uint32_t qz = (uint32_t) fminf(fmaxf(cz, 0.0f), 31.0f);
	uint32_t morton = 0u;
	for (uint32_t b = 0; b < 5u; ++b)
		morton |= (((qx >> b) & 1u) << (3u * b)) | (((qy >> b) & 1u) << (3u * b + 1u)) | (((qz >> b) & 1u) << (3u * b + 2u));
	return morton;
}

}  // namespace

__global__ __launch_bounds__(256) void nearest_key_kernel(NearestKeyArgs a) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	const bool active = i < a.n;
	uint32_t key = 0u;
	if (active)
		key = nearest_key(a.points[i], a);
	uint32_t leader, rank, size;
	wave_groups(key, active, leader, rank, size);
	if (active && rank == 0u)
		atomicAdd(&a.count[key], size);
	(void) leader;
}

__global__ __launch_bounds__(256) void nearest_scatter_kernel(NearestKeyArgs a) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	const bool active = i < a.n;
	uint32_t key = 0u;
	if (active)
		key = nearest_key(a.points[i], a);
	uint32_t leader, rank, size;
	wave_groups(key, active, leader, rank, size);
	uint32_t first = 0u;
	if (active && rank == 0u)
		first = atomicAdd(&a.count[key], size);
	first = (uint32_t) __shfl((int) first, (int) leader);
	if (active)
		a.order[first + rank] = i;
}

// ---- the query -------------------------------------------------------------------------------------------------------
constexpr uint32_t NEAREST_START = 1u, NEAREST_PRUNE = 2u;  // NearestArgs::walk

struct NearestArgs {
	const float4 *nodes_ptr;  // SceneBuffers::nodes: exact boxes, skip layout (NodeRec)
	const float4 *tris_ptr;   // TriRec by leaf
	const float4 *shade;      // ShadeRec by leaf
	const float4 *points;     // float4[n]
	const uint32_t *order;    // [n] point of packet lane k, or null: point k
	uint32_t n, node_count, tri_count;
	float max_distance;
	uint32_t walk;  // NEAREST_START: the lanes descend for a starting bound; NEAREST_PRUNE: boxes may be passed by.  Both
	                // only where every box holds the triangles beneath it (DeviceScene::boxesEnclose).
	const uint32_t *coords_flag;  // null, or one word: non-zero = the boxes were made from coordinates that are no numbers
	                              // (nearest_coordinates_kernel): `walk` counts as 0
	RecordOutputs out;
	uint8_t *hit;
	unsigned long long *counts;  // COUNT: [2] box tests and triangle tests, summed over the points
};

// What the host checks of the vertices it is given in host memory, for those it is given on the device: behind an update or
// a device-side build, into the word the later queries read.
__global__ __launch_bounds__(256) void nearest_coordinates_kernel(const float4 *vertices, uint32_t n, uint32_t *flag) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n)
		return;
	const float4 v = vertices[i];
	if (!(fabsf(v.x) <= 1.0e37f) || !(fabsf(v.y) <= 1.0e37f) || !(fabsf(v.z) <= 1.0e37f))  // (a NaN too)
		*flag = 1u;
}

// A lane's record: the minimum of (d2, leaf) so far, and the point it belongs to.
// (`region`: np_point's, the feature the point lies on; only the signed tails read it -- kernels/signed.hip.h)
struct Nearest {
	float d2;
	uint32_t leaf;
	float s, t, px, py, pz;
	int region;
};

__device__ __forceinline__ np_tri nearest_tri(const float4 q0, const float4 q1, const float4 q2, const float4 q3) {
	np_tri t;
	t.tax = q0.x; t.tay = q0.y; t.taz = q0.z;
	t.ux = q0.w; t.uy = q1.x; t.uz = q1.y;
	t.vx = q1.z; t.vy = q1.w; t.vz = q2.x;
	t.uu = q3.x; t.uv = q3.y; t.vv = q3.z; t.D = q3.w;
	return t;
}

// Leaf `leaf` against the lane's record; returns whether it replaced it.
__device__ __forceinline__ bool nearest_take(Nearest &best, const np_tri &tri, uint32_t leaf, float qx, float qy, float qz) {
	const np_point r = np_nearest(tri, qx, qy, qz);
	if (!np_better(r.d2, leaf, best.d2, best.leaf))
		return false;
	best.d2 = r.d2;
	best.leaf = leaf;
	best.s = r.s; best.t = r.t;
	best.px = r.px; best.py = r.py; best.pz = r.pz;
	best.region = r.region;
	return true;
}

// Part 1: the lane's own way down, into the nearest child's box at every inner node, and the leaf it ends at.  Records by
// buffer loads (out of range reads 0, which ends the descent: a child of size 0 is no child); `at` only grows.
template <bool COUNT>
__device__ __forceinline__ void nearest_descend(const SceneViews &scene, uint32_t tri_count, float qx, float qy, float qz, bool active,
                                                Nearest &best, uint32_t &node_tests, uint32_t &tri_tests) {
	if (!active)
		return;
	uint32_t at = 0u;
	float4 lo = load_f4(scene.nodes, 0u), hi = load_f4(scene.nodes, 16u);
	while (__float_as_uint(hi.w) == NONE) {
		const uint32_t end = at + __float_as_uint(lo.w);
		uint32_t c = at + 1u, pick = NONE;
		float pick_d2 = 0.0f;
		while (c < end) {
			const float4 clo = load_f4(scene.nodes, c * 32u), chi = load_f4(scene.nodes, c * 32u + 16u);
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
			return;  // (an inner node without children: no starting bound)
		at = pick;
	}
	const uint32_t leaf = __float_as_uint(hi.w);
	if (leaf >= tri_count)
		return;
	const uint32_t rec = leaf * LEAF_BYTES + LEAF_TRI_OFFSET;
	const float4 q0 = load_f4(scene.tris, rec), q1 = load_f4(scene.tris, rec + 16u), q2 = load_f4(scene.tris, rec + 32u),
	             q3 = load_f4(scene.tris, rec + 48u);
	if (COUNT)
		++tri_tests;
	(void) nearest_take(best, nearest_tri(q0, q1, q2, q3), leaf, qx, qy, qz);
}

constexpr uint32_t NEAREST_WAVES = 4u;

// Both parts for one packet: the record of the lane's point q (`alive`: the lane has one that looks at anything).  Every
// kernel of the family -- nearest_kernel, and the signed forms of kernels/signed.hip.h -- is this walk and a tail.
template <bool COUNT>
__device__ __forceinline__ Nearest nearest_walk(const NearestArgs &a, const float4 q, bool alive, uint32_t &node_tests, uint32_t &tri_tests) {
	Nearest best;
	best.d2 = __builtin_inff();
	best.leaf = NONE;
	best.s = best.t = 0.0f;
	best.px = best.py = best.pz = 0.0f;
	best.region = NP_FACE;
	// the limit a box's distance is held against: +inf where nothing may be passed by
	const uint32_t walk = (a.coords_flag && *a.coords_flag != 0u) ? 0u : a.walk;  // (wave-uniform)
	const bool prune = (walk & NEAREST_PRUNE) != 0u;
	float magnitude = 0.0f, limit2 = __builtin_inff(), radius2 = __builtin_inff();
	if (prune && a.node_count != 0u) {
		const u32x8 root = scalar_load_node(a.nodes_ptr, 0u);
		magnitude = np_magnitude(__uint_as_float(root[0]), __uint_as_float(root[1]), __uint_as_float(root[2]), __uint_as_float(root[4]),
		                         __uint_as_float(root[5]), __uint_as_float(root[6]), q.x, q.y, q.z);
		radius2 = np_limit2_of_distance(a.max_distance, magnitude);
		limit2 = radius2;
	}
	if ((walk & NEAREST_START) != 0u && prune && a.node_count != 0u) {
		const SceneViews scene = make_views(a.nodes_ptr, a.tris_ptr, a.node_count, a.tri_count);
		nearest_descend<COUNT>(scene, a.tri_count, q.x, q.y, q.z, alive, best, node_tests, tri_tests);
		limit2 = fminf(radius2, np_limit2(best.d2, magnitude));
	}
	uint32_t at = 0u;
	while (at < a.node_count) {
		const u32x8 node = scalar_load_node(a.nodes_ptr, at);
		const uint32_t size = node[3], leaf = node[7];
		const float box_d2 = np_box_d2(__uint_as_float(node[0]), __uint_as_float(node[1]), __uint_as_float(node[2]), __uint_as_float(node[4]),
		                               __uint_as_float(node[5]), __uint_as_float(node[6]), q.x, q.y, q.z);
		const bool need = alive && !np_prune(box_d2, limit2);
		const bool any = wave_ballot(need) != 0ull;
		if (COUNT && alive)
			++node_tests;
		if (any && leaf != NONE) {
			const float4 *tri = a.tris_ptr + LEAF_F4 * leaf + LEAF_TRI_F4;
			const float4 q0 = tri[0], q1 = tri[1], q2 = tri[2], q3 = tri[3];
			if (need) {
				if (COUNT)
					++tri_tests;
				if (nearest_take(best, nearest_tri(q0, q1, q2, q3), leaf, q.x, q.y, q.z) && prune)
					limit2 = fminf(radius2, np_limit2(best.d2, magnitude));
			}
		}
		const uint32_t step = any ? 1u : (size ? size : 1u);
		at = (uint32_t) __builtin_amdgcn_readfirstlane((int) (at + step));
	}
	return best;
}

// COUNT: the counted form for tools/distance_bench.py (rt_debug_set_nearest_walk); the product's host code never launches it.
template <bool COUNT>
__global__ __launch_bounds__(64 * NEAREST_WAVES) void nearest_kernel(NearestArgs a) {
	const uint32_t k = blockIdx.x * (64u * NEAREST_WAVES) + threadIdx.x;
	const bool live = k < a.n;
	uint32_t idx = k;
	if (live && a.order)
		idx = a.order[k];
	float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	if (live)
		q = a.points[idx];
	const bool alive = live && np_point_ok(q.x, q.y, q.z) && np_radius_ok(a.max_distance);
	uint32_t node_tests = 0u, tri_tests = 0u;
	const Nearest best = nearest_walk<COUNT>(a, q, alive, node_tests, tri_tests);
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
	if (a.out.distance)
		a.out.distance[idx] = found ? distance : __builtin_inff();
	if (a.out.leaf)
		a.out.leaf[idx] = found ? best.leaf : NONE;
	store_record(a.out, idx, a.shade, best.leaf, found, found ? 1.0f - best.s - best.t : 0.0f, found ? best.s : 0.0f, found ? best.t : 0.0f,
	             found ? best.px : 0.0f, found ? best.py : 0.0f, found ? best.pz : 0.0f);
}

}  // namespace ocrt
