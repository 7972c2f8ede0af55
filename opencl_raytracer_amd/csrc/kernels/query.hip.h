// kernels/query.hip.h -- ray queries: closest hit and occlusion for rays the caller supplies (include/rt_hip_query.h)
// (part of the one translation unit kernels.hip; see its head for the passes and the arithmetic contract)
//
// Three small kernels order the rays by a coherence key (query_key_kernel: histogram, query_scan_kernel: exclusive
// scan of the counts, query_scatter_kernel: the permutation), then query_kernel<CLOSEST> casts one packet of 64 rays per
// wave and writes every result back to the ray's own index.  The order only decides which rays share a packet: each
// result is the ray's own, so any order gives the same bits (and the order inside a bucket, which depends on how the
// waves' atomics land, is free to vary from call to call).
//
// The walk is the EXACT form of the shared walk (walk.hip.h, exact_walk) over the uploaded scene's
// exact node records (SceneBuffers::nodes, builder order): every lane runs the reference's own slab test
// (src/intersect_kernel.cl:21-61, slab_hit) where its own walk stands, so lane by lane it is the reference's
// scene_intersect (:184-213) whatever the ray holds -- zero, tiny, huge or non-finite components, far origins, any
// max_distance.  The padded records of the fast form are not used: their margins (scene_pack.cc, padded_bound) are
// proven for the frame's rays (the camera, and unit directions from hit points within the AO reach), not for rays from
// anywhere; DESIGN.md section 9 says what that costs.
#pragma once
#include "walk.hip.h"

namespace ocrt {

// ---- coherence key and counting sort --------------------------------------------------------------------------------
constexpr uint32_t QUERY_KEY_BITS = 16u, QUERY_BUCKETS = 1u << QUERY_KEY_BITS;
constexpr uint32_t QUERY_SCAN_THREADS = 1024u, QUERY_SCAN_PER_THREAD = QUERY_BUCKETS / QUERY_SCAN_THREADS;

struct QueryKeyArgs {
	const float4 *origins, *directions;
	const uint32_t *index;   // (scatter) null: ray k is rays[k]
	uint32_t *count;         // [QUERY_BUCKETS]: the histogram (key kernel), then the running cursors (scatter kernel)
	uint32_t *order;         // [n] (scatter): ray indices in key order
	uint32_t n;
	float lo[3], scale[3];   // origin quantisation: cell = (o - lo) * scale, 8 cells per axis inside the scene box
};

namespace {

// 16-bit key of a ray: bits 15..13 the sign octant of its direction (bit set: component >= +0, the side the reference's
// `div >= 0` puts the near plane on), bits 12..4 the Morton code of its origin's cell -- 8 x 8 x 8 cells over the scene's
// box --, bits 3..0 a coarse direction cell: |d_x| and |d_y| as shares of |d_x| + |d_y| + |d_z|, 2 bits each.  Origins
// outside the box (clamped to its border cells beyond half a box), non-finite ones and non-finite directions: 0xFFFF.
__device__ __forceinline__ uint32_t query_key(const float4 o, const float4 d, const QueryKeyArgs &a) {
	const float cx = (o.x - a.lo[0]) * a.scale[0], cy = (o.y - a.lo[1]) * a.scale[1], cz = (o.z - a.lo[2]) * a.scale[2];
	const float sum = fabsf(d.x) + fabsf(d.y) + fabsf(d.z);
	// (NaN fails every comparison: such rays take the last bucket)
	const bool near_box = cx >= -4.0f && cx <= 12.0f && cy >= -4.0f && cy <= 12.0f && cz >= -4.0f && cz <= 12.0f;
	if (!near_box || !(sum > 0.0f && sum <= 3.0e38f))
		return QUERY_BUCKETS - 1u;
	const uint32_t qx = (uint32_t) fminf(fmaxf(cx, 0.0f), 7.0f), qy = (uint32_t) fminf(fmaxf(cy, 0.0f), 7.0f);
	const uint32_t qz = (uint32_t) fminf(fmaxf(cz, 0.0f), 7.0f);
	uint32_t morton = 0u;
	for (uint32_t b = 0; b < 3u; ++b)
		morton |= (((qx >> b) & 1u) << (3u * b)) | (((qy >> b) & 1u) << (3u * b + 1u)) | (((qz >> b) & 1u) << (3u * b + 2u));
	const uint32_t sx = (uint32_t) fminf(fabsf(d.x) / sum * 4.0f, 3.0f), sy = (uint32_t) fminf(fabsf(d.y) / sum * 4.0f, 3.0f);
	const uint32_t octant = (__builtin_signbit(d.x) ? 0u : 1u) | (__builtin_signbit(d.y) ? 0u : 2u) | (__builtin_signbit(d.z) ? 0u : 4u);
	return octant << 13 | morton << 4 | sx << 2 | sy;
}

// The wave's lanes grouped by equal `key`: the lowest lane of each group (`leader`), this lane's rank in its group and
// the group's size -- so that one atomic per group and wave stands for all its lanes (one round per distinct key).
__device__ __forceinline__ void wave_groups(uint32_t key, bool active, uint32_t &leader, uint32_t &rank, uint32_t &size) {
	const uint32_t lane = fresh_lane();
	unsigned long long left = wave_ballot(active);
	leader = rank = size = 0u;
	while (left != 0ull) {
		const uint32_t first = (uint32_t) __builtin_ctzll(left);
		const uint32_t k = (uint32_t) __builtin_amdgcn_readlane((int) key, (int) first);
		const unsigned long long same = wave_ballot(active && key == k) & left;
		if ((same >> lane) & 1ull) {
			leader = first;
			rank = (uint32_t) __popcll(same & ((1ull << lane) - 1ull));
			size = (uint32_t) __popcll(same);
		}
		left &= ~same;
	}
}

}  // namespace

__global__ __launch_bounds__(256) void query_key_kernel(QueryKeyArgs a) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	const bool active = i < a.n;
	uint32_t key = 0u;
	if (active)
		key = query_key(a.origins[i], a.directions[i], a);
	uint32_t leader, rank, size;
	wave_groups(key, active, leader, rank, size);
	if (active && rank == 0u)
		atomicAdd(&a.count[key], size);
	(void) leader;
}

// One workgroup: count[] becomes its exclusive prefix sum (each thread a run of QUERY_SCAN_PER_THREAD buckets).
__global__ __launch_bounds__(QUERY_SCAN_THREADS) void query_scan_kernel(uint32_t *count) {
	__shared__ uint32_t partial[QUERY_SCAN_THREADS];
	const uint32_t t = threadIdx.x, base = t * QUERY_SCAN_PER_THREAD;
	uint32_t sum = 0u;
	for (uint32_t j = 0; j < QUERY_SCAN_PER_THREAD; ++j)
		sum += count[base + j];
	partial[t] = sum;
	__syncthreads();
	for (uint32_t step = 1u; step < QUERY_SCAN_THREADS; step <<= 1) {  // inclusive scan of the runs' sums (Hillis-Steele)
		const uint32_t add = t >= step ? partial[t - step] : 0u;
		__syncthreads();
		partial[t] += add;
		__syncthreads();
	}
	uint32_t running = partial[t] - sum;
	for (uint32_t j = 0; j < QUERY_SCAN_PER_THREAD; ++j) {
		const uint32_t c = count[base + j];
		count[base + j] = running;
		running += c;
	}
}

__global__ __launch_bounds__(256) void query_scatter_kernel(QueryKeyArgs a) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	const bool active = i < a.n;
	uint32_t key = 0u;
	if (active)
		key = query_key(a.origins[i], a.directions[i], a);
	uint32_t leader, rank, size;
	wave_groups(key, active, leader, rank, size);
	uint32_t first = 0u;
	if (active && rank == 0u)
		first = atomicAdd(&a.count[key], size);
	first = (uint32_t) __shfl((int) first, (int) leader);
	if (active)
		a.order[first + rank] = i;
}

// ---- the queries ----------------------------------------------------------------------------------------------------
// What the kernels that cast caller-supplied rays are launched with (query_kernel, kernels/multihit.hip.h).
struct RayQueryArgs {
	const float4 *nodes_ptr;  // SceneBuffers::nodes: exact boxes, builder order (NodeRec)
	const float4 *tris_ptr;   // TriRec by leaf
	const float4 *shade;      // ShadeRec by leaf
	const float4 *origins, *directions;  // float4[n]
	const uint32_t *order;    // [n] ray of packet lane k, or null: ray k
	uint32_t n, node_count;
	float max_distance;
	RecordOutputs out;        // by ray index, or by ray and slot; null: not written
};
struct QueryArgs : RayQueryArgs {
	uint8_t *hit;  // by ray index, or null.  CLOSEST: the hit flag; ANY: the occlusion flag
};

constexpr uint32_t QUERY_WAVES = 4u;

// The ray of packet lane `k`: ray `idx` of the call.  A partial last packet's dead lanes (`live` false) get a ray that
// walks nothing and write nothing.
__device__ __forceinline__ Ray packet_ray(const RayQueryArgs &a, uint32_t k, bool &live, uint32_t &idx) {
	live = k < a.n;
	idx = k;
	if (live && a.order)
		idx = a.order[k];
	float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f), d = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
	if (live) {
		o = a.origins[idx];
		d = a.directions[idx];
	}
	return make_ray(o.x, o.y, o.z, d.x, d.y, d.z);
}

// Barycentrics, point and normal of a record into `slot` of the arrays that were asked for.  The normal is
// normal(nx, ny, nz)'s, called only where one is asked for and the record is `shaded`; else zeros.
template <class Normal>
__device__ __forceinline__ void store_record(const RecordOutputs &out, size_t slot, bool shaded, float b0, float b1, float b2, float px, float py,
                                             float pz, Normal &&normal) {
	if (out.barycentric) {
		out.barycentric[3u * slot + 0u] = b0;
		out.barycentric[3u * slot + 1u] = b1;
		out.barycentric[3u * slot + 2u] = b2;
	}
	if (out.position) {
		out.position[3u * slot + 0u] = px;
		out.position[3u * slot + 1u] = py;
		out.position[3u * slot + 2u] = pz;
	}
	if (out.normal) {
		float nx = 0.0f, ny = 0.0f, nz = 0.0f;
		if (shaded)
			normal(nx, ny, nz);
		out.normal[3u * slot + 0u] = nx;
		out.normal[3u * slot + 1u] = ny;
		out.normal[3u * slot + 2u] = nz;
	}
}

// The plain kernels' form: the smooth normal of `leaf` (smooth_normal).
__device__ __forceinline__ void store_record(const RecordOutputs &out, size_t slot, const float4 *shade, uint32_t leaf, bool shaded,
                                             float b0, float b1, float b2, float px, float py, float pz) {
	store_record(out, slot, shaded, b0, b1, b2, px, py, pz, [&](float &nx, float &ny, float &nz) { smooth_normal(shade, leaf, b0, b1, b2, nx, ny, nz); });
}

// The closest-hit record of one ray, CLOSEST's contract below, for the kernels that make their own rays (layers_kernel).
// closest_entry: its state on entry to the walk -- isect.distance = INFINITY, the other fields 0, as the CPU oracle starts them.
__device__ __forceinline__ Hit closest_entry() {
	Hit best;
	best.distance = __builtin_inff();
	best.leaf = 0u;
	best.s = best.t = 0.0f;
	best.px = best.py = best.pz = 0.0f;
	return best;
}

// What closest_store wrote of the record where it was kept (zeros otherwise), for the epilogues that go on from it.
struct ClosestRecord {
	float b0, b1, b2, px, py, pz;
};

// closest_store: the boolean and the record into `slot` of the arrays that were asked for.  Where some triangle is accepted
// but none replaces the record (a distance of +inf or NaN) the record keeps its entry values -- leaf 0, barycentrics and
// point 0, distance +inf.  The smooth normal is the reference's get_smooth_normal for that record (smooth_normal, as the
// primary pass computes it).
__device__ __forceinline__ ClosestRecord closest_store(uint8_t *hit_flags, const RecordOutputs &out, size_t slot, const float4 *shade, bool hit,
                                                       const Hit &best) {
	if (hit_flags)
		hit_flags[slot] = hit ? 1u : 0u;
	const bool kept = hit && best.distance < __builtin_inff();  // (the record was replaced at least once)
	ClosestRecord r;
	r.b0 = kept ? 1.0f - best.s - best.t : 0.0f;
	r.b1 = kept ? best.s : 0.0f;
	r.b2 = kept ? best.t : 0.0f;
	r.px = kept ? best.px : 0.0f;
	r.py = kept ? best.py : 0.0f;
	r.pz = kept ? best.pz : 0.0f;
	if (out.distance)
		out.distance[slot] = best.distance;
	if (out.leaf)
		out.leaf[slot] = hit ? best.leaf : NONE;
	store_record(out, slot, shade, best.leaf, hit, r.b0, r.b1, r.b2, r.px, r.py, r.pz);
	return r;
}

// CLOSEST: the reference's scene_intersect with isect.distance = INFINITY on entry (the other fields 0, as the CPU oracle
// starts them): the boolean, and the record of the nearest accepted triangle with the lowest leaf index among equal
// distances (nearer()); where some triangle is accepted but none replaces the record (a distance of +inf or NaN) the
// record keeps its entry values -- leaf 0, barycentrics and point 0, distance +inf.  The smooth normal is the reference's
// get_smooth_normal for that record (smooth_normal, as the primary pass computes it).
// ANY: the same boolean; a lane leaves the walk at its first accepted triangle.
// (query_kernel keeps lines of its own for the entry state and the store: written through the helpers above, the compiler
// schedules query_kernel<true> differently -- 499 instructions for 494 -- and that kernel is not to move.  The leaf step
// stays in each kernel's own lambda: as a function of its own it costs the walk loop three scalar instructions a turn.)
template <bool CLOSEST>
__global__ __launch_bounds__(64 * QUERY_WAVES) void query_kernel(QueryArgs a) {
	bool live;
	uint32_t idx;
	const Ray ray = packet_ray(a, blockIdx.x * (64u * QUERY_WAVES) + threadIdx.x, live, idx);
	bool alive = live, hit = false;
	Hit best;
	best.distance = __builtin_inff();
	best.leaf = 0u;
	best.s = best.t = 0.0f;
	best.px = best.py = best.pz = 0.0f;
	exact_walk(a.nodes_ptr, a.node_count, ray, a.max_distance, alive, [&](uint32_t leaf, bool box) {
		const float4 *tri = a.tris_ptr + LEAF_F4 * leaf + LEAF_TRI_F4;
		const float4 q0 = tri[0], q1 = tri[1], q2 = tri[2], q3 = tri[3];
		if (box) {
			const TriResult tr = tri_eval<CLOSEST>(q0, q1, q2, q3, ray);
			if (tr.accepted) {
				hit = true;
				if (CLOSEST) {
					if (nearer(tr.distance, leaf, best))
						take(best, tr, leaf);
				} else {
					alive = false;
				}
			}
		}
		return !CLOSEST && wave_ballot(alive) == 0ull;
	});
	if (!live)
		return;
	if (a.hit)
		a.hit[idx] = hit ? 1u : 0u;
	if (!CLOSEST)
		return;
	const bool kept = hit && best.distance < __builtin_inff();  // (the record was replaced at least once)
	if (a.out.distance)
		a.out.distance[idx] = best.distance;
	if (a.out.leaf)
		a.out.leaf[idx] = hit ? best.leaf : NONE;
	store_record(a.out, idx, a.shade, best.leaf, hit, kept ? 1.0f - best.s - best.t : 0.0f, kept ? best.s : 0.0f, kept ? best.t : 0.0f,
	             kept ? best.px : 0.0f, kept ? best.py : 0.0f, kept ? best.pz : 0.0f);
}

}  // namespace ocrt
