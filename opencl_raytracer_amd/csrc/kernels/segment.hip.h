// kernels/segment.hip.h -- segment queries: is the straight line between two points free, and where is it blocked first
// (include/rt_hip_segment.h)
// (part of the one translation unit kernels.hip; see its head for the passes and the arithmetic contract)
//
// A segment (a, b) is the ray o = a, d = b - a -- one subtraction per component, nothing normalised -- and an interval
// (t_lo, t_hi) of ray parameters, fractions of the segment.  The walk is the exact form (walk.hip.h, exact_walk) with
// max_distance = t_hi: the reference's slab test culls in ray-parameter units (`t_min < max_distance`), so with d = b - a
// "this box begins behind the far end" IS the node test, at no instruction's cost in the loop.  The triangle test is the
// reference's (tri_eval's operations in tri_eval's order, segment_tri_eval below) with the interval on the plane
// parameter r: r > t_lo, r < t_hi, both false for a NaN.
//
// segment_kernel<CLOSEST>: one segment per lane, a packet of 64 per wave, query_kernel's shape; the segments are ordered
// by query_key of (a, b - a) (segment_key_kernel, segment_scatter_kernel around query_scan_kernel).
// visibility_mask_kernel: P points against T targets without the P x T rays anywhere: ray r = slot * T + j is made in the
// lane from points[order[slot]] and targets[j] (slot = r / T by a multiplication, visibility_divisor); a packet is 64
// consecutive rays, its flags are balloted and the first lane of every run that shares a (point, mask word) ORs the run's
// bits into the point's row -- ao_mask_kernel's tail.  The POINTS are ordered by position (nearest_key_kernel);
// visibility_count_kernel, a thread per point, writes the popcounts.
#pragma once
#include "nearest.hip.h"

namespace ocrt {

// ---- coherence key of a segment: query_key of (a, b - a) -------------------------------------------------------------
// (QueryKeyArgs::origins holds the `from` points, QueryKeyArgs::directions the `to` points)
namespace {

__device__ __forceinline__ uint32_t segment_key(const QueryKeyArgs &a, uint32_t i) {
	const float4 from = a.origins[i], to = a.directions[i];
	return query_key(from, make_float4(to.x - from.x, to.y - from.y, to.z - from.z, 0.0f), a);
}

}  // namespace

__global__ __launch_bounds__(256) void segment_key_kernel(QueryKeyArgs a) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	const bool active = i < a.n;
	uint32_t key = 0u;
	if (active)
		key = segment_key(a, i);
	uint32_t leader, rank, size;
	wave_groups(key, active, leader, rank, size);
	if (active && rank == 0u)
		atomicAdd(&a.count[key], size);
	(void) leader;
}

__global__ __launch_bounds__(256) void segment_scatter_kernel(QueryKeyArgs a) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	const bool active = i < a.n;
	uint32_t key = 0u;
	if (active)
		key = segment_key(a, i);
	uint32_t leader, rank, size;
	wave_groups(key, active, leader, rank, size);
	uint32_t first = 0u;
	if (active && rank == 0u)
		first = atomicAdd(&a.count[key], size);
	first = (uint32_t) __shfl((int) first, (int) leader);
	if (active)
		a.order[first + rank] = i;
}

// ---- the triangle test with the interval ------------------------------------------------------------------------------
// tri_eval's operations in tri_eval's order (reference src/intersect_kernel.cl:65-114), and the plane parameter r = a / b
// (:79) held to the interval: `accepted` is "the reference accepts the triangle AND r > t_lo AND r < t_hi".  The interval
// is a rejection like the reference's own, so it is applied where r is known: a packet none of whose lanes is left in
// the running saves the two divisions for s and t.
template <bool CLOSEST>
__device__ __forceinline__ TriResult segment_tri_eval(const float4 q0, const float4 q1, const float4 q2, const float4 q3, const Ray &r,
                                                      float t_lo, float t_hi, float &plane_r) {
	const float tax = q0.x, tay = q0.y, taz = q0.z;
	const float ux = q0.w, uy = q1.x, uz = q1.y;
	const float vx = q1.z, vy = q1.w, vz = q2.x;
	const float nx = q2.y, ny = q2.z, nz = q2.w;
	const float uu = q3.x, uv = q3.y, vv = q3.z, D = q3.w;
	TriResult out;
	out.accepted = false;
	out.s = out.t = 0.0f;
	out.px = out.py = out.pz = 0.0f;
	out.distance = 0.0f;
	const float a = -dot3(nx, ny, nz, r.ox - tax, r.oy - tay, r.oz - taz);
	const float b = dot3(nx, ny, nz, r.dx, r.dy, r.dz);
	const float rr = a / b;
	plane_r = rr;
	// (`!(x > y)`: a NaN is outside the interval)
	bool reject = (fabsf(b) < 0.000001f) | (rr < 0.0f) | !(rr > t_lo) | !(rr < t_hi);
	if (wave_ballot(!reject) == 0ull)
		return out;
	const float ipx = r.ox + rr * r.dx, ipy = r.oy + rr * r.dy, ipz = r.oz + rr * r.dz;
	const float wx = ipx - tax, wy = ipy - tay, wz = ipz - taz;
	const float wu = dot3(ux, uy, uz, wx, wy, wz);
	const float wv = dot3(wx, wy, wz, vx, vy, vz);
	const float slack_hi = __uint_as_float(0x3F800053u);
	const float s = (uv * wv - vv * wu) / D;
	reject |= (s < -0.00001f) | (s > slack_hi);
	if (wave_ballot(!reject) == 0ull)
		return out;
	const float t = (uv * wu - uu * wv) / D;
	reject |= (t < -0.00001f) | ((s + t) > slack_hi);
	out.accepted = !reject;
	out.s = s;
	out.t = t;
	out.px = ipx; out.py = ipy; out.pz = ipz;
	if (CLOSEST) {
		const float ex = ipx - r.ox, ey = ipy - r.oy, ez = ipz - r.oz;
		out.distance = length3(ex, ey, ez);
	}
	return out;
}

// ---- the pair forms ---------------------------------------------------------------------------------------------------
struct SegmentArgs {
	const float4 *nodes_ptr;  // SceneBuffers::nodes: exact boxes, builder order (NodeRec)
	const float4 *tris_ptr;   // TriRec by leaf
	const float4 *shade;      // ShadeRec by leaf
	const float4 *from, *to;  // float4[n]
	const uint32_t *order;    // [n] segment of packet lane k, or null: segment k
	uint32_t n, node_count;
	float t_lo, t_hi;
	RecordOutputs out;        // by segment index; null: not written
	uint8_t *hit;             // by segment index, or null.  CLOSEST: the hit flag; ANY: the occlusion flag
};

// The ray of packet lane `k`: segment `idx` of the call (segment_kernel and its instanced form,
// kernels/instance_segments.hip.h).  A partial last packet's dead lanes get a ray that walks nothing and write nothing.
__device__ __forceinline__ Ray segment_packet_ray(const float4 *from, const float4 *to, const uint32_t *order, uint32_t n, uint32_t k,
                                                  bool &live, uint32_t &idx) {
	live = k < n;
	idx = k;
	if (live && order)
		idx = order[k];
	float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f), e = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
	if (live) {
		o = from[idx];
		e = to[idx];
	}
	return make_ray(o.x, o.y, o.z, e.x - o.x, e.y - o.y, e.z - o.z);
}

// CLOSEST: the record of the blocker with the minimum of (distance, leaf) -- closest_entry, nearer, take and closest_store,
// the closest hit's own.  ANY: a lane leaves the walk at its first blocker; the walk ends when the packet has no live lane.
template <bool CLOSEST>
__global__ __launch_bounds__(64 * QUERY_WAVES) void segment_kernel(SegmentArgs a) {
	bool live;
	uint32_t idx;
	const Ray ray = segment_packet_ray(a.from, a.to, a.order, a.n, blockIdx.x * (64u * QUERY_WAVES) + threadIdx.x, live, idx);
	const float t_lo = a.t_lo, t_hi = a.t_hi;
	bool alive = live, hit = false;
	Hit best = closest_entry();
	exact_walk(a.nodes_ptr, a.node_count, ray, t_hi, alive, [&](uint32_t leaf, bool box) {
		const float4 *tri = a.tris_ptr + LEAF_F4 * leaf + LEAF_TRI_F4;
		const float4 q0 = tri[0], q1 = tri[1], q2 = tri[2], q3 = tri[3];
		if (box) {
			float plane_r;
			const TriResult tr = segment_tri_eval<CLOSEST>(q0, q1, q2, q3, ray, t_lo, t_hi, plane_r);
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
	if (!CLOSEST) {
		if (a.hit)
			a.hit[idx] = hit ? 1u : 0u;
		return;
	}
	(void) closest_store(a.hit, a.out, idx, a.shade, hit, best);
}

// ---- the many-to-many form --------------------------------------------------------------------------------------------
struct VisibilityArgs {
	const float4 *nodes_ptr;  // SceneBuffers::nodes: exact boxes, builder order (NodeRec)
	const float4 *tris_ptr;   // TriRec by leaf
	const float4 *points;     // float4[np]
	const float4 *targets;    // float4[nt]
	const uint32_t *order;    // [np] point of slot j, or null: point j
	uint32_t *mask;           // [np][words] occlusion flags by point index, zeroed before the launch
	uint32_t np, nt;
	uint32_t words;           // ceil(nt / 32)
	uint32_t total;           // np * nt
	uint32_t magic, shift;    // r / nt = (r * magic) >> shift for every r < 2^27 (visibility_divisor)
	uint32_t node_count;
	float t_lo, t_hi;
};

// Division of a ray index by nt as a multiplication (Granlund and Montgomery, "Division by invariant integers using
// multiplication", 1994, theorem 4.2): with l = ceil(log2 nt) and magic = ceil(2^(27 + l) / nt), floor(r / nt) is
// (r * magic) >> (27 + l) for every r < 2^27 -- a call has at most RT_QUERY_MAX_RAYS = 2^27 rays.  magic <= 2^28, the
// product is below 2^55.
inline void visibility_divisor(uint32_t nt, uint32_t &magic, uint32_t &shift) {
	uint32_t l = 0u;
	while ((1ull << l) < nt)
		++l;
	shift = 27u + l;
	magic = (uint32_t) (((1ull << shift) + nt - 1u) / nt);
}

// Ray `r` of the P x T list: the point `idx` of slot r / nt towards target `j` (visibility_mask_kernel and its instanced
// form).  A partial last packet's dead lanes walk nothing and flag nothing.
__device__ __forceinline__ Ray visibility_ray(const VisibilityArgs &a, uint32_t r, bool &live, uint32_t &idx, uint32_t &j) {
	live = r < a.total;
	idx = 0u;
	j = 0u;
	float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f), e = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
	if (live) {
		// (r / nt by a multiplication: a 32-bit division is some thirty vector instructions, a tenth of a short walk)
		const uint32_t slot = (uint32_t) (((unsigned long long) r * a.magic) >> a.shift);
		j = r - slot * a.nt;
		idx = a.order ? a.order[slot] : slot;
		o = a.points[idx];
		e = a.targets[j];
	}
	return make_ray(o.x, o.y, o.z, e.x - o.x, e.y - o.y, e.z - o.z);
}

// The packet's flags by (point, mask word): the first lane of a run of lanes that shares both ORs the run's bits in.
__device__ __forceinline__ void visibility_mask_store(const VisibilityArgs &a, bool live, uint32_t idx, uint32_t j, bool hit) {
	const unsigned long long hits = wave_ballot(hit);
	if (!live)
		return;
	const uint32_t lane = threadIdx.x & 63u, bit = j & 31u;
	if (!(lane == 0u || j == 0u || bit == 0u))
		return;
	// the run ends with the word, with the point or with the packet: 1 .. 32 lanes
	uint32_t len = 32u - bit;
	len = a.nt - j < len ? a.nt - j : len;
	len = 64u - lane < len ? 64u - lane : len;
	const uint32_t flags = (uint32_t) ((hits >> lane) & ((1ull << len) - 1ull)) << bit;
	if (flags)
		atomicOr(&a.mask[(size_t) idx * a.words + (j >> 5)], flags);
}

__global__ __launch_bounds__(64 * QUERY_WAVES) void visibility_mask_kernel(VisibilityArgs a) {
	bool live;
	uint32_t idx, j;
	const Ray ray = visibility_ray(a, blockIdx.x * (64u * QUERY_WAVES) + threadIdx.x, live, idx, j);
	const float t_lo = a.t_lo, t_hi = a.t_hi;
	bool alive = live, hit = false;
	// a lane leaves at its first blocker
	exact_walk(a.nodes_ptr, a.node_count, ray, t_hi, alive, [&](uint32_t leaf, bool box) {
		const float4 *tri = a.tris_ptr + LEAF_F4 * leaf + LEAF_TRI_F4;
		const float4 q0 = tri[0], q1 = tri[1], q2 = tri[2], q3 = tri[3];
		if (box) {
			float plane_r;
			const TriResult tr = segment_tri_eval<false>(q0, q1, q2, q3, ray, t_lo, t_hi, plane_r);
			if (tr.accepted) {
				hit = true;
				alive = false;
			}
		}
		return wave_ballot(alive) == 0ull;
	});
	visibility_mask_store(a, live, idx, j, hit);
}

// One thread per point: the popcount of its row -- the targets the point does NOT see.
__global__ __launch_bounds__(256) void visibility_count_kernel(const uint32_t *mask, uint32_t *count, uint32_t np, uint32_t words) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= np)
		return;
	const uint32_t *const row = mask + (size_t) i * words;
	uint32_t sum = 0u;
	for (uint32_t w = 0; w < words; ++w)
		sum += (uint32_t) __popc(row[w]);
	count[i] = sum;
}

}  // namespace ocrt
