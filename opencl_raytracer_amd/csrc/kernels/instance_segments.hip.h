// kernels/instance_segments.hip.h -- instanced segment queries: is the straight line between two world-space points free of
// every posed copy of the scene, where is it blocked first, and the masks of many points against many targets
// (include/rt_hip_instance_segments.h)
// (part of the one translation unit kernels.hip; see its head for the passes and the arithmetic contract)
//
// A segment (a, b) is the WORLD ray o = a, d = b - a -- one subtraction per component, nothing normalised -- and an interval
// (t_lo, t_hi) of ray parameters.  An affine map keeps ray parameters, so the interval means the same in an instance's
// object space: the walk is instance_kernel's two nested exact walks (kernels/instances.hip.h has the rules) with
// max_distance = t_hi in both, and the leaf step is segment_tri_eval<false> (kernels/segment.hip.h) on the OBJECT ray: the
// reference's triangle test with r > t_lo and r < t_hi on its plane parameter, whose early-out ballots save the two
// divisions once no lane of the packet is left in the interval.  (Not segment_tri_eval<true>: its distance would be the
// object ray's.)  instance_segment_walk<CLOSEST> below is that walk as one function for the two kernels of this file; it
// has lines of its own, as instance_kernel and instance_walk have theirs, so that no existing kernel's device code moves
// (DESIGN.md section 23).
//
// instance_segment_kernel<CLOSEST>: segment_kernel's packet -- one segment per lane, 64 per wave, `order` --, the nested
// walk, and for CLOSEST the candidate's world position and distance from the world ray and the returned r, the minimum by
// instance_nearer, and instance_kernel's epilogue (the normal: the raw weighted sum, transpose(O), ONE normalisation).
// instance_visibility_kernel: visibility_mask_kernel's ray (slot = r / nt by visibility_divisor, the point through `order`,
// target j) and tail (ballot, the first lane of each (point, mask word) run ORs the run's bits with one vector atomic)
// around the nested walk in its occlusion form.  The sort's kernels, visibility_count_kernel and the scan are the plain
// forms' own.
#pragma once
#include "instances.hip.h"
#include "segment.hip.h"

namespace ocrt {

// Returns whether the lane has a blocker.  CLOSEST: every blocker goes to blocker(k, leaf, tr, r) -- instance, leaf, the
// object-space test's result and its plane parameter --, nobody leaves; else a lane leaves both walks at its first
// blocker, and both end once the packet has no lane left.
template <bool CLOSEST, class Blocker>
__device__ __forceinline__ bool instance_segment_walk(const float4 *top_ptr, uint32_t top_count, const float4 *inverses, const float4 *nodes_ptr,
                                                      uint32_t node_count, const float4 *tris_ptr, const Ray &ray, float t_lo, float t_hi,
                                                      bool live, Blocker &&blocker) {
	bool alive = live, hit = false;
	exact_walk(top_ptr, top_count, ray, t_hi, alive, [&](uint32_t k, bool entered) {
		// (k comes out of a scalar register: the rows arrive by scalar loads, into SGPRs)
		float4 m0, m1, m2;
		scalar_load_rows(inverses, k, m0, m1, m2);
		const float ox = ((m0.x * ray.ox + m0.y * ray.oy) + m0.z * ray.oz) + m0.w;
		const float oy = ((m1.x * ray.ox + m1.y * ray.oy) + m1.z * ray.oz) + m1.w;
		const float oz = ((m2.x * ray.ox + m2.y * ray.oy) + m2.z * ray.oz) + m2.w;
		const float dx = (m0.x * ray.dx + m0.y * ray.dy) + m0.z * ray.dz;
		const float dy = (m1.x * ray.dx + m1.y * ray.dy) + m1.z * ray.dz;
		const float dz = (m2.x * ray.dx + m2.y * ray.dy) + m2.z * ray.dz;
		// make_ray ballots: the whole wave calls it, the lanes that did not enter with a ray that walks nothing
		const Ray object = make_ray(entered ? ox : 0.0f, entered ? oy : 0.0f, entered ? oz : 0.0f, entered ? dx : 1.0f, entered ? dy : 1.0f,
		                            entered ? dz : 1.0f);
		bool inside = entered;  // (`entered` implies `alive`: exact_box)
		exact_walk(nodes_ptr, node_count, object, t_hi, inside, [&](uint32_t leaf, bool box) {
			const float4 *tri = tris_ptr + LEAF_F4 * leaf + LEAF_TRI_F4;
			const float4 q0 = tri[0], q1 = tri[1], q2 = tri[2], q3 = tri[3];
			if (box) {
				float r;
				const TriResult tr = segment_tri_eval<false>(q0, q1, q2, q3, object, t_lo, t_hi, r);
				if (tr.accepted) {
					hit = true;
					if (CLOSEST) {
						blocker(k, leaf, tr, r);
					} else {
						alive = false;
						inside = false;
					}
				}
			}
			return !CLOSEST && wave_ballot(inside) == 0ull;
		});
		return !CLOSEST && wave_ballot(alive) == 0ull;
	});
	return hit;
}

// ---- the pair forms ---------------------------------------------------------------------------------------------------
struct InstanceSegmentArgs : SegmentArgs {  // (nodes_ptr, tris_ptr, shade: the scene's own; t_lo, t_hi: in both spaces)
	const float4 *top_ptr;   // the top-level tree: NodeRec[top_count], `leaf` the instance index
	const float4 *inverses;  // object_from_world, three float4 rows per instance
	uint32_t top_count;      // 2 * instances - 1
	uint32_t *instance;      // by segment index, or null (CLOSEST)
};

template <bool CLOSEST>
__global__ __launch_bounds__(64 * QUERY_WAVES) void instance_segment_kernel(InstanceSegmentArgs a) {
	const uint32_t k = blockIdx.x * (64u * QUERY_WAVES) + threadIdx.x;
	const bool live = k < a.n;  // (a partial last packet: its dead lanes walk nothing and write nothing)
	uint32_t idx = k;
	if (live && a.order)
		idx = a.order[k];
	float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f), e = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
	if (live) {
		o = a.from[idx];
		e = a.to[idx];
	}
	const Ray ray = make_ray(o.x, o.y, o.z, e.x - o.x, e.y - o.y, e.z - o.z);
	Hit best = closest_entry();
	uint32_t best_instance = 0u;
	const bool hit = instance_segment_walk<CLOSEST>(a.top_ptr, a.top_count, a.inverses, a.nodes_ptr, a.node_count, a.tris_ptr, ray, a.t_lo,
	                                                a.t_hi, live, [&](uint32_t inst, uint32_t leaf, const TriResult &tr, float r) {
		                                                // the record is the WORLD ray's: an affine map keeps r
		                                                const float px = ray.ox + r * ray.dx, py = ray.oy + r * ray.dy, pz = ray.oz + r * ray.dz;
		                                                const float distance = length3(px - ray.ox, py - ray.oy, pz - ray.oz);
		                                                if (instance_nearer(distance, inst, leaf, best, best_instance)) {
			                                                best.distance = distance;
			                                                best.leaf = leaf;
			                                                best.s = tr.s;
			                                                best.t = tr.t;
			                                                best.px = px; best.py = py; best.pz = pz;
			                                                best_instance = inst;
		                                                }
	                                                });
	if (!live)
		return;
	if (a.hit)
		a.hit[idx] = hit ? 1u : 0u;
	if (!CLOSEST)
		return;
	// the record, as instance_kernel<true> writes it
	const bool kept = hit && best.distance < __builtin_inff();  // (the record was replaced at least once)
	if (a.instance)
		a.instance[idx] = hit ? best_instance : NONE;
	if (a.out.distance)
		a.out.distance[idx] = best.distance;
	if (a.out.leaf)
		a.out.leaf[idx] = hit ? best.leaf : NONE;
	const float b0 = kept ? 1.0f - best.s - best.t : 0.0f, b1 = kept ? best.s : 0.0f, b2 = kept ? best.t : 0.0f;
	if (a.out.barycentric) {
		a.out.barycentric[3u * (size_t) idx + 0u] = b0;
		a.out.barycentric[3u * (size_t) idx + 1u] = b1;
		a.out.barycentric[3u * (size_t) idx + 2u] = b2;
	}
	if (a.out.position) {
		a.out.position[3u * (size_t) idx + 0u] = kept ? best.px : 0.0f;
		a.out.position[3u * (size_t) idx + 1u] = kept ? best.py : 0.0f;
		a.out.position[3u * (size_t) idx + 2u] = kept ? best.pz : 0.0f;
	}
	if (a.out.normal) {
		// get_smooth_normal's weighted sum in the object's frame, the inverse's transpose, ONE normalisation
		float wx = 0.0f, wy = 0.0f, wz = 0.0f;
		if (hit) {
			const float4 n0 = a.shade[3 * (size_t) best.leaf + 0], n1 = a.shade[3 * (size_t) best.leaf + 1], n2 = a.shade[3 * (size_t) best.leaf + 2];
			const float rx = (n0.x * b0 + n1.x * b1) + n2.x * b2;
			const float ry = (n0.y * b0 + n1.y * b1) + n2.y * b2;
			const float rz = (n0.z * b0 + n1.z * b1) + n2.z * b2;
			const float4 *rows = a.inverses + 3u * (size_t) best_instance;
			const float4 m0 = rows[0], m1 = rows[1], m2 = rows[2];
			wx = (m0.x * rx + m1.x * ry) + m2.x * rz;
			wy = (m0.y * rx + m1.y * ry) + m2.y * rz;
			wz = (m0.z * rx + m1.z * ry) + m2.z * rz;
			normalize3(wx, wy, wz);
		}
		a.out.normal[3u * (size_t) idx + 0u] = wx;
		a.out.normal[3u * (size_t) idx + 1u] = wy;
		a.out.normal[3u * (size_t) idx + 2u] = wz;
	}
}

// ---- the many-to-many form --------------------------------------------------------------------------------------------
struct InstanceVisibilityArgs : VisibilityArgs {  // (nodes_ptr, tris_ptr: the scene's own; points and targets in world space)
	const float4 *top_ptr;   // the top-level tree
	const float4 *inverses;  // object_from_world, three float4 rows per instance
	uint32_t top_count;
};

__global__ __launch_bounds__(64 * QUERY_WAVES) void instance_visibility_kernel(InstanceVisibilityArgs a) {
	const uint32_t r = blockIdx.x * (64u * QUERY_WAVES) + threadIdx.x;
	const bool live = r < a.total;  // (a partial last packet: its dead lanes walk nothing and flag nothing)
	uint32_t idx = 0u, j = 0u;
	float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f), e = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
	if (live) {
		// (r / nt by a multiplication, as visibility_mask_kernel)
		const uint32_t slot = (uint32_t) (((unsigned long long) r * a.magic) >> a.shift);
		j = r - slot * a.nt;
		idx = a.order ? a.order[slot] : slot;
		o = a.points[idx];
		e = a.targets[j];
	}
	const Ray ray = make_ray(o.x, o.y, o.z, e.x - o.x, e.y - o.y, e.z - o.z);
	const bool hit = instance_segment_walk<false>(a.top_ptr, a.top_count, a.inverses, a.nodes_ptr, a.node_count, a.tris_ptr, ray, a.t_lo, a.t_hi,
	                                              live, [](uint32_t, uint32_t, const TriResult &, float) {});
	// the packet's flags by (point, mask word): the first lane of a run of lanes that shares both ORs the run's bits in
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

}  // namespace ocrt
