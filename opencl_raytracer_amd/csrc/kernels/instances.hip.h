// kernels/instances.hip.h -- instanced ray queries: closest hit and occlusion against posed copies of the uploaded scene
// under a top-level tree (include/rt_hip_instances.h), and what every instanced kernel shares: the set, the nested walk, the
// closest candidate and the record's epilogue
// (part of the one translation unit kernels.hip; see its head for the passes and the arithmetic contract)
//
// instance_walk<CLOSEST> is two nested exact walks (walk.hip.h, exact_walk).  The OUTER walk runs over the top-level records
// (csrc/instances.cc) with the world ray: lane by lane the reference's slab test where the lane's own walk stands, so a lane
// ENTERS an instance iff every box on the way to its leaf passes.  At a leaf the instance index is wave-uniform: the twelve
// floats of its object_from_world arrive by scalar loads, every lane forms its object ray (instance_object_ray: products and
// sums in the header's order, each rounded on its own) and the INNER walk runs over the scene's own records with `alive && entered`
// as its `alive`.  Its leaf step is the caller's triangle test on the OBJECT ray handing the plane parameter r back: for
// rays, ambient occlusion and layers tri_eval's operations in tri_eval's order (instance_tri_eval; not segment_tri_eval,
// whose interval rejects a NaN r), for segments and masks segment_tri_eval<false> with the call's interval.  An affine map
// keeps ray parameters, so a candidate's world position is o + r d with the WORLD ray, and the distance its length from o
// (instance_candidate).  Nothing is pruned by the best distance so far: the reference's walk has no such step.  In the
// occlusion form a lane leaves both walks at its first candidate, and both end once the packet has no lane left.
//
// instance_kernel<CLOSEST>: a ray per lane, a packet of 64 per wave, query_kernel's shape, around that walk -- written out in
// the kernel, the one caller that measured slower through the function; the candidate and the
// record's epilogue are the shared ones.
//
// The record's epilogue of every instanced kernel that writes one is instance_store_record: query.hip.h's store_record with
// instance_normal for the normal (the instanced multi-hit resolve: the same two inside multihit.hip.h's resolve body).
// (instance_layers_kernel alone forms the normal itself: the head-light term and the ambient-occlusion list read it.)
#pragma once
#include "query.hip.h"

namespace ocrt {

// The instance set on the device, as every instanced kernel is handed it.
struct InstanceSet {
	const float4 *top_ptr;   // the top-level tree: NodeRec[top_count], `leaf` the instance index
	const float4 *inverses;  // object_from_world, three float4 rows per instance
	uint32_t top_count;      // 2 * instances - 1
};

struct InstanceArgs : RayQueryArgs {  // (nodes_ptr, tris_ptr, shade: the scene's own; max_distance: the call's, in both spaces)
	InstanceSet set;
	uint8_t *hit;             // by ray index, or null.  CLOSEST: the hit flag; ANY: the occlusion flag
	uint32_t *instance;       // by ray index, or null (CLOSEST)
};

// The three rows of instance k's object_from_world by scalar loads (asm, as scalar_load_node: plain loads through the
// pointer become vector loads of one address into twelve VGPRs).  `k` is wave-uniform.
typedef unsigned int u32x4s __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void scalar_load_rows(const float4 *inverses, uint32_t k, float4 &m0, float4 &m1, float4 &m2) {
	u32x8 r01;
	u32x4s r2;
	const uint32_t offset = (uint32_t) __builtin_amdgcn_readfirstlane((int) (k * 48u));
	asm volatile("s_load_dwordx8 %0, %2, %3\n\ts_load_dwordx4 %1, %2, %3 offset:32\n\ts_waitcnt lgkmcnt(0)"
	             : "=&s"(r01), "=&s"(r2)
	             : "s"(inverses), "s"(offset));
	m0 = make_float4(__uint_as_float(r01[0]), __uint_as_float(r01[1]), __uint_as_float(r01[2]), __uint_as_float(r01[3]));
	m1 = make_float4(__uint_as_float(r01[4]), __uint_as_float(r01[5]), __uint_as_float(r01[6]), __uint_as_float(r01[7]));
	m2 = make_float4(__uint_as_float(r2[0]), __uint_as_float(r2[1]), __uint_as_float(r2[2]), __uint_as_float(r2[3]));
}

// tri_eval<false> (reference src/intersect_kernel.cl:65-114) that also says r = a / b (:79).
__device__ __forceinline__ TriResult instance_tri_eval(const float4 q0, const float4 q1, const float4 q2, const float4 q3, const Ray &r,
                                                       float &plane_r) {
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
	bool reject = (fabsf(b) < 0.000001f) | (rr < 0.0f);
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
	return out;
}

// The object ray of a world ray under the rows m0, m1, m2 of an object_from_world: origin O o + t, direction O d, products
// and sums in the header's order.
__device__ __forceinline__ void instance_object_ray(const float4 m0, const float4 m1, const float4 m2, float wox, float woy, float woz, float wdx,
                                                    float wdy, float wdz, float &ox, float &oy, float &oz, float &dx, float &dy, float &dz) {
	ox = ((m0.x * wox + m0.y * woy) + m0.z * woz) + m0.w;
	oy = ((m1.x * wox + m1.y * woy) + m1.z * woz) + m1.w;
	oz = ((m2.x * wox + m2.y * woy) + m2.z * woz) + m2.w;
	dx = (m0.x * wdx + m0.y * wdy) + m0.z * wdz;
	dy = (m1.x * wdx + m1.y * wdy) + m1.z * wdz;
	dz = (m2.x * wdx + m2.y * wdy) + m2.z * wdz;
}

// nearer() with the instance between the distance and the leaf: a strictly smaller distance wins, and among equal
// distances below +inf the lower (instance, leaf) pair -- the top-level tree lists the instances in an order of its own.
__device__ __forceinline__ bool instance_nearer(float distance, uint32_t instance, uint32_t leaf, const Hit &best, uint32_t best_instance) {
	const bool lower = instance < best_instance || (instance == best_instance && leaf < best.leaf);
	return best.distance > distance || (best.distance == distance && lower && distance < __builtin_inff());
}

// The nested walk.  Returns whether the lane has a candidate: a leaf whose triangle leaf_test(q0, q1, q2, q3, object, r)
// accepts for the lane's object ray, r the test's plane parameter.  CLOSEST: every candidate goes to candidate(k, leaf, tr,
// r) -- instance, leaf, the object-space test's result and r --, nobody leaves; else a lane leaves both walks at its first
// candidate, and both end once the packet has no lane left.
template <bool CLOSEST, class LeafTest, class Candidate>
__device__ __forceinline__ bool instance_walk(const InstanceSet &set, const float4 *nodes_ptr, uint32_t node_count, const float4 *tris_ptr,
                                              const Ray &ray, float max_distance, bool live, LeafTest &&leaf_test, Candidate &&candidate) {
	bool alive = live, hit = false;
	exact_walk(set.top_ptr, set.top_count, ray, max_distance, alive, [&](uint32_t k, bool entered) {
		// (k comes out of a scalar register: the rows arrive by scalar loads, into SGPRs)
		float4 m0, m1, m2;
		scalar_load_rows(set.inverses, k, m0, m1, m2);
		float ox, oy, oz, dx, dy, dz;
		instance_object_ray(m0, m1, m2, ray.ox, ray.oy, ray.oz, ray.dx, ray.dy, ray.dz, ox, oy, oz, dx, dy, dz);
		// make_ray ballots: the whole wave calls it, the lanes that did not enter with a ray that walks nothing
		const Ray object = make_ray(entered ? ox : 0.0f, entered ? oy : 0.0f, entered ? oz : 0.0f, entered ? dx : 1.0f, entered ? dy : 1.0f,
		                            entered ? dz : 1.0f);
		bool inside = entered;  // (`entered` implies `alive`: exact_box)
		exact_walk(nodes_ptr, node_count, object, max_distance, inside, [&](uint32_t leaf, bool box) {
			const float4 *tri = tris_ptr + LEAF_F4 * leaf + LEAF_TRI_F4;
			const float4 q0 = tri[0], q1 = tri[1], q2 = tri[2], q3 = tri[3];
			if (box) {
				float r;
				const TriResult tr = leaf_test(q0, q1, q2, q3, object, r);
				if (tr.accepted) {
					hit = true;
					if (CLOSEST) {
						candidate(k, leaf, tr, r);
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

// The leaf test of rays, ambient occlusion and layers, and the candidate of the occlusion forms, which is never called.
struct InstanceTriEval {
	__device__ __forceinline__ TriResult operator()(const float4 q0, const float4 q1, const float4 q2, const float4 q3, const Ray &object,
	                                                float &r) const {
		return instance_tri_eval(q0, q1, q2, q3, object, r);
	}
};
struct NoCandidate {
	__device__ __forceinline__ void operator()(uint32_t, uint32_t, const TriResult &, float) const {}
};

// A candidate of the closest forms: the record is the WORLD ray's (an affine map keeps r), the minimum by instance_nearer.
__device__ __forceinline__ void instance_candidate(const Ray &ray, uint32_t k, uint32_t leaf, const TriResult &tr, float r, Hit &best,
                                                   uint32_t &best_instance) {
	const float px = ray.ox + r * ray.dx, py = ray.oy + r * ray.dy, pz = ray.oz + r * ray.dz;
	const float distance = length3(px - ray.ox, py - ray.oy, pz - ray.oz);
	if (instance_nearer(distance, k, leaf, best, best_instance)) {
		best.distance = distance;
		best.leaf = leaf;
		best.s = tr.s;
		best.t = tr.t;
		best.px = px; best.py = py; best.pz = pz;
		best_instance = k;
	}
}

// The instanced record's normal where there is a hit: get_smooth_normal's weighted sum in the object's frame, the inverse's
// transpose, ONE normalisation.
__device__ __forceinline__ void instance_normal(const float4 *shade, const float4 *inverses, uint32_t leaf, uint32_t instance, float b0,
                                                float b1, float b2, float &wx, float &wy, float &wz) {
	const float4 n0 = shade[3 * (size_t) leaf + 0], n1 = shade[3 * (size_t) leaf + 1], n2 = shade[3 * (size_t) leaf + 2];
	const float rx = (n0.x * b0 + n1.x * b1) + n2.x * b2;
	const float ry = (n0.y * b0 + n1.y * b1) + n2.y * b2;
	const float rz = (n0.z * b0 + n1.z * b1) + n2.z * b2;
	const float4 *rows = inverses + 3u * (size_t) instance;
	const float4 m0 = rows[0], m1 = rows[1], m2 = rows[2];
	wx = (m0.x * rx + m1.x * ry) + m2.x * rz;
	wy = (m0.y * rx + m1.y * ry) + m2.y * rz;
	wz = (m0.z * rx + m1.z * ry) + m2.z * rz;
	normalize3(wx, wy, wz);
}

// The instanced record's epilogue: store_record (query.hip.h) with instance_normal.
__device__ __forceinline__ void instance_store_record(const RecordOutputs &out, size_t slot, const float4 *shade, const float4 *inverses,
                                                      uint32_t leaf, uint32_t instance, bool shaded, float b0, float b1, float b2, float px,
                                                      float py, float pz) {
	store_record(out, slot, shaded, b0, b1, b2, px, py, pz,
	             [&](float &wx, float &wy, float &wz) { instance_normal(shade, inverses, leaf, instance, b0, b1, b2, wx, wy, wz); });
}

// The closest forms' record into `idx` of the arrays that were asked for (the flag is the caller's).  Where some triangle
// is accepted but none replaces the record it keeps its entry values, as closest_store's does.
__device__ __forceinline__ void instance_record_store(const RecordOutputs &out, uint32_t *instance, uint32_t idx, const float4 *shade,
                                                      const float4 *inverses, bool hit, const Hit &best, uint32_t best_instance) {
	const bool kept = hit && best.distance < __builtin_inff();  // (the record was replaced at least once)
	if (instance)
		instance[idx] = hit ? best_instance : NONE;
	if (out.distance)
		out.distance[idx] = best.distance;
	if (out.leaf)
		out.leaf[idx] = hit ? best.leaf : NONE;
	instance_store_record(out, idx, shade, inverses, best.leaf, best_instance, hit, kept ? 1.0f - best.s - best.t : 0.0f, kept ? best.s : 0.0f,
	                      kept ? best.t : 0.0f, kept ? best.px : 0.0f, kept ? best.py : 0.0f, kept ? best.pz : 0.0f);
}

// (instance_kernel keeps the walk's lines inline: through instance_walk the compiler schedules both instantiations
// differently, and they measured 2 to 5 % slower on the MI355X -- DESIGN.md section 24.  What the walk does is
// instance_walk's comment, word for word, with instance_tri_eval at the leaf; the object ray's six lines are
// instance_object_ray's.)
template <bool CLOSEST>
__global__ __launch_bounds__(64 * QUERY_WAVES) void instance_kernel(InstanceArgs a) {
	bool live;
	uint32_t idx;
	const Ray ray = packet_ray(a, blockIdx.x * (64u * QUERY_WAVES) + threadIdx.x, live, idx);
	const float max_distance = a.max_distance;
	bool alive = live, hit = false;
	Hit best = closest_entry();
	uint32_t best_instance = 0u;
	exact_walk(a.set.top_ptr, a.set.top_count, ray, max_distance, alive, [&](uint32_t k, bool entered) {
		float4 m0, m1, m2;
		scalar_load_rows(a.set.inverses, k, m0, m1, m2);
		const float ox = ((m0.x * ray.ox + m0.y * ray.oy) + m0.z * ray.oz) + m0.w;
		const float oy = ((m1.x * ray.ox + m1.y * ray.oy) + m1.z * ray.oz) + m1.w;
		const float oz = ((m2.x * ray.ox + m2.y * ray.oy) + m2.z * ray.oz) + m2.w;
		const float dx = (m0.x * ray.dx + m0.y * ray.dy) + m0.z * ray.dz;
		const float dy = (m1.x * ray.dx + m1.y * ray.dy) + m1.z * ray.dz;
		const float dz = (m2.x * ray.dx + m2.y * ray.dy) + m2.z * ray.dz;
		const Ray object = make_ray(entered ? ox : 0.0f, entered ? oy : 0.0f, entered ? oz : 0.0f, entered ? dx : 1.0f, entered ? dy : 1.0f,
		                            entered ? dz : 1.0f);
		bool inside = entered;
		exact_walk(a.nodes_ptr, a.node_count, object, max_distance, inside, [&](uint32_t leaf, bool box) {
			const float4 *tri = a.tris_ptr + LEAF_F4 * leaf + LEAF_TRI_F4;
			const float4 q0 = tri[0], q1 = tri[1], q2 = tri[2], q3 = tri[3];
			if (box) {
				float r;
				const TriResult tr = instance_tri_eval(q0, q1, q2, q3, object, r);
				if (tr.accepted) {
					hit = true;
					if (CLOSEST) {
						instance_candidate(ray, k, leaf, tr, r, best, best_instance);
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
	if (!live)
		return;
	if (a.hit)
		a.hit[idx] = hit ? 1u : 0u;
	if (CLOSEST)
		instance_record_store(a.out, a.instance, idx, a.shade, a.set.inverses, hit, best, best_instance);
}

}  // namespace ocrt
