// kernels/instance_views.hip.h -- the instance set seen and shaded: ambient occlusion at world-space points against the
// posed copies, and the frame's own rays of many views against them (include/rt_hip_instance_views.h)
// (part of the one translation unit kernels.hip; see its head for the passes and the arithmetic contract)
//
// instance_walk<CLOSEST> is instance_kernel's two nested exact walks (kernels/instances.hip.h has the rules: the outer walk
// over the top-level records with the world ray, O_k by scalar loads, the object ray in the header's operation order,
// make_ray by the whole wave, the inner walk over the scene's records with `alive && entered`) as one function for the two
// kernels below.  instance_kernel keeps its own lines: its device code is not to move.
//
// instance_ao_kernel<MODE>: ao_query_kernel's packet -- 64 consecutive rays of the flattened (slot, direction) list, each
// made in registers with that kernel's arithmetic --, the nested walk in its occlusion form, and ao_query_kernel's tail:
// ballot, one vector atomic per (packet, point), none where nothing was hit.  `order` and `seeds` are that kernel's, so the
// views path hands it the list of a chunk's hit sub-pixels unchanged.
//
// instance_layers_kernel: layers_kernel<true, true>'s tiling and ray -- one wave per 8 x 8 tile, blockIdx.y the view, the
// pose by scalar loads from the chunk's poses, camera_ray<true> --, the nested walk in its closest form with
// instance_nearer, and an epilogue that writes the instanced record as instance_kernel writes it (the normal: the raw
// weighted sum, transpose(O), ONE normalisation), the direction, the head-light term on that normal, and -- views always
// list -- the flag, seed, point and normal entries of the ambient-occlusion step with the missed sub-pixels' ao = 1 and
// value = 0.  What follows it (kernels/views.hip.h) runs as it is.
#pragma once
#include "ao_query.hip.h"
#include "instances.hip.h"
#include "layers.hip.h"

namespace ocrt {

// Returns whether the lane has a candidate.  CLOSEST: every candidate goes to candidate(k, leaf, tr, r) -- instance, leaf,
// the object-space test's result and its plane parameter --, nobody leaves; else a lane leaves both walks at its first
// candidate, and both end once the packet has no lane left.
template <bool CLOSEST, class Candidate>
__device__ __forceinline__ bool instance_walk(const float4 *top_ptr, uint32_t top_count, const float4 *inverses, const float4 *nodes_ptr,
                                              uint32_t node_count, const float4 *tris_ptr, const Ray &ray, float max_distance, bool live,
                                              Candidate &&candidate) {
	bool alive = live, hit = false;
	exact_walk(top_ptr, top_count, ray, max_distance, alive, [&](uint32_t k, bool entered) {
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
		exact_walk(nodes_ptr, node_count, object, max_distance, inside, [&](uint32_t leaf, bool box) {
			const float4 *tri = tris_ptr + LEAF_F4 * leaf + LEAF_TRI_F4;
			const float4 q0 = tri[0], q1 = tri[1], q2 = tri[2], q3 = tri[3];
			if (box) {
				float r;
				const TriResult tr = instance_tri_eval(q0, q1, q2, q3, object, r);
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

struct InstanceAoArgs : AoQueryArgs {  // (nodes_ptr, tris_ptr, node_count: the scene's own; max_distance: in both spaces)
	const float4 *top_ptr;   // the top-level tree: NodeRec[top_count], `leaf` the instance index
	const float4 *inverses;  // object_from_world, three float4 rows per instance
	uint32_t top_count;      // 2 * instances - 1
};

// MODE is AO_UNIFORM or AO_RANDOM, as for ao_query_kernel, whose lines the ray and the tail are.
template <int MODE>
__global__ __launch_bounds__(64 * QUERY_WAVES) void instance_ao_kernel(InstanceAoArgs a) {
	const uint32_t r = blockIdx.x * (64u * QUERY_WAVES) + threadIdx.x;
	const bool live = r < a.total;  // (a partial last packet: its dead lanes walk nothing and count nothing)
	uint32_t slot = 0u, idx = 0u;
	float ox = 0.0f, oy = 0.0f, oz = 0.0f, rx = 1.0f, ry = 1.0f, rz = 1.0f;
	if (live) {
		slot = r / a.rays;
		const uint32_t k = r - slot * a.rays;
		idx = a.order ? a.order[slot] : slot;
		const float4 p = a.points[idx], q = a.normals[idx];
		float nx = q.x, ny = q.y, nz = q.z;
		// p = point + normal * (1.0f / 100000.0f), reference :215
		const float eps = 1.0f / 100000.0f;
		ox = p.x + nx * eps;
		oy = p.y + ny * eps;
		oz = p.z + nz * eps;
		if (MODE == AO_RANDOM)
			normalize3(nx, ny, nz);  // hemisphere_sampler normalises once more, reference :155
		float bxx, bxy, bxz, bzx, bzy, bzz;
		tangent_frame(nx, ny, nz, bxx, bxy, bxz, bzx, bzy, bzz);
		float xs, ys, zs;
		if (MODE == AO_UNIFORM) {
			const float4 dir = a.ao_table[k];
			xs = dir.x; ys = dir.y; zs = dir.z;
		} else {
			// RANDOM: ray 0 goes along the normal (below), ray k >= 1 is sample k of the point's generator
			random_sample(a.seeds ? a.seeds[idx] : idx, k, xs, ys, zs);
		}
		// ray_dir = basis_x * xs + basis_y * ys + basis_z * zs
		rx = (bxx * xs + nx * ys) + bzx * zs;
		ry = (bxy * xs + ny * ys) + bzy * zs;
		rz = (bxz * xs + nz * ys) + bzz * zs;
		if (MODE == AO_RANDOM) {
			normalize3(rx, ry, rz);
			if (k == 0u) {  // the un-normalised normal itself (:263)
				rx = q.x; ry = q.y; rz = q.z;
			}
		}
	}
	const Ray ray = make_ray(ox, oy, oz, rx, ry, rz);
	const bool hit = instance_walk<false>(a.top_ptr, a.top_count, a.inverses, a.nodes_ptr, a.node_count, a.tris_ptr, ray, a.max_distance, live,
	                                      [](uint32_t, uint32_t, const TriResult &, float) {});
	// the packet's hits by point: the first lane of a point's run adds the run's share of the ballot
	const unsigned long long hits = wave_ballot(hit);
	if (!live)
		return;
	const uint32_t lane = threadIdx.x & 63u, packet = r - lane;  // (the packet's first ray)
	const uint32_t run = slot * a.rays;                          // (the point's first ray)
	const uint32_t first = run > packet ? run - packet : 0u;
	if (lane != first)
		return;
	const uint32_t end = run + a.rays - packet;  // (> first: ray r is the point's; may lie beyond the packet)
	const unsigned long long below_end = end >= 64u ? ~0ull : (1ull << end) - 1ull;
	const uint32_t occluded = (uint32_t) __popcll(hits & below_end & ~((1ull << first) - 1ull));
	if (occluded)
		atomicAdd(&a.count[idx], occluded);
}

struct InstanceLayersArgs : LayersArgs {  // (ARRAY and listing: `poses` is read; flags, seeds, points, normals where the step follows)
	const float4 *top_ptr;   // the top-level tree
	const float4 *inverses;  // object_from_world, three float4 rows per instance
	uint32_t top_count;
	uint32_t *instance;      // by sub-pixel index, the first view's block, or null
};

__global__ __launch_bounds__(64 * LAYERS_WAVES) void instance_layers_kernel(InstanceLayersArgs a) {
	// (wave-uniform by construction; read through the first lane so that the compiler keeps the tile in SGPRs, as the view is)
	const uint32_t tile = (uint32_t) __builtin_amdgcn_readfirstlane((int) (blockIdx.x * LAYERS_WAVES + (threadIdx.x >> 6)));
	const uint32_t view = blockIdx.y, lane = threadIdx.x & 63u;
	if (tile >= a.tiles)  // (the spare waves of a view's last workgroup)
		return;
	a.pose = a.poses[view];
	const uint32_t tile_y = tile / a.tiles_x, tile_x = tile - tile_y * a.tiles_x;
	const uint32_t x = tile_x * TILE_W + (lane & 7u), y = tile_y * TILE_H + (lane >> 3);
	// (a partial tile on the right or bottom edge: its lanes outside the image walk nothing and write nothing)
	const bool live = x < a.width && y < a.height;
	const Ray ray = camera_ray<true>(a, x, y);
	Hit best = closest_entry();
	uint32_t best_instance = 0u;
	const bool hit = instance_walk<true>(a.top_ptr, a.top_count, a.inverses, a.nodes_ptr, a.node_count, a.tris_ptr, ray, LAYERS_MAX_DISTANCE, live,
	                                     [&](uint32_t k, uint32_t leaf, const TriResult &tr, float r) {
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
	                                     });
	if (!live)
		return;
	const uint32_t seed = y * a.width + x;          // the sub-pixel's index within its view
	const size_t idx = (size_t) view * a.n + seed;  // ... and within the launch: view v's block of every layer
	// the record, as instance_kernel<true> writes it
	if (a.hit)
		a.hit[idx] = hit ? 1u : 0u;
	const bool kept = hit && best.distance < __builtin_inff();  // (the record was replaced at least once)
	if (a.instance)
		a.instance[idx] = hit ? best_instance : NONE;
	if (a.out.distance)
		a.out.distance[idx] = best.distance;
	if (a.out.leaf)
		a.out.leaf[idx] = hit ? best.leaf : NONE;
	const float b0 = kept ? 1.0f - best.s - best.t : 0.0f, b1 = kept ? best.s : 0.0f, b2 = kept ? best.t : 0.0f;
	const float px = kept ? best.px : 0.0f, py = kept ? best.py : 0.0f, pz = kept ? best.pz : 0.0f;
	if (a.out.barycentric) {
		a.out.barycentric[3u * idx + 0u] = b0;
		a.out.barycentric[3u * idx + 1u] = b1;
		a.out.barycentric[3u * idx + 2u] = b2;
	}
	if (a.out.position) {
		a.out.position[3u * idx + 0u] = px;
		a.out.position[3u * idx + 1u] = py;
		a.out.position[3u * idx + 2u] = pz;
	}
	if (a.direction) {
		a.direction[3u * idx + 0u] = ray.dx;
		a.direction[3u * idx + 1u] = ray.dy;
		a.direction[3u * idx + 2u] = ray.dz;
	}
	if (!a.out.normal && !a.shade && !a.value && !a.points)
		return;
	// get_smooth_normal's weighted sum in the object's frame, the inverse's transpose, ONE normalisation; the head-light
	// term (reference :296-304) on those words
	float value = 0.0f;
	float wx = 0.0f, wy = 0.0f, wz = 0.0f;
	if (hit) {
		const float4 n0 = a.shade_recs[3 * (size_t) best.leaf + 0], n1 = a.shade_recs[3 * (size_t) best.leaf + 1],
		             n2 = a.shade_recs[3 * (size_t) best.leaf + 2];
		const float rx = (n0.x * b0 + n1.x * b1) + n2.x * b2;
		const float ry = (n0.y * b0 + n1.y * b1) + n2.y * b2;
		const float rz = (n0.z * b0 + n1.z * b1) + n2.z * b2;
		const float4 *rows = a.inverses + 3u * (size_t) best_instance;
		const float4 m0 = rows[0], m1 = rows[1], m2 = rows[2];
		wx = (m0.x * rx + m1.x * ry) + m2.x * rz;
		wy = (m0.y * rx + m1.y * ry) + m2.y * rz;
		wz = (m0.z * rx + m1.z * ry) + m2.z * rz;
		normalize3(wx, wy, wz);
		value = 1.0f;
		if (a.shading)
			value = fminf(fmaxf(-dot3(wx, wy, wz, ray.dx, ray.dy, ray.dz), 0.0f), 1.0f);
	}
	if (a.out.normal) {
		a.out.normal[3u * idx + 0u] = wx;
		a.out.normal[3u * idx + 1u] = wy;
		a.out.normal[3u * idx + 2u] = wz;
	}
	if (a.shade)
		a.shade[idx] = value;
	if (a.value)
		a.value[idx] = value;
	if (!a.points)
		return;
	// the ambient-occlusion step follows: a missed sub-pixel is final, a hit one goes onto the list
	if (!hit) {
		if (a.ao)
			a.ao[idx] = 1.0f;
		if (a.product)
			a.product[idx] = 0.0f;
	}
	a.flags[idx] = hit ? 1u : 0u;
	if (hit) {
		a.seeds[idx] = seed;
		a.points[idx] = make_float4(px, py, pz, 1.0f);
		a.normals[idx] = make_float4(wx, wy, wz, value);
	}
}

}  // namespace ocrt
