// kernels/directional.hip.h -- directional occlusion queries: which of a point's ambient-occlusion rays were blocked, and
// the sum of the open ones' directions (include/rt_hip_directional.h)
// (part of the one translation unit kernels.hip; see its head for the passes and the arithmetic contract)
//
// The rays are those of an ambient-occlusion query (kernels/ao_query.hip.h): ray r = slot * rays_per_point + k is direction
// k of the point in slot `slot`, a wave casts a packet of 64 consecutive rays, and the walk is the exact form.  What a ray
// IS -- its origin, its point's tangent frame, its direction -- has one definition here, ao_point / ao_direction, used by
// the three kernels below: the walk that makes the masks, the resolve that sums directions, and the kernel that writes the
// rays out for the caller.  The walk's packet ray and its tail are functions (ao_mask_ray, ao_mask_flags) that its instanced
// form shares (kernels/instance_directional.hip.h).  (ao_query_kernel keeps a text of its own, ao_query_ray, shared with its
// instanced form alone: it is the frame layers' and views' kernel too.)
//
// Masks: hit flags are integers, and a flag has one place -- bit k & 31 of word k >> 5 of its point's row -- so the order
// in which the packets of a point arrive is free.  Per packet the flags are balloted; the first lane of every run of lanes
// that shares a (point, mask word) ORs the run's bits into that word: at most one vector atomic per (packet, point, word),
// none where nothing was hit.  With 32 rays per point or fewer that is the counting kernel's number of atomics.
//
// Resolve: one thread per point reads the point's own row (no order is involved), writes its popcount and 1 - hits / n, and
// -- where the sums are wanted -- makes the point's directions again, k = 0, 1, ... in that order, and adds the open ones:
// a sequential float sum, the same words whatever the launch looked like.
#pragma once
#include "ao_query.hip.h"

namespace ocrt {

// A point as its rays see it: the origin, the tangent frame (basis_y is the normal -- normalised once more in RANDOM mode,
// reference :155) and the normal as given (RANDOM casts it as ray 0, :263).
struct AoPoint {
	float ox, oy, oz;
	float bxx, bxy, bxz, nx, ny, nz, bzx, bzy, bzz;
	float qx, qy, qz;
};

template <int MODE>
__device__ __forceinline__ AoPoint ao_point(const float4 p, const float4 q) {
	AoPoint f;
	f.qx = q.x; f.qy = q.y; f.qz = q.z;
	f.nx = q.x; f.ny = q.y; f.nz = q.z;
	// p = point + normal * (1.0f / 100000.0f), reference :215
	const float eps = 1.0f / 100000.0f;
	f.ox = p.x + f.nx * eps;
	f.oy = p.y + f.ny * eps;
	f.oz = p.z + f.nz * eps;
	if (MODE == AO_RANDOM)
		normalize3(f.nx, f.ny, f.nz);  // hemisphere_sampler normalises once more, reference :155
	tangent_frame(f.nx, f.ny, f.nz, f.bxx, f.bxy, f.bxz, f.bzx, f.bzy, f.bzz);
	return f;
}

// The point's generator in front of sample k >= 1 (draws 2k-2 and 2k-1): where random_sample (kernels/ao.hip.h) stands
// when it has skipped to sample k.
__device__ __forceinline__ Rng ao_rng_at(uint32_t seed_index, uint32_t k) {
	Rng rng = rng_seed(536870923u * seed_index);
	for (uint32_t skip = 1; skip < k; ++skip) {
		rng_next(rng);
		rng_next(rng);
	}
	return rng;
}

// Direction k of the point, as cast.  UNIFORM: table direction k in the point's frame, not normalised.  RANDOM: ray 0 is
// the normal as given; ray k >= 1 takes the generator's next two draws -- `rng` must stand in front of sample k (ao_rng_at,
// or the call for k - 1) and is left in front of sample k + 1 -- with random_sample's arithmetic, and is normalised.
template <int MODE>
__device__ __forceinline__ void ao_direction(const AoPoint &f, const float4 *table, Rng &rng, uint32_t k, float &rx, float &ry, float &rz) {
	float xs, ys, zs;
	if (MODE == AO_UNIFORM) {
		const float4 dir = table[k];
		xs = dir.x; ys = dir.y; zs = dir.z;
	} else {
		if (k == 0u) {  // the un-normalised normal itself (:263); no draw is taken
			rx = f.qx; ry = f.qy; rz = f.qz;
			return;
		}
		const float xi1 = rng_float(rng);
		const float xi2 = rng_float(rng);
		const float theta = OCRT_ACOS(sqrtf(1.0f - xi1));
		const float phi = (float) (2.0 * (double) xi2);
		xs = OCRT_SIN(theta) * OCRT_COSPI(phi);
		ys = OCRT_COS(theta);
		zs = OCRT_SIN(theta) * OCRT_SINPI(phi);
	}
	// ray_dir = basis_x * xs + basis_y * ys + basis_z * zs
	rx = (f.bxx * xs + f.nx * ys) + f.bzx * zs;
	ry = (f.bxy * xs + f.ny * ys) + f.bzy * zs;
	rz = (f.bxz * xs + f.nz * ys) + f.bzz * zs;
	if (MODE == AO_RANDOM)
		normalize3(rx, ry, rz);
}

struct AoMaskArgs {
	const float4 *nodes_ptr;  // SceneBuffers::nodes: exact boxes, builder order (NodeRec)
	const float4 *tris_ptr;   // TriRec by leaf
	const float4 *ao_table;   // float4[rays] (UNIFORM)
	const float4 *points, *normals;  // float4[n]
	const uint32_t *seeds;    // [n] the reference's `index` of a point (RANDOM), or null: the point's own index
	const uint32_t *order;    // [n] point of slot j, or null: point j
	uint32_t *mask;           // [n][words] hit flags by point index, zeroed before the launch
	uint32_t n, rays;         // points, rays per point
	uint32_t words;           // ceil(rays / 32)
	uint32_t total;           // n * rays
	uint32_t node_count;
	float max_distance;
};

// The tail of the mask kernels (ao_mask_kernel, instance_ao_mask_kernel): the packet's flags by (point, mask word) -- the
// first lane of a run of lanes that shares both ORs the run's bits in.  The whole wave calls it (the ballot).
__device__ __forceinline__ void ao_mask_flags(const AoMaskArgs &a, bool live, uint32_t idx, uint32_t k, bool hit) {
	const unsigned long long hits = wave_ballot(hit);
	if (!live)
		return;
	const uint32_t lane = threadIdx.x & 63u, bit = k & 31u;
	if (!(lane == 0u || k == 0u || bit == 0u))
		return;
	// the run ends with the word, with the point or with the packet: 1 .. 32 lanes
	uint32_t len = 32u - bit;
	len = a.rays - k < len ? a.rays - k : len;
	len = 64u - lane < len ? 64u - lane : len;
	const uint32_t flags = (uint32_t) ((hits >> lane) & ((1ull << len) - 1ull)) << bit;
	if (flags)
		atomicOr(&a.mask[idx * a.words + (k >> 5)], flags);
}

// The packet's ray of the mask kernels: ray r of the flattened (slot, direction) list, made in registers; a dead lane (a
// partial last packet) gets a ray that walks nothing.  The whole wave calls it (make_ray ballots).  (Locals of its own,
// handed out at the end: written straight into the references the compiler allots ao_mask_kernel's registers in another
// order -- the same instructions under other names, and that kernel's assembly is not to move.)
template <int MODE>
__device__ __forceinline__ Ray ao_mask_ray(const AoMaskArgs &a, uint32_t r, bool &live, uint32_t &idx, uint32_t &k) {
	const bool in_range = r < a.total;
	uint32_t point = 0u, dir = 0u;
	float ox = 0.0f, oy = 0.0f, oz = 0.0f, rx = 1.0f, ry = 1.0f, rz = 1.0f;
	if (in_range) {
		const uint32_t slot = r / a.rays;
		dir = r - slot * a.rays;
		point = a.order ? a.order[slot] : slot;
		const AoPoint f = ao_point<MODE>(a.points[point], a.normals[point]);
		ox = f.ox; oy = f.oy; oz = f.oz;
		Rng rng{};
		if (MODE == AO_RANDOM)
			rng = ao_rng_at(a.seeds ? a.seeds[point] : point, dir);
		ao_direction<MODE>(f, a.ao_table, rng, dir, rx, ry, rz);
	}
	const Ray ray = make_ray(ox, oy, oz, rx, ry, rz);
	live = in_range;
	idx = point;
	k = dir;
	return ray;
}

// The packet shape, the rays and the walk of ao_query_kernel<MODE>; the tail keeps the hit flags apart.
template <int MODE>
__global__ __launch_bounds__(64 * QUERY_WAVES) void ao_mask_kernel(AoMaskArgs a) {
	const uint32_t r = blockIdx.x * (64u * QUERY_WAVES) + threadIdx.x;
	bool live;  // (a partial last packet: its dead lanes walk nothing and flag nothing)
	uint32_t idx, k;
	const Ray ray = ao_mask_ray<MODE>(a, r, live, idx, k);
	bool alive = live, hit = false;
	// a lane leaves at its first accepted triangle
	exact_walk(a.nodes_ptr, a.node_count, ray, a.max_distance, alive, [&](uint32_t leaf, bool box) {
		const float4 *tri = a.tris_ptr + LEAF_F4 * leaf + LEAF_TRI_F4;
		const float4 q0 = tri[0], q1 = tri[1], q2 = tri[2], q3 = tri[3];
		if (box) {
			const TriResult tr = tri_eval<false>(q0, q1, q2, q3, ray);
			if (tr.accepted) {
				hit = true;
				alive = false;
			}
		}
		return wave_ballot(alive) == 0ull;
	});
	ao_mask_flags(a, live, idx, k, hit);
}

struct AoResolveArgs {
	const uint32_t *mask;     // [n][words]
	const float4 *ao_table;   // float4[rays] (UNIFORM)
	const float4 *points, *normals;  // float4[n]
	const uint32_t *seeds;    // [n] or null: the point's own index
	uint32_t *occluded;       // [n] or null
	float *ao;                // [n] or null
	float *bent;              // [3 n] or null
	uint32_t n, rays, words;
	uint32_t ao_divisor;
};

// One thread per point: the popcount of its row, ao_query_finish_kernel's value, and the ordered sum of its open rays.
template <int MODE>
__global__ __launch_bounds__(256) void ao_directional_finish_kernel(AoResolveArgs a) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= a.n)
		return;
	const uint32_t *const row = a.mask + (size_t) i * a.words;
	if (a.occluded || a.ao) {
		uint32_t count = 0u;
		for (uint32_t w = 0; w < a.words; ++w)
			count += (uint32_t) __popc(row[w]);
		if (a.occluded)
			a.occluded[i] = count;
		if (a.ao) {
			const float divisor = (float) a.ao_divisor;
			a.ao[i] = 1.0f - ((float) count / divisor);
		}
	}
	if (!a.bent)
		return;
	const AoPoint f = ao_point<MODE>(a.points[i], a.normals[i]);
	Rng rng{};
	if (MODE == AO_RANDOM)
		rng = ao_rng_at(a.seeds ? a.seeds[i] : i, 1u);  // (stepped by ao_direction from here on)
	float bx = 0.0f, by = 0.0f, bz = 0.0f;
	uint32_t word = 0u;
	for (uint32_t k = 0; k < a.rays; ++k) {
		if ((k & 31u) == 0u)
			word = row[k >> 5];
		float rx, ry, rz;
		ao_direction<MODE>(f, a.ao_table, rng, k, rx, ry, rz);
		if (!((word >> (k & 31u)) & 1u)) {
			bx = bx + rx;
			by = by + ry;
			bz = bz + rz;
		}
	}
	a.bent[3 * (size_t) i + 0] = bx;
	a.bent[3 * (size_t) i + 1] = by;
	a.bent[3 * (size_t) i + 2] = bz;
}

struct AoRaysArgs {
	const float4 *ao_table;
	const float4 *points, *normals;
	const uint32_t *seeds;
	float4 *origins;     // [n] or null
	float4 *directions;  // [n * rays] or null
	uint32_t rays, total;
};

// One thread per ray: its direction, and -- the point's first ray -- the origin.
template <int MODE>
__global__ __launch_bounds__(256) void ao_rays_kernel(AoRaysArgs a) {
	const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= a.total)
		return;
	const uint32_t idx = r / a.rays, k = r - idx * a.rays;
	const AoPoint f = ao_point<MODE>(a.points[idx], a.normals[idx]);
	if (a.origins && k == 0u)
		a.origins[idx] = make_float4(f.ox, f.oy, f.oz, 0.0f);
	if (!a.directions)
		return;
	Rng rng{};
	if (MODE == AO_RANDOM)
		rng = ao_rng_at(a.seeds ? a.seeds[idx] : idx, k);
	float rx, ry, rz;
	ao_direction<MODE>(f, a.ao_table, rng, k, rx, ry, rz);
	a.directions[r] = make_float4(rx, ry, rz, 0.0f);
}

}  // namespace ocrt
