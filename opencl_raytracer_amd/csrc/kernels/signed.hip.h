// kernels/signed.hip.h -- signed distance queries: the sign table, the point form and the grid form
// (include/rt_hip_signed.h; the arithmetic is signed_point.h's over nearest_point.h's, the files the tests' oracle compiles)
// (part of the one translation unit kernels.hip; see its head for the passes and the arithmetic contract)
//
// The table.  Per leaf a SignRec of six float4 (signed_point.h: the pseudonormals of the edges AB, AC, BC and of the vertices
// A, B, C; the face's n^ and the corner angles in the .w): what a point's sign needs of the leaf that won is ONE record.
// It is made from the leaf records and the leaf-ordered faces without a float atomic: the 3 F corners are sorted twice
// (sign_sort.hip: by vertex id, and by the edge's (min, max) vertex pair; stable, so that equal keys stay in rising
// 3 leaf + corner), sign_heads_kernel folds "a new key starts here" into the top bit of the sorted values -- the keys are
// then dropped: 4 bytes per corner and sort are kept --, and sign_sum_kernel gives every segment head one thread that adds
// its members' terms in order and writes the sum to each member's slot.  The terms (n^, angle n^) are recomputed from the
// leaf record per member: nothing else is stored, and an update redoes the sums from the kept incidence alone.
//
// The queries are nearest_walk (kernels/nearest.hip.h) and a tail: the winning leaf's record is gathered, the feature's
// pseudonormal picked by the record's region code, g = dot(q - p, N), and the distance gets g's sign.  The grid form makes
// its points in registers: one wave takes one 4 x 4 x 4 brick of voxels (lane = x + 4 y + 16 z), which is the coherent
// packet the point form's sort tries to make; there is no point array, no order and no sort.
#pragma once
#include "nearest.hip.h"

namespace ocrt {

constexpr uint32_t SIGN_HEAD = 0x80000000u;  // in a kept incidence word: the first member of its segment
constexpr uint32_t SIGN_REC_F4 = SP_REC_FLOATS / 4u;

// ---- the table ---------------------------------------------------------------------------------------------------------
// The sorts' inputs: for corner i = 3 leaf + c the vertex id, the edge key of edge c (AB, AC, BC) and the value i.
__global__ __launch_bounds__(256) void sign_keys_kernel(const uint32_t *faces, uint32_t corners, uint32_t *vertex_keys,
                                                        unsigned long long *edge_keys, uint32_t *values) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= corners)
		return;
	const uint32_t leaf = i / 3u, c = i - 3u * leaf;
	const uint32_t face[3] = { faces[3u * leaf], faces[3u * leaf + 1u], faces[3u * leaf + 2u] };
	vertex_keys[i] = face[c];
	edge_keys[i] = sp_edge_key(face, (int) c);
	values[i] = i;
}

// kept[i] = sorted value i, with SIGN_HEAD where its key differs from the one before it.
template <class Key>
__global__ __launch_bounds__(256) void sign_heads_kernel(const Key *sorted_keys, const uint32_t *sorted_values, uint32_t corners, uint32_t *kept) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= corners)
		return;
	const bool head = i == 0u || sorted_keys[i - 1u] != sorted_keys[i];
	kept[i] = sorted_values[i] | (head ? SIGN_HEAD : 0u);
}

__device__ __forceinline__ sp_leaf sign_leaf(const float4 *tris, uint32_t leaf) {
	const float4 *tri = tris + LEAF_F4 * leaf + LEAF_TRI_F4;
	return sp_leaf_of(nearest_tri(tri[0], tri[1], tri[2], tri[3]));
}

// One thread per entry of a kept incidence list; the heads sum their segment -- EDGES: n^ per member into float4 0 .. 2 of
// the members' records; else angle n^ into float4 3 .. 5 -- in the list's order, which is rising leaf, then corner.
template <bool EDGES>
__global__ __launch_bounds__(256) void sign_sum_kernel(const uint32_t *kept, uint32_t corners, const float4 *tris, uint32_t tri_count, float4 *table) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= corners || !(kept[i] & SIGN_HEAD))
		return;
	sp_vec sum = sp_make(0.0f, 0.0f, 0.0f);
	uint32_t end = i;
	do {
		const uint32_t value = kept[end] & ~SIGN_HEAD, leaf = value / 3u;
		if (leaf < tri_count) {
			const sp_leaf term = sign_leaf(tris, leaf);
			sum = EDGES ? sp_add_normal(sum, term) : sp_add_corner(sum, term, (int) (value - 3u * leaf));
		}
		++end;
	} while (end < corners && !(kept[end] & SIGN_HEAD));
	for (uint32_t k = i; k < end; ++k) {
		const uint32_t value = kept[k] & ~SIGN_HEAD, leaf = value / 3u, c = value - 3u * leaf;
		if (leaf >= tri_count)
			continue;
		// (.w is the per-leaf kernel's: three floats are written)
		float *at = (float *) (table + (size_t) SIGN_REC_F4 * leaf + (EDGES ? c : 3u + c));
		at[0] = sum.x; at[1] = sum.y; at[2] = sum.z;
	}
}

// The .w of a leaf's record: n^ in the edges' three, the corner angles in the vertices'.
__global__ __launch_bounds__(256) void sign_leaf_kernel(const float4 *tris, uint32_t tri_count, float4 *table) {
	const uint32_t leaf = blockIdx.x * blockDim.x + threadIdx.x;
	if (leaf >= tri_count)
		return;
	const sp_leaf l = sign_leaf(tris, leaf);
	float *rec = (float *) (table + (size_t) SIGN_REC_F4 * leaf);
	rec[3] = l.n.x; rec[7] = l.n.y; rec[11] = l.n.z;
	rec[15] = l.angle[0]; rec[19] = l.angle[1]; rec[23] = l.angle[2];
}

// ---- the tail ----------------------------------------------------------------------------------------------------------
struct Signed {
	float distance;  // signed; +inf: not found
	float nx, ny, nz, g;
	bool found;
};

__device__ __forceinline__ Signed signed_tail(const Nearest &best, const float4 *table, uint32_t tri_count, const float4 q, bool alive,
                                              float max_distance) {
	Signed r;
	const float distance = sqrtf(best.d2);
	r.found = alive && best.d2 < __builtin_inff() && distance <= max_distance;
	r.distance = __builtin_inff();
	r.nx = r.ny = r.nz = r.g = 0.0f;
	if (r.found)
		r.distance = distance;
	if (r.found && best.leaf < tri_count) {  // (a leaf index beyond the table -- damaged arrays -- has no sign)
		const float4 *rec = table + (size_t) SIGN_REC_F4 * best.leaf;
		if (best.region == NP_FACE) {
			r.nx = rec[0].w; r.ny = rec[1].w; r.nz = rec[2].w;
		} else {
			const float4 n = rec[sp_slot(best.region)];
			r.nx = n.x; r.ny = n.y; r.nz = n.z;
		}
		r.g = sp_side(q.x, q.y, q.z, best.px, best.py, best.pz, sp_make(r.nx, r.ny, r.nz));
		r.distance = r.g < 0.0f ? -distance : distance;
	}
	return r;
}

// ---- the point form ----------------------------------------------------------------------------------------------------
struct SignedArgs {
	NearestArgs nearest;   // (counts: null; out, hit: the record's arrays)
	const float4 *table;   // SignRec by leaf
	uint8_t *feature;      // [n] NP_*, 0xFF: not found; or null
	float4 *pseudonormal;  // [n] N and g; or null
};

__global__ __launch_bounds__(64 * NEAREST_WAVES) void signed_kernel(SignedArgs s) {
	const NearestArgs &a = s.nearest;
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
	const Nearest best = nearest_walk<false>(a, q, alive, node_tests, tri_tests);
	if (!live)
		return;
	const Signed sign = signed_tail(best, s.table, a.tri_count, q, alive, a.max_distance);
	const bool found = sign.found;
	if (a.hit)
		a.hit[idx] = found ? 1u : 0u;
	if (a.out.distance)
		a.out.distance[idx] = sign.distance;
	if (a.out.leaf)
		a.out.leaf[idx] = found ? best.leaf : NONE;
	if (s.feature)
		s.feature[idx] = found ? (uint8_t) best.region : (uint8_t) 0xFFu;
	if (s.pseudonormal)
		s.pseudonormal[idx] = make_float4(sign.nx, sign.ny, sign.nz, sign.g);
	store_record(a.out, idx, a.shade, best.leaf, found, found ? 1.0f - best.s - best.t : 0.0f, found ? best.s : 0.0f, found ? best.t : 0.0f,
	             found ? best.px : 0.0f, found ? best.py : 0.0f, found ? best.pz : 0.0f);
}

// ---- the grid form -----------------------------------------------------------------------------------------------------
// Voxel (i, j, k) of the call is the point origin + (i, j, k) * spacing, each coordinate origin + float(i) * spacing rounded
// as written.  The launch covers the slab of `nz` slices from slice `z_first` on; bricks count in x, then y, then z.
struct SignedGridArgs {
	NearestArgs nearest;  // (points, order, out, hit: null; n: unused)
	const float4 *table;
	float origin[3], spacing[3];
	uint32_t nx, ny, nz, z_first;
	uint32_t bricks_x, bricks_y, bricks;
	float *distance;  // [nz][ny][nx] of the slab, or null
	uint32_t *leaf;   // the same shape, or null
};

__global__ __launch_bounds__(64 * NEAREST_WAVES) void signed_grid_kernel(SignedGridArgs s) {
	const NearestArgs &a = s.nearest;
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t brick = (uint32_t) __builtin_amdgcn_readfirstlane((int) (blockIdx.x * NEAREST_WAVES + (threadIdx.x >> 6)));
	if (brick >= s.bricks)
		return;  // (a whole wave)
	const uint32_t bz = brick / (s.bricks_x * s.bricks_y), rest = brick - bz * (s.bricks_x * s.bricks_y);
	const uint32_t by = rest / s.bricks_x, bx = rest - by * s.bricks_x;
	const uint32_t i = 4u * bx + (lane & 3u), j = 4u * by + ((lane >> 2) & 3u), k = 4u * bz + (lane >> 4);
	const bool live = i < s.nx && j < s.ny && k < s.nz;
	float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	if (live) {
		q.x = s.origin[0] + (float) i * s.spacing[0];
		q.y = s.origin[1] + (float) j * s.spacing[1];
		q.z = s.origin[2] + (float) (s.z_first + k) * s.spacing[2];
	}
	const bool alive = live && np_point_ok(q.x, q.y, q.z) && np_radius_ok(a.max_distance);
	uint32_t node_tests = 0u, tri_tests = 0u;
	const Nearest best = nearest_walk<false>(a, q, alive, node_tests, tri_tests);
	if (!live)
		return;
	const Signed sign = signed_tail(best, s.table, a.tri_count, q, alive, a.max_distance);
	const size_t voxel = ((size_t) k * s.ny + j) * s.nx + i;
	if (s.distance)
		s.distance[voxel] = sign.distance;
	if (s.leaf)
		s.leaf[voxel] = sign.found ? best.leaf : NONE;
}

}  // namespace ocrt
