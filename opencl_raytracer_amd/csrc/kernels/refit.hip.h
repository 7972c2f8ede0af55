// kernels/refit.hip.h -- vertex updates (include/rt_hip_update.h): the leaf records and every box of an uploaded scene made
// again from new vertex positions, on the device.  The rule is refit.h's; the arithmetic of a leaf record is pack_scene's
// (scene_pack.cc), operation for operation -- this file is compiled without contraction like the host's --, so the records
// carry the bits a fresh upload of the same positions would.
//
//   refit_leaves_kernel   a lane per leaf: three vertices through the leaf's face, the TriRec, the ShadeRec where normals
//                         were given, the leaf's box into its NodeRec (lo and hi alone: `skip` and `leaf` are never written).
//   refit_inner_kernel    a workgroup per GROUP of the host-made schedule (refit.h, RefitSchedule), one launch per pass:
//                         rounds by height inside the group, a barrier between rounds, the group's own boxes in LDS.  What
//                         a group reads beside them -- leaves, nodes of earlier passes -- an EARLIER LAUNCH wrote: no
//                         workgroup ever waits for another, nothing crosses between workgroups inside a launch.
#pragma once

namespace ocrt {

constexpr uint32_t REFIT_LEAF_LANES = 256u;   // refit_leaves_kernel: four waves, each transposes its own 64 records
constexpr uint32_t REFIT_INNER_LANES = 256u;
constexpr uint32_t REFIT_GROUP_MAX = 1024u;   // refit.h, REFIT_MAX_GROUP: the boxes of a group in LDS (24 KB)
constexpr uint32_t REFIT_LOCAL_REF = 0x80000000u;  // refit.h, REFIT_LOCAL

struct RefitLeafArgs {
	const uint32_t *faces;      // three vertex ids per leaf, in leaf order
	const uint32_t *leaf_node;  // the node of every leaf
	const float4 *vertices;     // the new positions
	const float4 *vnormals;     // the new normals, or null: the ShadeRecs stay
	float4 *tris;               // TriRec[leaves]
	float4 *shade;              // ShadeRec[leaves]
	float *nodes;               // NodeRec[nodes], as floats: lo at 8 * i, hi at 8 * i + 4
	uint32_t leaves;
};

// std::min(a, std::min(b, c)) and std::max(a, std::max(b, c)) as the builder evaluates them (bvh.cc, Prims): comparisons
// and selects, which keep the zero the builder keeps -- not v_min_f32 / v_max_f32.
__device__ __forceinline__ float refit_min3(float a, float b, float c) {
	const float m = c < b ? c : b;
	return m < a ? m : a;
}
__device__ __forceinline__ float refit_max3(float a, float b, float c) {
	const float m = b < c ? c : b;
	return a < m ? m : a;
}

// The 96-byte and 48-byte records leave the wave as whole float4s, lane i of store j writing float4 j * 64 + i of the wave's
// 64 records: consecutive lanes, consecutive 16 bytes (a lane that stored its own record would write 16 bytes every 96).
// The records pass through the wave's slice of LDS for that, six float4 per lane.
__global__ __launch_bounds__(REFIT_LEAF_LANES) void refit_leaves_kernel(const RefitLeafArgs a) {
	__shared__ float4 staged[REFIT_LEAF_LANES / 64u][64u * 6u];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const uint32_t first = blockIdx.x * REFIT_LEAF_LANES + wave * 64u;  // the wave's first leaf
	const uint32_t leaf = first + lane;
	const bool live = leaf < a.leaves;  // (no lane leaves early: the barriers below are the workgroup's)
	float4 *const mine = &staged[wave][lane * 6u];
	uint32_t i0 = 0, i1 = 0, i2 = 0;
	if (live) {
		i0 = a.faces[3u * leaf];
		i1 = a.faces[3u * leaf + 1u];
		i2 = a.faces[3u * leaf + 2u];
		const float4 va = a.vertices[i0], vb = a.vertices[i1], vc = a.vertices[i2];
		const float ux = vb.x - va.x, uy = vb.y - va.y, uz = vb.z - va.z;
		const float vx = vc.x - va.x, vy = vc.y - va.y, vz = vc.z - va.z;
		float nx, ny, nz;
		cross3(ux, uy, uz, vx, vy, vz, nx, ny, nz);
		const float uu = dot3(ux, uy, uz, ux, uy, uz);
		const float uv = dot3(ux, uy, uz, vx, vy, vz);
		const float vv = dot3(vx, vy, vz, vx, vy, vz);
		const float D = uv * uv - uu * vv;
		const float lox = refit_min3(va.x, vb.x, vc.x), loy = refit_min3(va.y, vb.y, vc.y), loz = refit_min3(va.z, vb.z, vc.z);
		const float hix = refit_max3(va.x, vb.x, vc.x), hiy = refit_max3(va.y, vb.y, vc.y), hiz = refit_max3(va.z, vb.z, vc.z);
		mine[0] = make_float4(lox, loy, loz, 0.0f);
		mine[1] = make_float4(hix, hiy, hiz, tri_inverse_d(D));
		mine[2] = make_float4(va.x, va.y, va.z, ux);
		mine[3] = make_float4(uy, uz, vx, vy);
		mine[4] = make_float4(vz, nx, ny, nz);
		mine[5] = make_float4(uu, uv, vv, D);
		float *const node = a.nodes + 8ull * a.leaf_node[leaf];
		node[0] = lox; node[1] = loy; node[2] = loz;
		node[4] = hix; node[5] = hiy; node[6] = hiz;
	}
	const uint32_t records = first >= a.leaves ? 0u : a.leaves - first < 64u ? a.leaves - first : 64u;
	__syncthreads();
	{
		float4 *const out = a.tris + 6ull * first;
#pragma unroll
		for (uint32_t j = 0; j < 6u; ++j)
			if (j * 64u + lane < records * 6u)
				out[j * 64u + lane] = staged[wave][j * 64u + lane];
	}
	if (!a.vnormals)
		return;  // (the whole grid alike)
	__syncthreads();
	if (live) {
		const float4 n0 = a.vnormals[i0], n1 = a.vnormals[i1], n2 = a.vnormals[i2];
		float4 *const three = &staged[wave][lane * 3u];
		three[0] = make_float4(n0.x, n0.y, n0.z, 0.0f);
		three[1] = make_float4(n1.x, n1.y, n1.z, 0.0f);
		three[2] = make_float4(n2.x, n2.y, n2.z, 0.0f);
	}
	__syncthreads();
	float4 *const out = a.shade + 3ull * first;
#pragma unroll
	for (uint32_t j = 0; j < 3u; ++j)
		if (j * 64u + lane < records * 3u)
			out[j * 64u + lane] = staged[wave][j * 64u + lane];
}

struct RefitInnerArgs {
	const uint4 *entries;      // RefitSchedule::entries: node, first child reference, children, round
	const uint32_t *children;  // RefitSchedule::children
	const uint4 *groups;       // RefitSchedule::groups: first entry, entries, rounds, pass
	float *nodes;              // NodeRec[nodes], as floats
	uint32_t first_group;      // the pass's first group; the grid is the pass's groups
};

__global__ __launch_bounds__(REFIT_INNER_LANES) void refit_inner_kernel(const RefitInnerArgs a) {
	__shared__ float box[6][REFIT_GROUP_MAX];
	const uint4 group = a.groups[a.first_group + blockIdx.x];
	const uint32_t entries = group.y < REFIT_GROUP_MAX ? group.y : REFIT_GROUP_MAX;  // (the host never makes a larger one)
	for (uint32_t round = 0; round < group.z; ++round) {
		for (uint32_t e = threadIdx.x; e < entries; e += REFIT_INNER_LANES) {
			const uint4 entry = a.entries[group.x + e];
			if (entry.w != round)
				continue;
			float lo[3] = { 0.0f, 0.0f, 0.0f }, hi[3] = { 0.0f, 0.0f, 0.0f };
			for (uint32_t k = 0; k < entry.z; ++k) {
				const uint32_t ref = a.children[entry.y + k];
				float clo[3], chi[3];
				if (ref & REFIT_LOCAL_REF) {
					const uint32_t slot = (ref & ~REFIT_LOCAL_REF) & (REFIT_GROUP_MAX - 1u);
#pragma unroll
					for (uint32_t c = 0; c < 3u; ++c) {
						clo[c] = box[c][slot];
						chi[c] = box[3u + c][slot];
					}
				} else {
					const float4 l = *(const float4 *) (a.nodes + 8ull * ref), h = *(const float4 *) (a.nodes + 8ull * ref + 4u);
					clo[0] = l.x; clo[1] = l.y; clo[2] = l.z;
					chi[0] = h.x; chi[1] = h.y; chi[2] = h.z;
				}
#pragma unroll
				for (uint32_t c = 0; c < 3u; ++c) {
					// the refit rule: std::min(acc, next), std::max(acc, next) from the first child on
					lo[c] = k == 0u ? clo[c] : (clo[c] < lo[c] ? clo[c] : lo[c]);
					hi[c] = k == 0u ? chi[c] : (hi[c] < chi[c] ? chi[c] : hi[c]);
				}
			}
			float *const node = a.nodes + 8ull * entry.x;
#pragma unroll
			for (uint32_t c = 0; c < 3u; ++c) {
				box[c][e] = lo[c];
				box[3u + c][e] = hi[c];
				node[c] = lo[c];
				node[4u + c] = hi[c];
			}
		}
		__syncthreads();
	}
}

}  // namespace ocrt
