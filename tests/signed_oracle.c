/*
 * signed_oracle.c -- CPU oracle of the signed distance queries (include/rt_hip_signed.h).  TEST INFRASTRUCTURE ONLY.
 *
 * The contract by brute force: the sign table from the leaf-ordered faces by plain loops in leaf order (no sort of corners:
 * a vertex's sum is an accumulator indexed by the vertex, an edge's members are found by a sort of (key, 3 leaf + edge)
 * pairs with qsort), every point against every leaf, no tree.  The arithmetic is the one file the kernels compile
 * (csrc/signed_point.h over csrc/nearest_point.h); the leaf's values are nearest_oracle.c's no_leaf.
 * Built by tests/signed_oracle.py with -O2 -ffp-contract=off -fno-fast-math.
 */
#include <stdlib.h>

#include "nearest_oracle.c"

#include "../opencl_raytracer_amd/csrc/signed_point.h"

typedef struct so_pair {
	uint64_t key;
	uint32_t value;
} so_pair;

static int so_compare(const void *a, const void *b) {
	const so_pair *x = (const so_pair *) a, *y = (const so_pair *) b;
	if (x->key != y->key)
		return x->key < y->key ? -1 : 1;
	return x->value < y->value ? -1 : x->value > y->value ? 1 : 0;
}

/* The sign table: SP_REC_FLOATS floats per leaf.  `vertices`: how many there are.  Returns 0, or -1 without memory. */
int so_table(const uint32_t *faces, uint32_t leaves, const float *v4, uint32_t vertices, float *table) {
	sp_vec *sum = (sp_vec *) calloc(vertices ? vertices : 1u, sizeof(sp_vec));
	so_pair *edges = (so_pair *) malloc((size_t) (leaves ? leaves : 1u) * 3u * sizeof(so_pair));
	if (!sum || !edges) {
		free(sum);
		free(edges);
		return -1;
	}
	for (uint32_t l = 0; l < leaves; ++l) {
		const sp_leaf leaf = sp_leaf_of(no_leaf(faces, v4, l));
		float *rec = table + (size_t) SP_REC_FLOATS * l;
		for (int c = 0; c < 3; ++c) {
			const uint32_t x = faces[3u * l + (uint32_t) c];
			sum[x] = sp_add_corner(sum[x], leaf, c);
			rec[12 + 4 * c + 3] = leaf.angle[c];
			edges[3u * l + (uint32_t) c].key = sp_edge_key(faces + 3u * l, c);
			edges[3u * l + (uint32_t) c].value = 3u * l + (uint32_t) c;
		}
		rec[3] = leaf.n.x; rec[7] = leaf.n.y; rec[11] = leaf.n.z;
	}
	for (uint32_t l = 0; l < leaves; ++l)
		for (int c = 0; c < 3; ++c) {
			const sp_vec s = sum[faces[3u * l + (uint32_t) c]];
			float *at = table + (size_t) SP_REC_FLOATS * l + 12 + 4 * c;
			at[0] = s.x; at[1] = s.y; at[2] = s.z;
		}
	qsort(edges, (size_t) leaves * 3u, sizeof(so_pair), so_compare);
	for (size_t first = 0, n = (size_t) leaves * 3u; first < n;) {
		size_t end = first;
		sp_vec s = sp_make(0.0f, 0.0f, 0.0f);
		for (; end < n && edges[end].key == edges[first].key; ++end)
			s = sp_add_normal(s, sp_leaf_of(no_leaf(faces, v4, edges[end].value / 3u)));
		for (size_t k = first; k < end; ++k) {
			float *at = table + (size_t) SP_REC_FLOATS * (edges[k].value / 3u) + 4u * (edges[k].value % 3u);
			at[0] = s.x; at[1] = s.y; at[2] = s.z;
		}
		first = end;
	}
	free(sum);
	free(edges);
	return 0;
}

float so_angle(const float *a, const float *b) { return sp_angle(sp_make(a[0], a[1], a[2]), sp_make(b[0], b[1], b[2])); }

/* Points [0, n) against leaves [0, leaves); `table`: so_table's.  Any output may be NULL.  The record is
 * no_closest_points', the distance signed; feature: NP_* (0xFF: not found); pseudonormal4: N and g (zeros: not found). */
void so_signed_distance(const uint32_t *faces, uint32_t leaves, const float *v4, const float *n4, const float *table, const float *q4,
                        uint32_t n, float max_distance, uint8_t *found, float *distance, uint32_t *leaf, float *bary, float *pos,
                        float *normal, uint8_t *feature, float *pseudonormal4) {
	no_closest_points(faces, leaves, v4, n4, q4, n, max_distance, found, NULL, leaf, bary, pos, normal);
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 64) num_threads(no_threads())
#endif
	for (int64_t i = 0; i < (int64_t) n; ++i) {
		const float qx = q4[4 * i], qy = q4[4 * i + 1], qz = q4[4 * i + 2];
		float best_d2 = INFINITY;
		uint32_t best_leaf = NO_NONE;
		np_point best;
		memset(&best, 0, sizeof best);
		if (np_radius_ok(max_distance) && np_point_ok(qx, qy, qz))
			for (uint32_t l = 0; l < leaves; ++l) {
				const np_point r = np_nearest(no_leaf(faces, v4, l), qx, qy, qz);
				if (np_better(r.d2, l, best_d2, best_leaf)) {
					best_d2 = r.d2;
					best_leaf = l;
					best = r;
				}
			}
		const float d = sqrtf(best_d2);
		const int ok = best_d2 < INFINITY && d <= max_distance;
		sp_vec N = sp_make(0.0f, 0.0f, 0.0f);
		float g = 0.0f;
		if (ok) {
			N = sp_pseudonormal(table + (size_t) SP_REC_FLOATS * best_leaf, best.region);
			g = sp_side(qx, qy, qz, best.px, best.py, best.pz, N);
		}
		if (distance)
			distance[i] = ok ? (g < 0.0f ? -d : d) : INFINITY;
		if (feature)
			feature[i] = ok ? (uint8_t) best.region : 0xFFu;
		if (pseudonormal4) {
			pseudonormal4[4 * i] = N.x; pseudonormal4[4 * i + 1] = N.y; pseudonormal4[4 * i + 2] = N.z; pseudonormal4[4 * i + 3] = g;
		}
	}
}
