/*
 * nearest_oracle.c -- CPU oracle of the closest-point queries (include/rt_hip_nearest.h).  TEST INFRASTRUCTURE ONLY.
 *
 * The contract by brute force: every point against every leaf in leaf order, no tree, no pruning; the per-leaf routine is
 * the one file the kernel compiles (csrc/nearest_point.h).  The leaf's values are made from the leaf-ordered faces and the
 * vertices as the packer makes them (scene_pack.cc): u = tb - ta, v = tc - ta, uu, uv, vv by dot, D = uv uv - uu vv.
 * Built by tests/nearest_oracle.py with -O2 -ffp-contract=off -fno-fast-math.
 */
#include <stdint.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#include "../opencl_raytracer_amd/csrc/nearest_point.h"

#define NO_NONE 0xFFFFFFFFu
#define NO_MAX_THREADS 16

static int no_threads(void) {
#ifdef _OPENMP
	const int n = omp_get_max_threads();
	return n < NO_MAX_THREADS ? n : NO_MAX_THREADS;
#else
	return 1;
#endif
}

/* The values the device holds of leaf `leaf`. */
np_tri no_leaf(const uint32_t *faces, const float *v4, uint32_t leaf) {
	const float *a = v4 + 4u * faces[3u * leaf], *b = v4 + 4u * faces[3u * leaf + 1u], *c = v4 + 4u * faces[3u * leaf + 2u];
	np_tri t;
	t.tax = a[0]; t.tay = a[1]; t.taz = a[2];
	t.ux = b[0] - a[0]; t.uy = b[1] - a[1]; t.uz = b[2] - a[2];
	t.vx = c[0] - a[0]; t.vy = c[1] - a[1]; t.vz = c[2] - a[2];
	t.uu = np_dot(t.ux, t.uy, t.uz, t.ux, t.uy, t.uz);
	t.uv = np_dot(t.ux, t.uy, t.uz, t.vx, t.vy, t.vz);
	t.vv = np_dot(t.vx, t.vy, t.vz, t.vx, t.vy, t.vz);
	t.D = t.uv * t.uv - t.uu * t.vv;
	return t;
}

/* One (point, leaf) pair: s, t, p and d2 into out6. */
void no_pair(const uint32_t *faces, const float *v4, uint32_t leaf, const float *q, float *out6) {
	const np_point r = np_nearest(no_leaf(faces, v4, leaf), q[0], q[1], q[2]);
	out6[0] = r.s; out6[1] = r.t; out6[2] = r.px; out6[3] = r.py; out6[4] = r.pz; out6[5] = r.d2;
}

/* Points [0, n) against leaves [0, leaves).  Any output may be NULL. */
void no_closest_points(const uint32_t *faces, uint32_t leaves, const float *v4, const float *n4, const float *q4, uint32_t n,
                       float max_distance, uint8_t *found, float *distance, uint32_t *leaf, float *bary, float *pos, float *normal) {
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
		float b0 = 0.0f, b1 = 0.0f, b2 = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f;
		if (ok) {
			b0 = 1.0f - best.s - best.t;
			b1 = best.s;
			b2 = best.t;
			if (normal) { /* the smooth normal of rt_hip_query.h: the weighted vertex normals, then normalised */
				const float *n0 = n4 + 4u * faces[3u * best_leaf], *n1 = n4 + 4u * faces[3u * best_leaf + 1u],
				            *n2 = n4 + 4u * faces[3u * best_leaf + 2u];
				float len;
				nx = (n0[0] * b0 + n1[0] * b1) + n2[0] * b2;
				ny = (n0[1] * b0 + n1[1] * b1) + n2[1] * b2;
				nz = (n0[2] * b0 + n1[2] * b1) + n2[2] * b2;
				len = sqrtf(np_dot(nx, ny, nz, nx, ny, nz));
				nx = nx / len; ny = ny / len; nz = nz / len;
			}
		}
		if (found)
			found[i] = (uint8_t) ok;
		if (distance)
			distance[i] = ok ? d : INFINITY;
		if (leaf)
			leaf[i] = ok ? best_leaf : NO_NONE;
		if (bary) {
			bary[3 * i] = b0; bary[3 * i + 1] = b1; bary[3 * i + 2] = b2;
		}
		if (pos) {
			pos[3 * i] = ok ? best.px : 0.0f; pos[3 * i + 1] = ok ? best.py : 0.0f; pos[3 * i + 2] = ok ? best.pz : 0.0f;
		}
		if (normal) {
			normal[3 * i] = nx; normal[3 * i + 1] = ny; normal[3 * i + 2] = nz;
		}
	}
}
