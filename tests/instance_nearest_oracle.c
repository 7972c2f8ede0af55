/*
 * instance_nearest_oracle.c -- CPU oracle of the instanced closest-point queries (include/rt_hip_instance_nearest.h).
 * TEST INFRASTRUCTURE ONLY.
 *
 * The contract by brute force: every point against every pair (instance, leaf), instances outermost, leaves in leaf order;
 * no tree, no pruning, no object-space point.  The world triangle, the three-key order and the per-leaf routine are the
 * files the kernel compiles (csrc/instance_nearest.h, csrc/nearest_point.h); a leaf's object-space values are made as
 * tests/nearest_oracle.c makes them.  The normal is rt_hip_instances.h's: the raw smooth normal, the inverse's transpose, one
 * normalisation.  Built by tests/instance_nearest_oracle.py with -O2 -ffp-contract=off -fno-fast-math.
 */
#include <stdint.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#include "../opencl_raytracer_amd/csrc/nearest_point.h"
#include "../opencl_raytracer_amd/csrc/instance_nearest.h"

#define INO_NONE 0xFFFFFFFFu
#define INO_MAX_THREADS 16

static int ino_threads(void) {
#ifdef _OPENMP
	const int n = omp_get_max_threads();
	return n < INO_MAX_THREADS ? n : INO_MAX_THREADS;
#else
	return 1;
#endif
}

/* The values the device holds of leaf `leaf` (tests/nearest_oracle.c, no_leaf). */
static np_tri ino_leaf(const uint32_t *faces, const float *v4, uint32_t leaf) {
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

static inp_rows ino_rows(const float *m12) {
	inp_rows r;
	memcpy(r.m, m12, sizeof r.m);
	return r;
}

/* Points [0, n) against instances [0, instances) x leaves [0, leaves).  W, O: float[instances][12].  Any output may be NULL. */
void ino_closest_points(const uint32_t *faces, uint32_t leaves, const float *v4, const float *n4, const float *W, const float *O,
                        uint32_t instances, const float *q4, uint32_t n, float max_distance, uint8_t *found, float *distance,
                        uint32_t *leaf, float *bary, float *pos, float *normal, uint32_t *instance) {
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 16) num_threads(ino_threads())
#endif
	for (int64_t i = 0; i < (int64_t) n; ++i) {
		const float qx = q4[4 * i], qy = q4[4 * i + 1], qz = q4[4 * i + 2];
		float best_d2 = INFINITY;
		uint32_t best_leaf = INO_NONE, best_instance = INO_NONE;
		np_point best;
		memset(&best, 0, sizeof best);
		if (np_radius_ok(max_distance) && np_point_ok(qx, qy, qz))
			for (uint32_t k = 0; k < instances; ++k) {
				const inp_rows w = ino_rows(W + 12u * (size_t) k);
				for (uint32_t l = 0; l < leaves; ++l) {
					const np_point r = np_nearest(inp_world_tri(w, ino_leaf(faces, v4, l)), qx, qy, qz);
					if (inp_better(r.d2, k, l, best_d2, best_instance, best_leaf)) {
						best_d2 = r.d2;
						best_instance = k;
						best_leaf = l;
						best = r;
					}
				}
			}
		const float d = sqrtf(best_d2);
		const int ok = best_d2 < INFINITY && d <= max_distance;
		float b0 = 0.0f, b1 = 0.0f, b2 = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f;
		if (ok) {
			b0 = 1.0f - best.s - best.t;
			b1 = best.s;
			b2 = best.t;
			if (normal) {
				const float *n0 = n4 + 4u * faces[3u * best_leaf], *n1 = n4 + 4u * faces[3u * best_leaf + 1u],
				            *n2 = n4 + 4u * faces[3u * best_leaf + 2u], *m = O + 12u * (size_t) best_instance;
				const float rx = (n0[0] * b0 + n1[0] * b1) + n2[0] * b2;
				const float ry = (n0[1] * b0 + n1[1] * b1) + n2[1] * b2;
				const float rz = (n0[2] * b0 + n1[2] * b1) + n2[2] * b2;
				float len;
				nx = (m[0] * rx + m[4] * ry) + m[8] * rz;
				ny = (m[1] * rx + m[5] * ry) + m[9] * rz;
				nz = (m[2] * rx + m[6] * ry) + m[10] * rz;
				len = sqrtf(np_dot(nx, ny, nz, nx, ny, nz));
				nx = nx / len; ny = ny / len; nz = nz / len;
			}
		}
		if (found)
			found[i] = (uint8_t) ok;
		if (distance)
			distance[i] = ok ? d : INFINITY;
		if (leaf)
			leaf[i] = ok ? best_leaf : INO_NONE;
		if (instance)
			instance[i] = ok ? best_instance : INO_NONE;
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
