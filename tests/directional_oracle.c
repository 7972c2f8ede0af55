/*
 * directional_oracle.c -- CPU oracle of the directional occlusion queries (include/rt_hip_directional.h).  TEST
 * INFRASTRUCTURE ONLY.
 *
 * The loop of the oracle's ambient_occlusion (oracle/rt_oracle.c, the restatement of the reference's
 * src/intersect_kernel.cl:214-277) stated once more with the oracle's own hemisphere_basis, orc_ao_table, rng_* and
 * scene_hit, so that what the function only counts can be seen: per point the origin, the directions as cast, the hit
 * flag of every ray -- bit k & 31 of word k >> 5 -- and the sum of the open rays' directions, added in ray order.
 * tests/test_directional_cpu.py holds it against ambient_occlusion itself (tests/ao_oracle.c).  Built by
 * tests/directional_oracle.py with the oracle's flags (-O2 -ffp-contract=off -fno-fast-math).
 */
#include "../oracle/rt_oracle.c"

#include <stdlib.h>

#define DRO_MAX_THREADS 16

static int dro_threads(void) {
#ifdef _OPENMP
	const int n = omp_get_max_threads();
	return n < DRO_MAX_THREADS ? n : DRO_MAX_THREADS;
#else
	return 1;
#endif
}

/* Rays per point with these options: the table's size (UNIFORM), ao_num_samples + 2 (RANDOM). */
uint32_t dro_rays_per_point(const orc_params *p) { return p->ao_method == 0 ? orc_ao_table(p, NULL, 0) : p->ao_num_samples + 2u; }

/* One ray of a point: recorded, cast, flagged, and -- if open -- added. */
static void dro_cast(const orc_params *p, const orc_scene *s, v3 origin, v3 dir, uint32_t k, float *dirs, uint32_t *row, v3 *sum) {
	ray_counters rc = { 0, 0 };
	if (dirs) {
		dirs[3 * k + 0] = dir.x;
		dirs[3 * k + 1] = dir.y;
		dirs[3 * k + 2] = dir.z;
	}
	if (scene_hit(s, origin, dir, NULL, p->ao_max_distance, &rc)) {
		if (row)
			row[k >> 5] |= 1u << (k & 31u);
	} else {
		sum->x = sum->x + dir.x;
		sum->y = sum->y + dir.y;
		sum->z = sum->z + dir.z;
	}
}

/* For i in [0, n), index_i = seeds[i], or i when seeds is NULL: origins float[n][3], dirs float[n][R][3], mask
 * uint32[n][ceil(R / 32)], bent float[n][3]; any may be NULL.  Returns R, 0 when the table does not fit or cannot be
 * allocated. */
uint32_t dro_directional(const orc_params *p, const orc_scene *s, const float *p4, const float *n4, const uint32_t *seeds, uint32_t n,
                         float *origins, float *dirs, uint32_t *mask, float *bent) {
	float *table = NULL;
	uint32_t table_n = 0;
	if (p->ao_method == 0) {
		table_n = orc_ao_table(p, NULL, 0);
		if (table_n > ORC_MAX_AO_DIRS)
			return 0;
		table = (float *) malloc(3u * sizeof(float) * (table_n ? table_n : 1u));
		if (!table)
			return 0;
		orc_ao_table(p, table, table_n);
	}
	const uint32_t R = p->ao_method == 0 ? table_n : p->ao_num_samples + 2u, W = (R + 31u) / 32u;
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 16) num_threads(dro_threads())
#endif
	for (int64_t i = 0; i < (int64_t) n; ++i) {
		const v3 point = v3_load4(p4, (uint32_t) i), normal = v3_load4(n4, (uint32_t) i);
		const uint32_t index = seeds ? seeds[i] : (uint32_t) i;
		float *const d = dirs ? dirs + 3u * (size_t) R * (size_t) i : NULL;
		uint32_t *const row = mask ? mask + (size_t) W * (size_t) i : NULL;
		for (uint32_t w = 0; row && w < W; ++w)
			row[w] = 0u;
		/* rt_oracle.c:249 */
		const v3 origin = v3_add(point, v3_scale(normal, 1.0f / 100000.0f));
		v3 sum = v3_make(0.0f, 0.0f, 0.0f);
		v3 basis_x, basis_z;
		if (p->ao_method == 0) {
			/* rt_oracle.c:253-262 */
			const v3 basis_y = normal;
			hemisphere_basis(basis_y, &basis_x, &basis_z);
			for (uint32_t k = 0; k < table_n; ++k) {
				const float xs = table[3 * k + 0], ys = table[3 * k + 1], zs = table[3 * k + 2];
				const v3 dir = v3_add(v3_add(v3_scale(basis_x, xs), v3_scale(basis_y, ys)), v3_scale(basis_z, zs));
				dro_cast(p, s, origin, dir, k, d, row, &sum);
			}
		} else {
			/* rt_oracle.c:268-289 */
			const v3 basis_y = v3_normalize(normal);
			hemisphere_basis(basis_y, &basis_x, &basis_z);
			rng128 rng;
			rng_seed(&rng, 536870923u * index);
			uint32_t count = p->ao_num_samples;
			++count;
			dro_cast(p, s, origin, normal, 0u, d, row, &sum);
			for (uint32_t j = 0; j < count; ++j) {
				const float xi1 = rng_float(&rng);
				const float xi2 = rng_float(&rng);
				const float theta = acosf(sqrtf(1.0f - xi1));
				const float phi = (float) (2.0 * xi2);
				const float xs = sinf(theta) * cl_cospi(phi);
				const float ys = cosf(theta);
				const float zs = sinf(theta) * cl_sinpi(phi);
				const v3 dir = v3_normalize(v3_add(v3_add(v3_scale(basis_x, xs), v3_scale(basis_y, ys)), v3_scale(basis_z, zs)));
				dro_cast(p, s, origin, dir, j + 1u, d, row, &sum);
			}
		}
		if (origins) {
			origins[3 * (size_t) i + 0] = origin.x;
			origins[3 * (size_t) i + 1] = origin.y;
			origins[3 * (size_t) i + 2] = origin.z;
		}
		if (bent) {
			bent[3 * (size_t) i + 0] = sum.x;
			bent[3 * (size_t) i + 1] = sum.y;
			bent[3 * (size_t) i + 2] = sum.z;
		}
	}
	free(table);
	return R;
}
