/*
 * ao_oracle.c -- CPU oracle of the ambient-occlusion queries (include/rt_hip_ao.h).  TEST INFRASTRUCTURE ONLY.
 *
 * A batch wrapper of the oracle's own ambient_occlusion (oracle/rt_oracle.c, the restatement of the reference's
 * src/intersect_kernel.cl:214-277) with the UNIFORM direction table from orc_ao_table: value and hits per point, for
 * given points, normals and seeds.  Built by tests/ao_oracle.py with the oracle's flags (-O2 -ffp-contract=off
 * -fno-fast-math).
 */
#include "../oracle/rt_oracle.c"

#include <stdlib.h>

#define AOO_MAX_THREADS 16

static int aoo_threads(void) {
#ifdef _OPENMP
	const int n = omp_get_max_threads();
	return n < AOO_MAX_THREADS ? n : AOO_MAX_THREADS;
#else
	return 1;
#endif
}

/* ambient_occlusion(point_i, normal_i, index_i) for i in [0, n): index_i = seeds[i], or i when seeds is NULL.  `ao` and
 * `hits` may be NULL.  Returns the rays cast per point, 0 when the table does not fit or cannot be allocated. */
uint32_t aoo_ambient_occlusion(const orc_params *p, const orc_scene *s, const float *p4, const float *n4, const uint32_t *seeds,
                               uint32_t n, float *ao, uint32_t *hits) {
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
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 16) num_threads(aoo_threads())
#endif
	for (int64_t i = 0; i < (int64_t) n; ++i) {
		ray_counters rc = { 0, 0 };
		uint64_t rays = 0, occluded = 0;
		const float value = ambient_occlusion(p, s, table, table_n, v3_load4(p4, (uint32_t) i), v3_load4(n4, (uint32_t) i),
		                                      seeds ? seeds[i] : (uint32_t) i, &rc, &rays, &occluded);
		if (ao)
			ao[i] = value;
		if (hits)
			hits[i] = (uint32_t) occluded;
	}
	free(table);
	return p->ao_method == 0 ? table_n : p->ao_num_samples + 2u;
}
