/*
 * camera_oracle.c -- CPU oracle of the posed camera (include/rt_hip_camera.h).  TEST INFRASTRUCTURE ONLY.
 *
 * shade_subpixel of oracle/rt_oracle.c (the restatement of the reference's __kernel intersect, src/intersect_kernel.cl:
 * 278-310) once more, with the ray's origin and direction made from a pose as the camera contract states it: per
 * component w_k = ((right_k * cx) + (up_k * cy)) + forward_k, direction = normalize(w), origin = eye.  Everything
 * after the ray -- scene_hit, the smooth normal, shade, ambient_occlusion with index = y * W + x -- is the oracle's own,
 * called as shade_subpixel calls it.  Built by tests/camera_oracle.py with the oracle's flags (-O2 -ffp-contract=off
 * -fno-fast-math): no product or sum below is contracted.
 */
#include "../oracle/rt_oracle.c"

#define CO_MAX_THREADS 16

/* pose: eye, right, up, forward -- twelve floats */
static float co_subpixel(const orc_params *p, const orc_scene *s, const float *pose, const float *table, uint32_t table_n,
                         uint32_t x, uint32_t y, orc_counters *c) {
	const uint32_t W = p->width, H = p->height;
	const uint32_t index = y * W + x;
	const v3 eye = v3_make(pose[0], pose[1], pose[2]);
	const v3 R = v3_make(pose[3], pose[4], pose[5]), U = v3_make(pose[6], pose[7], pose[8]), F = v3_make(pose[9], pose[10], pose[11]);
	const float a = p->focal_length * (float) (int32_t) (W > H ? W : H);
	const float cx = ((float) x + 0.5f) / a - (float) (int32_t) W / (2.0f * a);
	const float cy = -(((float) y + 0.5f) / a - (float) (int32_t) H / (2.0f * a));
	const v3 w = v3_make(((R.x * cx) + (U.x * cy)) + F.x, ((R.y * cx) + (U.y * cy)) + F.y, ((R.z * cx) + (U.z * cy)) + F.z);
	const v3 ray_dir = v3_normalize(w);
	hit_record rec;
	memset(&rec, 0, sizeof rec);
	rec.distance = INFINITY;
	ray_counters rc = { 0, 0 };
	const int hit = scene_hit(s, eye, ray_dir, &rec, 100000.0f, &rc);
	c->primary_rays++;
	c->primary_node_visits += rc.node_visits;
	c->primary_tri_tests += rc.tri_tests;
	if (!hit)
		return 0.0f;
	c->primary_hits++;
	/* get_smooth_normal, :118-127 */
	const uint32_t v0 = s->faces[rec.face_id + 0];
	const uint32_t v1 = s->faces[rec.face_id + 1];
	const uint32_t v2 = s->faces[rec.face_id + 2];
	const v3 normal = v3_normalize(v3_add(
	    v3_add(v3_scale(v3_load4(s->normals, v0), rec.barycentric.x), v3_scale(v3_load4(s->normals, v1), rec.barycentric.y)),
	    v3_scale(v3_load4(s->normals, v2), rec.barycentric.z)));
	float value = 1.0f;
	if (p->shading_enable) /* shade, :115-117 */
		value = f_min(f_max(-v3_dot(normal, ray_dir), 0.f), 1.f);
	if (p->ao_enable && p->ao_num_samples > 0) {
		ray_counters arc = { 0, 0 };
		value *= ambient_occlusion(p, s, table, table_n, rec.position, normal, index, &arc, &c->ao_rays, &c->ao_occluded);
		c->ao_node_visits += arc.node_visits;
		c->ao_tri_tests += arc.tri_tests;
	}
	return value;
}

/* The whole frame, as orc_render; returns the threads used, -1 if the direction table is too large. */
int co_render(const orc_params *p, const orc_scene *s, const float *pose, float *image, orc_counters *counters) {
	static float table_storage[3 * ORC_MAX_AO_DIRS];
	float *table = table_storage;
	uint32_t table_n = 0;
	if (p->ao_enable && p->ao_num_samples > 0 && p->ao_method == 0) {
		table_n = orc_ao_table(p, table, ORC_MAX_AO_DIRS);
		if (table_n > ORC_MAX_AO_DIRS)
			return -1;
	}
	orc_counters total;
	memset(&total, 0, sizeof total);
	int used = 1;
#ifdef _OPENMP
	used = omp_get_max_threads();
	if (used > CO_MAX_THREADS)
		used = CO_MAX_THREADS;
#pragma omp parallel num_threads(used)
#endif
	{
		orc_counters local;
		memset(&local, 0, sizeof local);
#ifdef _OPENMP
#pragma omp for schedule(dynamic, 1)
#endif
		for (int64_t y = 0; y < (int64_t) p->height; ++y)
			for (uint32_t x = 0; x < p->width; ++x)
				image[(size_t) y * p->width + x] = co_subpixel(p, s, pose, table, table_n, x, (uint32_t) y, &local);
#ifdef _OPENMP
#pragma omp critical
#endif
		{
			total.primary_rays += local.primary_rays;
			total.primary_hits += local.primary_hits;
			total.primary_node_visits += local.primary_node_visits;
			total.primary_tri_tests += local.primary_tri_tests;
			total.ao_rays += local.ao_rays;
			total.ao_occluded += local.ao_occluded;
			total.ao_node_visits += local.ao_node_visits;
			total.ao_tri_tests += local.ao_tri_tests;
		}
	}
	if (counters)
		*counters = total;
	return used;
}
