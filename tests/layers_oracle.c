/*
 * layers_oracle.c -- CPU oracle of the frame layers (include/rt_hip_layers.h).  TEST INFRASTRUCTURE ONLY.
 *
 * co_subpixel of tests/camera_oracle.c (itself shade_subpixel of oracle/rt_oracle.c, the restatement of the reference's
 * __kernel intersect, src/intersect_kernel.cl:278-310) once more, writing every layer instead of only the value.
 * Without a pose the ray is shade_subpixel's own -- origin (0, 0, 2), direction normalize((cx, cy, -1)) --; with one it is
 * co_subpixel's: w_k = ((right_k * cx) + (up_k * cy)) + forward_k, direction = normalize(w), origin = eye.  Everything
 * after the ray -- scene_hit, the smooth normal, shade, ambient_occlusion with index = y * W + x -- is the oracle's own,
 * called as shade_subpixel calls it.  Built by tests/layers_oracle.py with the oracle's flags (-O2 -ffp-contract=off
 * -fno-fast-math): no product or sum below is contracted.
 */
#include "../oracle/rt_oracle.c"

#define LO_NONE 0xFFFFFFFFu
#define LO_MAX_THREADS 16

typedef struct lo_layers {
	uint8_t *hit;
	float *distance;
	uint32_t *leaf;
	float *barycentric, *position, *normal, *direction, *shade, *ao, *value;
} lo_layers;

static void lo_store3(float *to, size_t i, v3 v) {
	to[3 * i + 0] = v.x;
	to[3 * i + 1] = v.y;
	to[3 * i + 2] = v.z;
}

/* pose: eye, right, up, forward -- twelve floats --, or NULL: the reference's camera */
static void lo_subpixel(const orc_params *p, const orc_scene *s, const float *pose, const float *table, uint32_t table_n,
                        uint32_t x, uint32_t y, const lo_layers *out) {
	const uint32_t W = p->width, H = p->height;
	const uint32_t index = y * W + x;
	const float a = p->focal_length * (float) (int32_t) (W > H ? W : H);
	const float cx = ((float) x + 0.5f) / a - (float) (int32_t) W / (2.0f * a);
	const float cy = -(((float) y + 0.5f) / a - (float) (int32_t) H / (2.0f * a));
	v3 eye = v3_make(0.0f, 0.0f, 2.0f);
	v3 ray_dir;
	if (pose) {
		const v3 R = v3_make(pose[3], pose[4], pose[5]), U = v3_make(pose[6], pose[7], pose[8]), F = v3_make(pose[9], pose[10], pose[11]);
		eye = v3_make(pose[0], pose[1], pose[2]);
		ray_dir = v3_normalize(v3_make(((R.x * cx) + (U.x * cy)) + F.x, ((R.y * cx) + (U.y * cy)) + F.y, ((R.z * cx) + (U.z * cy)) + F.z));
	} else {
		ray_dir = v3_normalize(v3_make(cx, cy, -1.0f));
	}
	hit_record rec;
	memset(&rec, 0, sizeof rec);
	rec.distance = INFINITY;
	ray_counters rc = { 0, 0 };
	const int hit = scene_hit(s, eye, ray_dir, &rec, 100000.0f, &rc);
	v3 normal = v3_make(0.0f, 0.0f, 0.0f);
	float shade = 0.0f, ao = 1.0f, value = 0.0f;
	if (hit) {
		/* get_smooth_normal, :118-127 */
		const uint32_t v0 = s->faces[rec.face_id + 0];
		const uint32_t v1 = s->faces[rec.face_id + 1];
		const uint32_t v2 = s->faces[rec.face_id + 2];
		normal = v3_normalize(v3_add(
		    v3_add(v3_scale(v3_load4(s->normals, v0), rec.barycentric.x), v3_scale(v3_load4(s->normals, v1), rec.barycentric.y)),
		    v3_scale(v3_load4(s->normals, v2), rec.barycentric.z)));
		shade = 1.0f;
		if (p->shading_enable) /* shade, :115-117 */
			shade = f_min(f_max(-v3_dot(normal, ray_dir), 0.f), 1.f);
		value = shade;
		if (p->ao_enable && p->ao_num_samples > 0) {
			ray_counters arc = { 0, 0 };
			uint64_t rays = 0, occluded = 0;
			ao = ambient_occlusion(p, s, table, table_n, rec.position, normal, index, &arc, &rays, &occluded);
			value *= ao;
		}
	} else {
		memset(&rec, 0, sizeof rec);
		rec.distance = INFINITY;
	}
	out->hit[index] = (uint8_t) (hit ? 1 : 0);
	out->distance[index] = rec.distance;
	out->leaf[index] = hit ? rec.face_id / 3u : LO_NONE;
	lo_store3(out->barycentric, index, rec.barycentric);
	lo_store3(out->position, index, rec.position);
	lo_store3(out->normal, index, normal);
	lo_store3(out->direction, index, ray_dir);
	out->shade[index] = shade;
	out->ao[index] = ao;
	out->value[index] = value;
}

/* Every layer of the whole frame (all ten arrays are written); returns the threads used, -1 if the direction table is
 * too large. */
int lo_render(const orc_params *p, const orc_scene *s, const float *pose, const lo_layers *out) {
	static float table_storage[3 * ORC_MAX_AO_DIRS];
	float *table = table_storage;
	uint32_t table_n = 0;
	if (p->ao_enable && p->ao_num_samples > 0 && p->ao_method == 0) {
		table_n = orc_ao_table(p, table, ORC_MAX_AO_DIRS);
		if (table_n > ORC_MAX_AO_DIRS)
			return -1;
	}
	int used = 1;
#ifdef _OPENMP
	used = omp_get_max_threads();
	if (used > LO_MAX_THREADS)
		used = LO_MAX_THREADS;
#pragma omp parallel for schedule(dynamic, 1) num_threads(used)
#endif
	for (int64_t y = 0; y < (int64_t) p->height; ++y)
		for (uint32_t x = 0; x < p->width; ++x)
			lo_subpixel(p, s, pose, table, table_n, x, (uint32_t) y, out);
	return used;
}
