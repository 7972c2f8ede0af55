/*
 * query_oracle.c -- CPU oracle of the ray queries (include/rt_hip_query.h).  TEST INFRASTRUCTURE ONLY.
 *
 * Batch wrappers of the oracle's own scene_hit (oracle/rt_oracle.c, the restatement of the reference's scene_intersect)
 * for closest hit and any hit, the smooth normal as shade_subpixel computes it there, and the reference camera's rays.
 * Built by tests/query_oracle.py with the oracle's flags (-O2 -ffp-contract=off -fno-fast-math).
 */
#include "../oracle/rt_oracle.c"

#define QO_NONE 0xFFFFFFFFu
#define QO_MAX_THREADS 16

static int qo_threads(void) {
#ifdef _OPENMP
	const int n = omp_get_max_threads();
	return n < QO_MAX_THREADS ? n : QO_MAX_THREADS;
#else
	return 1;
#endif
}

/* Closest hit of rays [0, n): scene_hit with rec.distance = INFINITY and the other fields 0 on entry.  Without a hit:
 * distance +inf, leaf QO_NONE, barycentrics / position / normal 0.  Any output may be NULL. */
void qo_closest(const orc_scene *s, const float *o4, const float *d4, uint32_t n, float max_distance, uint8_t *hit,
                float *distance, uint32_t *leaf, float *bary, float *pos, float *normal) {
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 256) num_threads(qo_threads())
#endif
	for (int64_t i = 0; i < (int64_t) n; ++i) {
		const v3 o = v3_load4(o4, (uint32_t) i), d = v3_load4(d4, (uint32_t) i);
		hit_record rec;
		memset(&rec, 0, sizeof rec);
		rec.distance = INFINITY;
		ray_counters rc = { 0, 0 };
		const int h = scene_hit(s, o, d, &rec, max_distance, &rc);
		v3 nrm = v3_make(0.0f, 0.0f, 0.0f);
		if (h) { /* get_smooth_normal, as shade_subpixel */
			const uint32_t v0 = s->faces[rec.face_id + 0], v1 = s->faces[rec.face_id + 1], v2 = s->faces[rec.face_id + 2];
			nrm = v3_normalize(v3_add(v3_add(v3_scale(v3_load4(s->normals, v0), rec.barycentric.x),
			                                 v3_scale(v3_load4(s->normals, v1), rec.barycentric.y)),
			                          v3_scale(v3_load4(s->normals, v2), rec.barycentric.z)));
		} else {
			memset(&rec, 0, sizeof rec);
			rec.distance = INFINITY;
		}
		if (hit)
			hit[i] = (uint8_t) (h ? 1 : 0);
		if (distance)
			distance[i] = rec.distance;
		if (leaf)
			leaf[i] = h ? rec.face_id / 3u : QO_NONE;
		if (bary) {
			bary[3 * i + 0] = rec.barycentric.x;
			bary[3 * i + 1] = rec.barycentric.y;
			bary[3 * i + 2] = rec.barycentric.z;
		}
		if (pos) {
			pos[3 * i + 0] = rec.position.x;
			pos[3 * i + 1] = rec.position.y;
			pos[3 * i + 2] = rec.position.z;
		}
		if (normal) {
			normal[3 * i + 0] = nrm.x;
			normal[3 * i + 1] = nrm.y;
			normal[3 * i + 2] = nrm.z;
		}
	}
}

/* Any hit: the boolean of scene_hit without a record (as the reference's ambient_occlusion calls it). */
void qo_any(const orc_scene *s, const float *o4, const float *d4, uint32_t n, float max_distance, uint8_t *hit) {
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 256) num_threads(qo_threads())
#endif
	for (int64_t i = 0; i < (int64_t) n; ++i) {
		ray_counters rc = { 0, 0 };
		hit[i] = (uint8_t) (scene_hit(s, v3_load4(o4, (uint32_t) i), v3_load4(d4, (uint32_t) i), NULL, max_distance, &rc) ? 1 : 0);
	}
}

/* The reference camera's ray of every sub-pixel (shade_subpixel): origin (0, 0, 2), index y * width + x. */
void qo_camera_rays(const orc_params *p, float *o4, float *d4) {
	const uint32_t W = p->width, H = p->height;
	const float a = p->focal_length * (float) (int32_t) (W > H ? W : H);
	for (uint32_t y = 0; y < H; ++y)
		for (uint32_t x = 0; x < W; ++x) {
			const size_t i = (size_t) y * W + x;
			const v3 dir = v3_normalize(v3_make(((float) x + 0.5f) / a - (float) (int32_t) W / (2.0f * a),
			                                    -(((float) y + 0.5f) / a - (float) (int32_t) H / (2.0f * a)), -1.0f));
			o4[4 * i + 0] = 0.0f; o4[4 * i + 1] = 0.0f; o4[4 * i + 2] = 2.0f; o4[4 * i + 3] = 0.0f;
			d4[4 * i + 0] = dir.x; d4[4 * i + 1] = dir.y; d4[4 * i + 2] = dir.z; d4[4 * i + 3] = 0.0f;
		}
}

/* The head-light term of a sub-pixel from its query results (shade_subpixel, :296-304): dot in the product's order. */
void qo_shade(const uint8_t *hit, const float *normal, const float *d4, uint32_t n, int shading, float *value) {
	for (uint32_t i = 0; i < n; ++i) {
		float v = 0.0f;
		if (hit[i]) {
			v = 1.0f;
			if (shading) {
				const v3 nn = v3_make(normal[3 * i], normal[3 * i + 1], normal[3 * i + 2]);
				v = f_min(f_max(-v3_dot(nn, v3_load4(d4, i)), 0.f), 1.f);
			}
		}
		value[i] = v;
	}
}
