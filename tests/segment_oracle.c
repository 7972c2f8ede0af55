/*
 * segment_oracle.c -- CPU oracle of the segment queries (include/rt_hip_segment.h).  TEST INFRASTRUCTURE ONLY.
 *
 * Walks the uploaded tree as the oracle's own scene_hit does (oracle/rt_oracle.c, the restatement of the reference's
 * scene_intersect) with the oracle's box test at max_distance = t_hi, and restates the triangle test (tri_hit there, the
 * reference's triangle_intersect) with the interval on the plane parameter: a leaf is a blocker when the triangle is
 * accepted AND r > t_lo AND r < t_hi in binary32.  Built by tests/segment_oracle.py with the oracle's flags
 * (-O2 -ffp-contract=off -fno-fast-math).
 */
#include "../oracle/rt_oracle.c"

#define SO_NONE 0xFFFFFFFFu
#define SO_MAX_THREADS 16

static int so_threads(void) {
#ifdef _OPENMP
	const int n = omp_get_max_threads();
	return n < SO_MAX_THREADS ? n : SO_MAX_THREADS;
#else
	return 1;
#endif
}

/* tri_hit with the interval.  The reference's rejections in the reference's order, each on the value it is made on; the
 * interval is one more of them (a NaN r fails both comparisons).  rec may be NULL. */
static inline int seg_tri_hit(v3 ta, v3 tb, v3 tc, uint32_t face_id, v3 o, v3 d, float t_lo, float t_hi, hit_record *rec) {
	const v3 u = v3_sub(tb, ta);
	const v3 v = v3_sub(tc, ta);
	const v3 n = v3_cross(u, v);
	const v3 w0 = v3_sub(o, ta);
	const float a = -v3_dot(n, w0);
	const float b = v3_dot(n, d);
	if (fabsf(b) < 0.000001f)
		return 0;
	const float r = a / b;
	if ((double) r < 0.0)
		return 0;
	if (!(r > t_lo) || !(r < t_hi))
		return 0;
	const v3 ip = v3_add(o, v3_scale(d, r));
	const float uu = v3_dot(u, u);
	const float uv = v3_dot(u, v);
	const float vv = v3_dot(v, v);
	const v3 w = v3_sub(ip, ta);
	const float wu = v3_dot(u, w);
	const float wv = v3_dot(w, v);
	const float D = uv * uv - uu * vv;
	const float s = (uv * wv - vv * wu) / D;
	if (s < -0.00001f || (double) s > 1.00001)
		return 0;
	const float t = (uv * wu - uu * wv) / D;
	if (t < -0.00001f || (double) (s + t) > 1.00001)
		return 0;
	if (rec) {
		const float distance = v3_length(v3_sub(ip, o));
		if (rec->distance > distance) {
			rec->face_id = face_id;
			rec->barycentric = v3_make(1.0f - s - t, s, t);
			rec->position = ip;
			rec->distance = distance;
		}
	}
	return 1;
}

/* scene_hit's walk: the box test with max_distance = t_hi, the leaves in their order (so the first of equal distances is
 * the lowest leaf). */
static int seg_scene_hit(const orc_scene *s, v3 o, v3 d, float t_lo, float t_hi, hit_record *rec) {
	int blocked = 0;
	uint32_t triangle_index = 0;
	const uint32_t count = s->nodes[0];
	for (uint32_t i = 0; i < count;) {
		const uint32_t node_count = s->nodes[i];
		if (!box_hit(s->aabbs + 8u * (size_t) i, o, d, t_hi)) {
			triangle_index += (node_count + 1) >> 1;
			i += node_count;
		} else {
			if (node_count == 1) {
				const uint32_t face_id = triangle_index * 3;
				blocked |= seg_tri_hit(v3_load4(s->vertices, s->faces[face_id + 0]), v3_load4(s->vertices, s->faces[face_id + 1]),
				                       v3_load4(s->vertices, s->faces[face_id + 2]), face_id, o, d, t_lo, t_hi, rec);
				++triangle_index;
			}
			++i;
		}
	}
	return blocked;
}

/* The ray of a segment: o = a, d = b - a, one subtraction per component. */
static inline v3 so_direction(v3 a, v3 b) { return v3_sub(b, a); }

/* Closest form of segments [0, n): the record starts at distance +inf, the other fields 0.  Without a blocker: distance
 * +inf, leaf SO_NONE, barycentrics / position / normal 0.  Any output may be NULL. */
void so_closest(const orc_scene *s, const float *a4, const float *b4, uint32_t n, float t_lo, float t_hi, uint8_t *hit, float *distance,
                uint32_t *leaf, float *bary, float *pos, float *normal) {
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 256) num_threads(so_threads())
#endif
	for (int64_t i = 0; i < (int64_t) n; ++i) {
		const v3 o = v3_load4(a4, (uint32_t) i), d = so_direction(o, v3_load4(b4, (uint32_t) i));
		hit_record rec;
		memset(&rec, 0, sizeof rec);
		rec.distance = INFINITY;
		const int h = seg_scene_hit(s, o, d, t_lo, t_hi, &rec);
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
			leaf[i] = h ? rec.face_id / 3u : SO_NONE;
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

/* Occluded form: the boolean alone. */
void so_occluded(const orc_scene *s, const float *a4, const float *b4, uint32_t n, float t_lo, float t_hi, uint8_t *occluded) {
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 256) num_threads(so_threads())
#endif
	for (int64_t i = 0; i < (int64_t) n; ++i) {
		const v3 o = v3_load4(a4, (uint32_t) i);
		occluded[i] = (uint8_t) (seg_scene_hit(s, o, so_direction(o, v3_load4(b4, (uint32_t) i)), t_lo, t_hi, NULL) ? 1 : 0);
	}
}

/* The many-to-many form: mask[np][words], words = (nt + 31) / 32, and count[np]; either may be NULL. */
void so_visibility(const orc_scene *s, const float *p4, uint32_t np, const float *t4, uint32_t nt, float t_lo, float t_hi, uint32_t *mask,
                   uint32_t *count) {
	const uint32_t words = (nt + 31u) / 32u;
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 16) num_threads(so_threads())
#endif
	for (int64_t i = 0; i < (int64_t) np; ++i) {
		const v3 o = v3_load4(p4, (uint32_t) i);
		uint32_t sum = 0;
		if (mask)
			memset(mask + (size_t) i * words, 0, (size_t) words * sizeof(uint32_t));
		for (uint32_t j = 0; j < nt; ++j)
			if (seg_scene_hit(s, o, so_direction(o, v3_load4(t4, j)), t_lo, t_hi, NULL)) {
				++sum;
				if (mask)
					mask[(size_t) i * words + (j >> 5)] |= 1u << (j & 31u);
			}
		if (count)
			count[i] = sum;
	}
}
