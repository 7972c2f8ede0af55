/*
 * instance_segment_oracle.c -- CPU oracle of the instanced segment queries (include/rt_hip_instance_segments.h).
 * TEST INFRASTRUCTURE ONLY.
 *
 * Written from the header.  A segment (a, b) is the world ray o = a, d = b - a, one subtraction per component.  The
 * top-level tree it is handed -- the library's own, read back or planned -- is walked with the oracle's box test
 * (oracle/rt_oracle.c, box_hit: the reference's aabb_intersect) for the world ray at max_distance = t_hi; at a leaf the
 * object ray is formed with rt_hip_instances.h's operations from the twelve floats of object_from_world, the scene's tree
 * is walked as scene_hit walks it, at max_distance = t_hi too, and the triangle test (tri_hit, the reference's
 * triangle_intersect) is restated on the OBJECT ray with the interval on its plane parameter: r > t_lo and r < t_hi in
 * binary32, both false for a NaN.  A blocker's position is o + r d with the WORLD ray, its distance that point's length
 * from o; the record kept is the minimum of (distance, instance, leaf).  Pair forms only: the mask form is the occluded
 * form of the pairs written out.  Built by tests/instance_segment_oracle.py with the oracle's flags
 * (-O2 -ffp-contract=off -fno-fast-math).
 */
#include "../oracle/rt_oracle.c"

#define ISO_NONE 0xFFFFFFFFu
#define ISO_MAX_THREADS 16

typedef struct iso_node { /* the record of the top-level tree */
	float lo[3];
	uint32_t skip;
	float hi[3];
	uint32_t leaf;
} iso_node;

typedef struct iso_record {
	uint32_t instance, leaf;
	float s, t;
	v3 position;
	float distance;
} iso_record;

static int iso_threads(void) {
#ifdef _OPENMP
	const int n = omp_get_max_threads();
	return n < ISO_MAX_THREADS ? n : ISO_MAX_THREADS;
#else
	return 1;
#endif
}

/* triangle_intersect's rejections in its order, the interval among them where r is known; says r, s, t of a blocker. */
static inline int iso_tri_blocks(v3 ta, v3 tb, v3 tc, v3 o, v3 d, float t_lo, float t_hi, float *r_out, float *s_out, float *t_out) {
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
	*r_out = r;
	*s_out = s;
	*t_out = t;
	return 1;
}

/* One row of O applied to a point (w = 1) or a direction (w = 0): rt_hip_instances.h's association. */
static inline float iso_row_point(const float *m, v3 p) { return ((m[0] * p.x + m[1] * p.y) + m[2] * p.z) + m[3]; }
static inline float iso_row_direction(const float *m, v3 p) { return (m[0] * p.x + m[1] * p.y) + m[2] * p.z; }

/* The blockers of the segment in instance k.  rec NULL: the boolean alone, at the first of them. */
static int iso_instance_blocks(const orc_scene *s, uint32_t k, const float *O, v3 o, v3 d, float t_lo, float t_hi, iso_record *rec) {
	const v3 oo = v3_make(iso_row_point(O, o), iso_row_point(O + 4, o), iso_row_point(O + 8, o));
	const v3 od = v3_make(iso_row_direction(O, d), iso_row_direction(O + 4, d), iso_row_direction(O + 8, d));
	int found = 0;
	uint32_t triangle_index = 0;
	const uint32_t count = s->nodes[0];
	for (uint32_t i = 0; i < count;) {
		const uint32_t node_count = s->nodes[i];
		if (!box_hit(s->aabbs + 8u * (size_t) i, oo, od, t_hi)) {
			triangle_index += (node_count + 1) >> 1;
			i += node_count;
			continue;
		}
		if (node_count == 1) {
			const uint32_t face_id = triangle_index * 3;
			float r, bs, bt;
			if (iso_tri_blocks(v3_load4(s->vertices, s->faces[face_id + 0]), v3_load4(s->vertices, s->faces[face_id + 1]),
			                   v3_load4(s->vertices, s->faces[face_id + 2]), oo, od, t_lo, t_hi, &r, &bs, &bt)) {
				found = 1;
				if (!rec)
					return 1;
				const v3 p = v3_make(o.x + r * d.x, o.y + r * d.y, o.z + r * d.z);
				const float distance = v3_length(v3_sub(p, o));
				const int lower = k < rec->instance || (k == rec->instance && triangle_index < rec->leaf);
				if (rec->distance > distance || (rec->distance == distance && lower && distance < INFINITY)) {
					rec->instance = k;
					rec->leaf = triangle_index;
					rec->s = bs;
					rec->t = bt;
					rec->position = p;
					rec->distance = distance;
				}
			}
			++triangle_index;
		}
		++i;
	}
	return found;
}

/* The top-level walk: an instance is entered when every box on the way to its leaf passes for the world ray and t_hi. */
static int iso_blocks(const orc_scene *s, const iso_node *top, uint32_t top_count, const float *O, v3 o, v3 d, float t_lo, float t_hi,
                      iso_record *rec) {
	int found = 0;
	for (uint32_t i = 0; i < top_count;) {
		const float bb[8] = { top[i].lo[0], top[i].lo[1], top[i].lo[2], 0.0f, top[i].hi[0], top[i].hi[1], top[i].hi[2], 0.0f };
		if (!box_hit(bb, o, d, t_hi)) {
			i += top[i].skip;
			continue;
		}
		if (top[i].leaf != ISO_NONE) {
			found |= iso_instance_blocks(s, top[i].leaf, O + 12u * (size_t) top[i].leaf, o, d, t_lo, t_hi, rec);
			if (found && !rec)
				return 1;
		}
		++i;
	}
	return found;
}

/* Closest form of segments [0, n).  Any output may be NULL. */
void iso_closest(const orc_scene *s, const iso_node *top, uint32_t top_count, const float *O, const float *a4, const float *b4, uint32_t n,
                 float t_lo, float t_hi, uint8_t *hit, float *distance, uint32_t *leaf, float *bary, float *pos, float *normal,
                 uint32_t *instance) {
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 64) num_threads(iso_threads())
#endif
	for (int64_t i = 0; i < (int64_t) n; ++i) {
		const v3 o = v3_load4(a4, (uint32_t) i), d = v3_sub(v3_load4(b4, (uint32_t) i), o);
		iso_record rec;
		memset(&rec, 0, sizeof rec);
		rec.distance = INFINITY;
		const int h = iso_blocks(s, top, top_count, O, o, d, t_lo, t_hi, &rec);
		const int kept = h && rec.distance < INFINITY;
		const v3 b = kept ? v3_make(1.0f - rec.s - rec.t, rec.s, rec.t) : v3_make(0.0f, 0.0f, 0.0f);
		v3 nrm = v3_make(0.0f, 0.0f, 0.0f);
		if (h) { /* the raw weighted sum, the inverse's transpose, one normalisation */
			const uint32_t face_id = rec.leaf * 3u;
			const uint32_t v0 = s->faces[face_id + 0], v1 = s->faces[face_id + 1], v2 = s->faces[face_id + 2];
			const v3 raw = v3_add(v3_add(v3_scale(v3_load4(s->normals, v0), b.x), v3_scale(v3_load4(s->normals, v1), b.y)),
			                      v3_scale(v3_load4(s->normals, v2), b.z));
			const float *m = O + 12u * (size_t) rec.instance;
			nrm = v3_normalize(v3_make((m[0] * raw.x + m[4] * raw.y) + m[8] * raw.z, (m[1] * raw.x + m[5] * raw.y) + m[9] * raw.z,
			                           (m[2] * raw.x + m[6] * raw.y) + m[10] * raw.z));
		}
		if (hit)
			hit[i] = (uint8_t) (h ? 1 : 0);
		if (distance)
			distance[i] = rec.distance;
		if (leaf)
			leaf[i] = h ? rec.leaf : ISO_NONE;
		if (instance)
			instance[i] = h ? rec.instance : ISO_NONE;
		if (bary) {
			bary[3 * i + 0] = b.x;
			bary[3 * i + 1] = b.y;
			bary[3 * i + 2] = b.z;
		}
		if (pos) {
			pos[3 * i + 0] = kept ? rec.position.x : 0.0f;
			pos[3 * i + 1] = kept ? rec.position.y : 0.0f;
			pos[3 * i + 2] = kept ? rec.position.z : 0.0f;
		}
		if (normal) {
			normal[3 * i + 0] = nrm.x;
			normal[3 * i + 1] = nrm.y;
			normal[3 * i + 2] = nrm.z;
		}
	}
}

/* Occluded form: the boolean alone. */
void iso_occluded(const orc_scene *s, const iso_node *top, uint32_t top_count, const float *O, const float *a4, const float *b4, uint32_t n,
                  float t_lo, float t_hi, uint8_t *occluded) {
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 64) num_threads(iso_threads())
#endif
	for (int64_t i = 0; i < (int64_t) n; ++i) {
		const v3 o = v3_load4(a4, (uint32_t) i);
		occluded[i] = (uint8_t) (iso_blocks(s, top, top_count, O, o, v3_sub(v3_load4(b4, (uint32_t) i), o), t_lo, t_hi, NULL) ? 1 : 0);
	}
}
