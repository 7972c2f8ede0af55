/*
 * instance_oracle.c -- CPU oracle of the instanced ray queries (include/rt_hip_instances.h).  TEST INFRASTRUCTURE ONLY.
 *
 * Walks the top-level tree it is handed -- the library's own, read back or planned -- with the oracle's box test
 * (oracle/rt_oracle.c, box_hit: the reference's aabb_intersect) and the world ray; at a leaf it forms the object ray with
 * the header's operations from the twelve floats of object_from_world it is handed, walks the scene's tree as scene_hit
 * does there, and restates the triangle test (tri_hit, the reference's triangle_intersect) so that it hands back r = a / b.
 * A candidate's position is o + r d with the WORLD ray, its distance that point's length from o; the record kept is the
 * minimum of (distance, instance, leaf).  Built by tests/instance_oracle.py with the oracle's flags
 * (-O2 -ffp-contract=off -fno-fast-math).
 */
#include "../oracle/rt_oracle.c"

#define IO_NONE 0xFFFFFFFFu
#define IO_MAX_THREADS 16

typedef struct io_node { /* the record of the top-level tree */
	float lo[3];
	uint32_t skip;
	float hi[3];
	uint32_t leaf;
} io_node;

typedef struct io_record {
	uint32_t instance, leaf;
	float s, t;
	v3 position;
	float distance;
} io_record;

static int io_threads(void) {
#ifdef _OPENMP
	const int n = omp_get_max_threads();
	return n < IO_MAX_THREADS ? n : IO_MAX_THREADS;
#else
	return 1;
#endif
}

/* tri_hit's rejections in tri_hit's order; says r, s, t of an accepted triangle. */
static inline int io_tri_hit(v3 ta, v3 tb, v3 tc, v3 o, v3 d, float *r_out, float *s_out, float *t_out) {
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

/* One row of O applied to a point (w = 1) or a direction (w = 0): the header's association. */
static inline float io_row_point(const float *m, v3 p) { return ((m[0] * p.x + m[1] * p.y) + m[2] * p.z) + m[3]; }
static inline float io_row_direction(const float *m, v3 p) { return (m[0] * p.x + m[1] * p.y) + m[2] * p.z; }

/* The scene's own walk for the object ray of instance k; the world ray makes the record.  rec NULL: the boolean alone. */
static int io_instance_hit(const orc_scene *s, uint32_t k, const float *O, v3 o, v3 d, float max_distance, io_record *rec) {
	const v3 oo = v3_make(io_row_point(O, o), io_row_point(O + 4, o), io_row_point(O + 8, o));
	const v3 od = v3_make(io_row_direction(O, d), io_row_direction(O + 4, d), io_row_direction(O + 8, d));
	int found = 0;
	uint32_t triangle_index = 0;
	const uint32_t count = s->nodes[0];
	for (uint32_t i = 0; i < count;) {
		const uint32_t node_count = s->nodes[i];
		if (!box_hit(s->aabbs + 8u * (size_t) i, oo, od, max_distance)) {
			triangle_index += (node_count + 1) >> 1;
			i += node_count;
		} else {
			if (node_count == 1) {
				const uint32_t face_id = triangle_index * 3;
				float r, bs, bt;
				if (io_tri_hit(v3_load4(s->vertices, s->faces[face_id + 0]), v3_load4(s->vertices, s->faces[face_id + 1]),
				               v3_load4(s->vertices, s->faces[face_id + 2]), oo, od, &r, &bs, &bt)) {
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
	}
	return found;
}

/* The top-level walk: a record is entered when its box passes, a leaf record is an instance. */
static int io_scene_hit(const orc_scene *s, const io_node *top, uint32_t top_count, const float *O, v3 o, v3 d, float max_distance,
                        io_record *rec) {
	int found = 0;
	for (uint32_t i = 0; i < top_count;) {
		float bb[8] = { top[i].lo[0], top[i].lo[1], top[i].lo[2], 0.0f, top[i].hi[0], top[i].hi[1], top[i].hi[2], 0.0f };
		if (!box_hit(bb, o, d, max_distance)) {
			i += top[i].skip;
			continue;
		}
		if (top[i].leaf != IO_NONE) {
			found |= io_instance_hit(s, top[i].leaf, O + 12u * (size_t) top[i].leaf, o, d, max_distance, rec);
			if (found && !rec)
				return 1;
		}
		++i;
	}
	return found;
}

/* Closest form of rays [0, n).  Any output may be NULL. */
void io_closest(const orc_scene *s, const io_node *top, uint32_t top_count, const float *O, const float *o4, const float *d4, uint32_t n,
                float max_distance, uint8_t *hit, float *distance, uint32_t *leaf, float *bary, float *pos, float *normal, uint32_t *instance) {
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 64) num_threads(io_threads())
#endif
	for (int64_t i = 0; i < (int64_t) n; ++i) {
		const v3 o = v3_load4(o4, (uint32_t) i), d = v3_load4(d4, (uint32_t) i);
		io_record rec;
		memset(&rec, 0, sizeof rec);
		rec.distance = INFINITY;
		const int h = io_scene_hit(s, top, top_count, O, o, d, max_distance, &rec);
		const int kept = h && rec.distance < INFINITY;
		const v3 b = kept ? v3_make(1.0f - rec.s - rec.t, rec.s, rec.t) : v3_make(0.0f, 0.0f, 0.0f);
		v3 nrm = v3_make(0.0f, 0.0f, 0.0f);
		if (h) { /* get_smooth_normal before its normalisation, the inverse's transpose, one normalisation */
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
			leaf[i] = h ? rec.leaf : IO_NONE;
		if (instance)
			instance[i] = h ? rec.instance : IO_NONE;
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
void io_occluded(const orc_scene *s, const io_node *top, uint32_t top_count, const float *O, const float *o4, const float *d4, uint32_t n,
                 float max_distance, uint8_t *occluded) {
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 64) num_threads(io_threads())
#endif
	for (int64_t i = 0; i < (int64_t) n; ++i)
		occluded[i] = (uint8_t) (io_scene_hit(s, top, top_count, O, v3_load4(o4, (uint32_t) i), v3_load4(d4, (uint32_t) i), max_distance, NULL) ? 1 : 0);
}
