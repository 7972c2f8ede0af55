/*
 * instance_multihit_oracle.c -- CPU oracle of the instanced multi-hit queries (include/rt_hip_instance_multihit.h).  TEST
 * INFRASTRUCTURE ONLY.
 *
 * tests/instance_oracle.c's two walks -- the top-level tree it is handed with the oracle's box test and the world ray, at a
 * leaf the object ray from the twelve floats of object_from_world, the scene's own tree as scene_hit walks it, the triangle
 * test restated so that it hands back r = a / b -- with tests/multihit_oracle.c's bookkeeping: EVERY candidate is collected
 * (position o + r d with the WORLD ray, distance that point's length from o, reported as +inf where it is not below +inf),
 * the candidates are sorted by (reported distance, instance, leaf), and the count and the first k of them are written, the
 * normal of each as instance_oracle.c makes the closest hit's.  Built by tests/instance_multihit_oracle.py with the
 * oracle's flags (-O2 -ffp-contract=off -fno-fast-math).
 */
#include "../oracle/rt_oracle.c"

#include <stdlib.h>

#define IM_NONE 0xFFFFFFFFu
#define IM_MAX_THREADS 16

typedef struct im_node { /* the record of the top-level tree */
	float lo[3];
	uint32_t skip;
	float hi[3];
	uint32_t leaf;
} im_node;

typedef struct im_member {
	uint32_t instance, leaf;
	int kept; /* a computed distance below +inf */
	float s, t;
	v3 position;
	float distance; /* as reported */
} im_member;

typedef struct im_list {
	im_member *at;
	size_t members, room;
} im_list;

static int im_threads(void) {
#ifdef _OPENMP
	const int n = omp_get_max_threads();
	return n < IM_MAX_THREADS ? n : IM_MAX_THREADS;
#else
	return 1;
#endif
}

static int im_before(const void *pa, const void *pb) {
	const im_member *a = (const im_member *) pa, *b = (const im_member *) pb;
	if (a->distance < b->distance)
		return -1;
	if (a->distance > b->distance)
		return 1;
	if (a->instance != b->instance)
		return a->instance < b->instance ? -1 : 1;
	return a->leaf < b->leaf ? -1 : (a->leaf > b->leaf ? 1 : 0);
}

/* tri_hit's rejections in tri_hit's order; says r, s, t of an accepted triangle (instance_oracle.c: io_tri_hit). */
static inline int im_tri_hit(v3 ta, v3 tb, v3 tc, v3 o, v3 d, float *r_out, float *s_out, float *t_out) {
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
static inline float im_row_point(const float *m, v3 p) { return ((m[0] * p.x + m[1] * p.y) + m[2] * p.z) + m[3]; }
static inline float im_row_direction(const float *m, v3 p) { return (m[0] * p.x + m[1] * p.y) + m[2] * p.z; }

/* The scene's own walk for the object ray of instance k: every accepted leaf onto the list, its record the world ray's. */
static void im_instance_members(const orc_scene *s, uint32_t k, const float *O, v3 o, v3 d, float max_distance, im_list *list) {
	const v3 oo = v3_make(im_row_point(O, o), im_row_point(O + 4, o), im_row_point(O + 8, o));
	const v3 od = v3_make(im_row_direction(O, d), im_row_direction(O + 4, d), im_row_direction(O + 8, d));
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
				if (im_tri_hit(v3_load4(s->vertices, s->faces[face_id + 0]), v3_load4(s->vertices, s->faces[face_id + 1]),
				               v3_load4(s->vertices, s->faces[face_id + 2]), oo, od, &r, &bs, &bt)) {
					if (list->members == list->room) {
						list->room = list->room ? 2 * list->room : 64;
						list->at = (im_member *) realloc(list->at, list->room * sizeof *list->at);
						if (!list->at)
							abort();
					}
					im_member *m = list->at + list->members++;
					const v3 p = v3_make(o.x + r * d.x, o.y + r * d.y, o.z + r * d.z);
					const float distance = v3_length(v3_sub(p, o));
					m->instance = k;
					m->leaf = triangle_index;
					m->kept = distance < INFINITY;
					m->s = bs;
					m->t = bt;
					m->position = p;
					m->distance = m->kept ? distance : INFINITY;
				}
				++triangle_index;
			}
			++i;
		}
	}
}

/* Rays [0, n): count[i] = the candidates of ray i over all instances, slots i * k .. i * k + k - 1 the first k of them;
 * unused slots: distance +inf, leaf and instance IM_NONE, barycentrics / position / normal 0.  Any output may be NULL. */
void im_multihit(const orc_scene *s, const im_node *top, uint32_t top_count, const float *O, const float *o4, const float *d4, uint32_t n,
                 float max_distance, uint32_t k, uint32_t *count, float *distance, uint32_t *leaf, float *bary, float *pos, float *normal,
                 uint32_t *instance) {
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 64) num_threads(im_threads())
#endif
	for (int64_t i = 0; i < (int64_t) n; ++i) {
		const v3 o = v3_load4(o4, (uint32_t) i), d = v3_load4(d4, (uint32_t) i);
		im_list list = { NULL, 0, 0 };
		/* the top-level walk: a record is entered when its box passes, a leaf record is an instance */
		for (uint32_t at = 0; at < top_count;) {
			float bb[8] = { top[at].lo[0], top[at].lo[1], top[at].lo[2], 0.0f, top[at].hi[0], top[at].hi[1], top[at].hi[2], 0.0f };
			if (!box_hit(bb, o, d, max_distance)) {
				at += top[at].skip;
				continue;
			}
			if (top[at].leaf != IM_NONE)
				im_instance_members(s, top[at].leaf, O + 12u * (size_t) top[at].leaf, o, d, max_distance, &list);
			++at;
		}
		if (list.members)
			qsort(list.at, list.members, sizeof *list.at, im_before);
		if (count)
			count[i] = (uint32_t) list.members;
		for (uint32_t j = 0; j < k; ++j) {
			const size_t slot = (size_t) i * k + j;
			const int used = j < list.members;
			const im_member *m = used ? list.at + j : NULL;
			const int kept = used && m->kept;
			const v3 b = kept ? v3_make(1.0f - m->s - m->t, m->s, m->t) : v3_make(0.0f, 0.0f, 0.0f);
			v3 nrm = v3_make(0.0f, 0.0f, 0.0f);
			if (kept) { /* get_smooth_normal before its normalisation, the inverse's transpose, one normalisation */
				const uint32_t face_id = m->leaf * 3u;
				const uint32_t v0 = s->faces[face_id + 0], v1 = s->faces[face_id + 1], v2 = s->faces[face_id + 2];
				const v3 raw = v3_add(v3_add(v3_scale(v3_load4(s->normals, v0), b.x), v3_scale(v3_load4(s->normals, v1), b.y)),
				                      v3_scale(v3_load4(s->normals, v2), b.z));
				const float *r = O + 12u * (size_t) m->instance;
				nrm = v3_normalize(v3_make((r[0] * raw.x + r[4] * raw.y) + r[8] * raw.z, (r[1] * raw.x + r[5] * raw.y) + r[9] * raw.z,
				                           (r[2] * raw.x + r[6] * raw.y) + r[10] * raw.z));
			}
			if (distance)
				distance[slot] = used ? m->distance : INFINITY;
			if (leaf)
				leaf[slot] = used ? m->leaf : IM_NONE;
			if (instance)
				instance[slot] = used ? m->instance : IM_NONE;
			if (bary) {
				bary[3 * slot + 0] = b.x;
				bary[3 * slot + 1] = b.y;
				bary[3 * slot + 2] = b.z;
			}
			if (pos) {
				pos[3 * slot + 0] = kept ? m->position.x : 0.0f;
				pos[3 * slot + 1] = kept ? m->position.y : 0.0f;
				pos[3 * slot + 2] = kept ? m->position.z : 0.0f;
			}
			if (normal) {
				normal[3 * slot + 0] = nrm.x;
				normal[3 * slot + 1] = nrm.y;
				normal[3 * slot + 2] = nrm.z;
			}
		}
		free(list.at);
	}
}
