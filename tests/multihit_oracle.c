/*
 * multihit_oracle.c -- CPU oracle of the multi-hit ray queries (include/rt_hip_multihit.h).  TEST INFRASTRUCTURE ONLY.
 *
 * The loop of the oracle's own scene_hit (oracle/rt_oracle.c, the restatement of the reference's scene_intersect) with
 * a FRESH record at every reached leaf -- distance = INFINITY, the rest 0, what tri_hit then writes is the member's
 * record --, the accepted leaves sorted by (reported distance, leaf index), the count and the first k of them, and the
 * smooth normal of each as tests/query_oracle.c computes it for the closest hit.
 * Built by tests/multihit_oracle.py with the oracle's flags (-O2 -ffp-contract=off -fno-fast-math).
 */
#include "../oracle/rt_oracle.c"

#include <stdlib.h>

#define MO_NONE 0xFFFFFFFFu
#define MO_MAX_THREADS 16

static int mo_threads(void) {
#ifdef _OPENMP
	const int n = omp_get_max_threads();
	return n < MO_MAX_THREADS ? n : MO_MAX_THREADS;
#else
	return 1;
#endif
}

typedef struct mo_member {
	uint32_t leaf;
	int kept; /* the record was replaced: a computed distance below +inf */
	hit_record rec;
} mo_member;

static int mo_before(const void *pa, const void *pb) {
	const mo_member *a = (const mo_member *) pa, *b = (const mo_member *) pb;
	if (a->rec.distance < b->rec.distance)
		return -1;
	if (a->rec.distance > b->rec.distance)
		return 1;
	return a->leaf < b->leaf ? -1 : (a->leaf > b->leaf ? 1 : 0);
}

/* Rays [0, n): count[i] = the accepted leaves of ray i, slots i * k .. i * k + k - 1 the first k of them; unused slots:
 * distance +inf, leaf MO_NONE, barycentrics / position / normal 0.  Any output may be NULL. */
void mo_multihit(const orc_scene *s, const float *o4, const float *d4, uint32_t n, float max_distance, uint32_t k, uint32_t *count,
                 float *distance, uint32_t *leaf, float *bary, float *pos, float *normal) {
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 256) num_threads(mo_threads())
#endif
	for (int64_t i = 0; i < (int64_t) n; ++i) {
		const v3 o = v3_load4(o4, (uint32_t) i), d = v3_load4(d4, (uint32_t) i);
		mo_member *found = NULL;
		size_t members = 0, room = 0;
		/* scene_hit's loop */
		uint32_t triangle_index = 0;
		const uint32_t nodes = s->nodes[0];
		for (uint32_t at = 0; at < nodes;) {
			const uint32_t node_count = s->nodes[at];
			if (!box_hit(s->aabbs + 8u * (size_t) at, o, d, max_distance)) {
				triangle_index += (node_count + 1) >> 1;
				at += node_count;
			} else {
				if (node_count == 1) {
					const uint32_t face_id = triangle_index * 3;
					hit_record rec;
					memset(&rec, 0, sizeof rec);
					rec.distance = INFINITY;
					if (tri_hit(v3_load4(s->vertices, s->faces[face_id + 0]), v3_load4(s->vertices, s->faces[face_id + 1]),
					            v3_load4(s->vertices, s->faces[face_id + 2]), face_id, o, d, &rec)) {
						if (members == room) {
							room = room ? 2 * room : 64;
							found = (mo_member *) realloc(found, room * sizeof *found);
							if (!found)
								abort();
						}
						found[members].leaf = triangle_index;
						found[members].kept = rec.distance < INFINITY;
						found[members].rec = rec;
						++members;
					}
					++triangle_index;
				}
				++at;
			}
		}
		qsort(found, members, sizeof *found, mo_before);
		if (count)
			count[i] = (uint32_t) members;
		for (uint32_t j = 0; j < k; ++j) {
			const size_t slot = (size_t) i * k + j;
			const int used = j < members;
			hit_record rec;
			memset(&rec, 0, sizeof rec);
			rec.distance = INFINITY;
			v3 nrm = v3_make(0.0f, 0.0f, 0.0f);
			if (used && found[j].kept) { /* get_smooth_normal, as qo_closest */
				rec = found[j].rec;
				const uint32_t v0 = s->faces[rec.face_id + 0], v1 = s->faces[rec.face_id + 1], v2 = s->faces[rec.face_id + 2];
				nrm = v3_normalize(v3_add(v3_add(v3_scale(v3_load4(s->normals, v0), rec.barycentric.x),
				                                 v3_scale(v3_load4(s->normals, v1), rec.barycentric.y)),
				                          v3_scale(v3_load4(s->normals, v2), rec.barycentric.z)));
			}
			if (distance)
				distance[slot] = rec.distance;
			if (leaf)
				leaf[slot] = used ? found[j].leaf : MO_NONE;
			if (bary) {
				bary[3 * slot + 0] = rec.barycentric.x;
				bary[3 * slot + 1] = rec.barycentric.y;
				bary[3 * slot + 2] = rec.barycentric.z;
			}
			if (pos) {
				pos[3 * slot + 0] = rec.position.x;
				pos[3 * slot + 1] = rec.position.y;
				pos[3 * slot + 2] = rec.position.z;
			}
			if (normal) {
				normal[3 * slot + 0] = nrm.x;
				normal[3 * slot + 1] = nrm.y;
				normal[3 * slot + 2] = nrm.z;
			}
		}
		free(found);
	}
}
