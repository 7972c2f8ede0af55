/* rt_hip_multihit.h -- multi-hit ray queries on an uploaded scene: how many triangles a ray crosses, and the first k of
 * them in order.
 *
 * Beside rt_hip_query.h, whose entry points answer "is there a hit" and "the nearest hit".  These answer everything
 * the reference's walk accepts along a ray: the number of surfaces, the layers behind the nearest one, entry / exit
 * pairs -- without re-casting from behind each hit with an epsilon, which against the reference's tolerant triangle
 * test (+-1e-5 in the barycentrics: both neighbours accept a shared edge) skips or repeats layers.
 *
 * The reference's scene_intersect (src/intersect_kernel.cl:184-213) does not prune on the running nearest distance, so
 * what it accepts for a ray is a set that the scene arrays, the ray and max_distance fix, whatever the order of the
 * walk.  Bit for bit under the arithmetic contract, with the exact form of the walk: every float input is
 * legal, as in rt_hip_query.h.
 *
 * Accepted set.  Per ray i, A is the set of leaves L such that every box from the root to L, its own included, passes
 * aabb_intersect (:21-61) with the call's max_distance, and triangle_intersect (:65-114) returns true for L's triangle.
 * Record of a member: what triangle_intersect writes into a record that has distance = INFINITY and all other fields 0
 * on entry.  A member whose computed distance is not below +inf (+inf or NaN) does not replace that record: it is still
 * counted, and it is reported with distance +inf, its OWN leaf index, and barycentrics, position and normal 0.
 *
 *   count[i] = |A|: exact, not limited by k.
 *   Slots 0 .. min(k, |A|) - 1 of ray i hold the first members of A by (reported distance ascending, leaf index
 *   ascending) -- reported distances are never NaN, so this is a total order.  The remaining slots are unused: distance
 *   +inf, leaf 0xFFFFFFFF, barycentrics, position and normal 0.
 *   k ranges from 0 to RT_MULTIHIT_MAX_K.  With k == 0 only `count` may be non-NULL.
 *
 * It follows that count[i] > 0 is rt_trace_occluded's answer for the same ray and max_distance, and that where
 * rt_trace_closest returns a hit with distance < +inf, slot 0 equals that hit's distance, leaf, barycentrics, position
 * and normal word for word.  As there, max_distance only culls BOXES, directions are not normalised, and leaf indices
 * count the leaves of the uploaded tree in its order.
 *
 * Sorting, streams and state are those of rt_hip_query.h: the rays are ordered by a coherence key from
 * RT_QUERY_SORT_MIN rays on unless RT_QUERY_NO_SORT is passed, and the results do not depend on the order; the query
 * goes on the host's stream unless one is given; it uses scratch of its own (grown on demand, freed by rt_destroy) and
 * leaves frames, their captured graph and rt_get_stats alone; rt_last_query_ms reports this query too (sort + walk +
 * the pass that writes the slots' records).  Not for the hosts of a frame ring (rt_ring_host): RT_E_STATE.
 *
 * Errors: RT_E_STATE before an upload; RT_E_INVALID for null rays with n > 0, device ray pointers not 16-byte aligned,
 * device outputs not 4-byte aligned, k > RT_MULTIHIT_MAX_K, k == 0 with any slot array non-NULL,
 * n * max(k, 1) > RT_QUERY_MAX_RAYS.  n == 0 succeeds and launches nothing.
 */
#ifndef RT_HIP_MULTIHIT_H
#define RT_HIP_MULTIHIT_H

#include "rt_hip.h"
#include "rt_hip_query.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_MULTIHIT_MAX_K 16u /* slots per ray: the walk keeps a ray's list in on-chip memory, 256 rays x 16 slots x 8 B */

typedef struct rt_multihit_arrays { /* any pointer may be NULL: that output is not written */
	uint32_t *count;       /* [n]      accepted triangles of the ray: all of them, not capped at k */
	float *distance;       /* [n*k]    slot j of ray i at i*k + j; +inf in unused slots */
	uint32_t *leaf;        /* [n*k]    0xFFFFFFFF in unused slots */
	float *barycentric;    /* [3*n*k]  (1-s-t, s, t); 0 in unused slots */
	float *position;       /* [3*n*k]  0 in unused slots */
	float *normal;         /* [3*n*k]  get_smooth_normal of the slot's record; 0 in unused slots */
} rt_multihit_arrays;

/* Host memory, blocking.  origins4 / directions4: float4[n], .w ignored.  `out` may be NULL (nothing is written). */
int rt_trace_multihit(rt_host *h, const float *origins4, const float *directions4, uint32_t n, float max_distance, uint32_t k,
                      uint32_t flags, const rt_multihit_arrays *out);

/* Device memory on the host's device, enqueued on `hip_stream` (NULL: the host's stream); returns without waiting.  The
 * rays must stay unchanged until the query has run.  `out` points to host memory that holds device pointers and is read
 * during the call. */
int rt_trace_multihit_device(rt_host *h, const float *origins4, const float *directions4, uint32_t n, float max_distance,
                             uint32_t k, uint32_t flags, const rt_multihit_arrays *out, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
