/* rt_hip_instance_multihit.h -- instanced multi-hit ray queries: how many surfaces a world-space ray crosses among the posed
 * copies of the uploaded scene, and the first k of them in order.
 *
 * The composition of rt_hip_instances.h (the set, the top-level tree, the object ray, a candidate's record) and
 * rt_hip_multihit.h (the accepted set, its count, its first k members): thickness, depth peeling and entry / exit pairs
 * through several copies of a posed assembly, without merging vertices and rebuilding -- and without re-casting
 * rt_trace_instances_closest from behind each hit, which skips or repeats layers under the reference's tolerant triangle
 * test (rt_hip_multihit.h says why).  Bit for bit under the arithmetic contract; every float input is legal.
 *
 * Accepted set.  For ray (o, d) and the call's max_distance, A is the set of pairs (instance k, leaf L) that are CANDIDATES
 * under rt_hip_instances.h:
 *   - k is ENTERED: every top-level box from the root to k's leaf passes the reference's aabb_intersect
 *     (src/intersect_kernel.cl:21-61) for (o, d, max_distance);
 *   - the object ray (o', d') is formed from the rows (m0 m1 m2 m3) of O_k with that header's operations:
 *     o'.x = ((m0 o.x + m1 o.y) + m2 o.z) + m3, d'.x = (m0 d.x + m1 d.y) + m2 d.z, y and z from rows 1 and 2;
 *   - L is accepted by the reference's scene_intersect walk (:184-213) of the scene's own tree for (o', d', max_distance):
 *     every box from the root to L, its own included, passes aabb_intersect, and triangle_intersect (:65-114) returns true
 *     for L's triangle.  That walk prunes nothing on a distance, so A is fixed by the scene arrays, the set's tree and
 *     inverses, the ray and max_distance, whatever the order of the walk.
 * Record of a member.  That header's: with the plane parameter r = a / b (:79) and (s, t) of the object-space test,
 * position = o + r d in WORLD space, per component o.x + r * d.x; distance = length(position - o) as the reference computes
 * length; barycentrics (1 - s - t, s, t); leaf L; instance k.  Normal: with those barycentrics raw = (n0 b0 + n1 b1) + n2 b2,
 * w = transpose(O_k) raw with w.x = (O00 raw.x + O10 raw.y) + O20 raw.z and so on, and ONE normalisation of w.
 * A member whose computed distance is not below +inf (+inf or NaN) is still counted, and it is reported with distance +inf,
 * its OWN instance and leaf, and barycentrics, position and normal 0 (the rule of rt_hip_multihit.h).
 *
 *   count[i] = |A|: exact, over all instances, not limited by k.
 *   Slots 0 .. min(k, |A|) - 1 of ray i hold the first members of A by (reported distance, instance, leaf) ascending --
 *   reported distances are never NaN, so this is a total order.  The remaining slots are unused: distance +inf, leaf and
 *   instance 0xFFFFFFFF, barycentrics, position and normal 0.
 *   k ranges from 0 to RT_MULTIHIT_MAX_K.  With k == 0 only `count` may be non-NULL.  n * max(k, 1) <= RT_QUERY_MAX_RAYS.
 *
 * It follows that
 *   - count[i] > 0 is rt_trace_instances_occluded's flag for the same ray and max_distance;
 *   - where rt_trace_instances_closest returns a distance below +inf, slot 0 equals that record word for word -- distance,
 *     leaf, barycentrics, position, normal and instance;
 *   - a call with k returns the first k slots of the call with RT_MULTIHIT_MAX_K;
 *   - with ONE instance whose transform is the identity, for rays whose six components are finite and hold no -0, count
 *     equals rt_trace_multihit's and every slot equals its slot word for word, with instance 0 in the used slots
 *     (rt_hip_instances.h says why -0 is excluded).
 * As there, max_distance only culls BOXES and means the same in both spaces, directions are not normalised, and leaf
 * indices count the leaves of the uploaded tree in its order.
 *
 * Sorting, streams and state are the union of the two parents': the rays are ordered by the ray queries' coherence key from
 * RT_QUERY_SORT_MIN rays on unless RT_QUERY_NO_SORT is passed, origins quantised over the top-level root box, and not a bit
 * depends on the order; the query goes on the host's stream unless one is given; it uses scratch of the host's own (a
 * ray's list is 12 bytes per slot: distance, instance, leaf) and leaves frames, their captured graph and rt_get_stats
 * alone; rt_last_query_ms reports this query too (sort + walk + the pass that writes the slots' records).  The tree is made
 * again first after rt_update_vertices, rt_build_scene and a new upload.  Every plain entry point still ignores the set.
 *
 * Errors: RT_E_STATE before an upload, with no instances set, on the hosts of a frame ring; RT_E_INVALID as
 * rt_hip_multihit.h -- null rays with n > 0, device ray pointers not 16-byte aligned, device outputs (`instance` among
 * them) not 4-byte aligned, k > RT_MULTIHIT_MAX_K, k == 0 with any slot array (`instance` among them) non-NULL,
 * n * max(k, 1) > RT_QUERY_MAX_RAYS.  n == 0 succeeds and launches nothing.
 */
#ifndef RT_HIP_INSTANCE_MULTIHIT_H
#define RT_HIP_INSTANCE_MULTIHIT_H

#include "rt_hip_instances.h"
#include "rt_hip_multihit.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rt_instance_multihit_arrays { /* any pointer may be NULL: that output is not written */
	rt_multihit_arrays slots;
	uint32_t *instance; /* [n*k]  slot j of ray i at i*k + j; 0xFFFFFFFF in unused slots */
} rt_instance_multihit_arrays;

/* Host memory, blocking.  origins4 / directions4: float4[n], world space, .w ignored.  `out` may be NULL (nothing is written). */
int rt_trace_instances_multihit(rt_host *h, const float *origins4, const float *directions4, uint32_t n, float max_distance,
                                uint32_t k, uint32_t flags, const rt_instance_multihit_arrays *out);

/* Device memory on the host's device, enqueued on `hip_stream` (NULL: the host's stream); returns without waiting.  The
 * rays must stay unchanged until the query has run.  `out` points to host memory that holds device pointers and is read
 * during the call. */
int rt_trace_instances_multihit_device(rt_host *h, const float *origins4, const float *directions4, uint32_t n, float max_distance,
                                       uint32_t k, uint32_t flags, const rt_instance_multihit_arrays *out, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
