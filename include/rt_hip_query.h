/* rt_hip_query.h -- ray queries on an uploaded scene: closest hit and occlusion for rays the caller supplies.
 *
 * Beside the seam (rt_hip.h), like rt_hip_ring.h and rt_hip_debug.h: the reference only casts the rays it makes itself
 * (the camera at (0, 0, 2) and the ambient-occlusion rays around its hits, src/intersect_kernel.cl:278-310).  These
 * entry points answer, for any rays, what the reference's scene_intersect (:184-213) answers for them -- bit for bit
 * under the arithmetic contract -- on the scene a render host holds after rt_upload / rt_upload_scene.
 *
 * Per ray i (origin o_i, direction d_i, the call's max_distance), closest hit returns what
 *     scene_intersect(nodes, aabbs, faces, vertices, normals, o_i, d_i, &isect, max_distance)
 * returns with isect.distance = INFINITY and every other field 0 on entry: the boolean, and the record of the nearest
 * accepted triangle -- leaf index (face_id / 3), barycentrics (1 - s - t, s, t), point o + r d, distance length(p - o) --
 * plus the smooth normal get_smooth_normal (:118-127) computes for it.  The reference's rules hold as they are:
 *   - max_distance only culls BOXES (t_min < max_distance); a triangle beyond it is returned if its box begins before it;
 *   - directions are not normalised;
 *   - among equal nearest distances the lowest leaf index wins;
 *   - every float input is legal (zero / tiny / huge components, far origins, NaN or inf anywhere, a max_distance of inf,
 *     0, < 0 or NaN): such a ray gets the reference's answer, usually "no hit".
 * Where a triangle is accepted but none replaces the record (a distance of +inf or NaN), `hit` is 1 with the record's
 * entry values: leaf 0, barycentrics and position 0, distance +inf.  Without a hit: distance +inf, leaf 0xFFFFFFFF,
 * barycentrics, position and normal 0.
 * Occlusion returns the same boolean as closest hit for the same ray and max_distance (it stops at the first accepted
 * triangle).
 *
 * Leaf indices count the leaves of the uploaded tree in its order.  For a scene built by rt_scene_build_bvh, the face
 * of the file that leaf L holds is rt_scene_triangles(s)[L] (rt_hip.h); for arrays given to rt_upload, it is the
 * triangle at faces[3 L .. 3 L + 2].
 *
 * A query changes nothing a frame produces or reports: it reads the scene's arrays, uses scratch buffers of its own
 * (grown on demand, freed by rt_destroy) and leaves the frame's buffers, captured graph and counters (rt_get_stats)
 * alone.  Queries go on the host's stream (rt_set_stream) unless a stream is given; a frame in flight on that stream is
 * not disturbed.  Not for the hosts of a frame ring (rt_ring_host): RT_E_STATE.
 *
 * Errors: RT_E_STATE before an upload; RT_E_INVALID for null rays with n > 0, device ray pointers not 16-byte aligned,
 * device float / uint32 outputs not 4-byte aligned, n > RT_QUERY_MAX_RAYS.  n == 0 succeeds and launches nothing.
 */
#ifndef RT_HIP_QUERY_H
#define RT_HIP_QUERY_H

#include "rt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_QUERY_MAX_RAYS (1u << 27) /* rays per call */

/* flags */
#define RT_QUERY_NO_SORT 1u /* the rays are coherent already (neighbours in the arrays go the same way): cast them in
                               their own order.  Batches below RT_QUERY_SORT_MIN rays are never sorted. */
#define RT_QUERY_SORT_MIN 16384u

typedef struct rt_hit_arrays { /* any pointer may be NULL: that output is not written */
	uint8_t *hit;          /* [n] 1 = hit */
	float *distance;       /* [n] +inf when no hit */
	uint32_t *leaf;        /* [n] reference face_id / 3 (leaf order); 0xFFFFFFFF when no hit */
	float *barycentric;    /* [3n] (1-s-t, s, t) */
	float *position;       /* [3n] */
	float *normal;         /* [3n] smooth normal (get_smooth_normal) */
} rt_hit_arrays;

/* Host memory, blocking.  origins4 / directions4: float4[n], .w ignored.  `out` may be NULL (nothing is written). */
int rt_trace_closest(rt_host *h, const float *origins4, const float *directions4, uint32_t n, float max_distance,
                     uint32_t flags, const rt_hit_arrays *out);
int rt_trace_occluded(rt_host *h, const float *origins4, const float *directions4, uint32_t n, float max_distance,
                      uint32_t flags, uint8_t *occluded);

/* Device memory on the host's device, enqueued on `hip_stream` (NULL: the host's stream); returns without waiting.  The
 * rays must stay unchanged until the query has run (they are read twice when sorted).  `out` points to host memory that
 * holds device pointers and is read during the call. */
int rt_trace_closest_device(rt_host *h, const float *origins4, const float *directions4, uint32_t n, float max_distance,
                            uint32_t flags, const rt_hit_arrays *out, void *hip_stream);
int rt_trace_occluded_device(rt_host *h, const float *origins4, const float *directions4, uint32_t n, float max_distance,
                             uint32_t flags, uint8_t *occluded, void *hip_stream);

/* HIP-event time in ms of the last query's kernels (sort + walk; waits for that query to end); 0 before the first.  The
 * last query of either kind: a ray query of this header or an ambient-occlusion query (rt_hip_ao.h: sort + walk + the
 * finishing kernel). */
float rt_last_query_ms(const rt_host *h);

#ifdef __cplusplus
}
#endif
#endif
