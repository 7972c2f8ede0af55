/* rt_hip_segment.h -- segment queries on an uploaded scene: line of sight between points the caller supplies, the first
 * blocker of a segment, and visibility masks of many points against many targets.
 *
 * Beside rt_hip_query.h.  A ray query cannot say whether point A sees point B: its max_distance "only culls BOXES", its
 * direction is not normalised, and it has no lower bound, so a ray that starts on a surface finds that surface.  These
 * entry points answer the question itself, under the arithmetic contract (every operation rounded on its own,
 * in the reference's order), on the scene a render host holds after rt_upload / rt_upload_scene, rt_update_vertices or
 * rt_build_scene.
 *
 * A segment is a pair of points (a, b).  Its ray is o = a, d = b - a: each component of d is one binary32 subtraction,
 * nothing is normalised.  A call has two floats t_lo, t_hi, fractions of the segment (0 is a, 1 is b).  The BLOCKERS of a
 * segment are the leaves L that meet all three conditions:
 *   1. every box from the root to L, its own included, passes the reference's aabb_intersect (src/intersect_kernel.cl:21-61)
 *      for (o, d) with max_distance = t_hi.  That test culls in ray parameters (t_min < max_distance): with d = b - a it
 *      says "this box begins before the far end of the interval";
 *   2. triangle_intersect (:65-114) accepts L's triangle for (o, d);
 *   3. its plane parameter r = a / b (:79) satisfies r > t_lo and r < t_hi, compared in binary32.  An r that is NaN
 *      blocks nothing.
 *
 * Occluded form: occluded[i] = 1 iff segment i has a blocker.
 * Closest form: the record of rt_hit_arrays (rt_hip_query.h) for the blocker with the minimum of (distance, leaf), where
 * distance is length(ip - o) as the reference computes it (NOT r: for a segment of length l it is about r l) and equal
 * distances go to the lowest leaf.  `hit` is 1 iff there is a blocker.  Without a blocker: distance +inf, leaf 0xFFFFFFFF,
 * barycentrics, position and normal 0.  For a blocker whose distance is +inf or NaN the rule is rt_hip_query.h's: `hit` is
 * 1 and the record keeps its entry values (leaf 0, barycentrics and position 0, distance +inf).
 *
 * Every float input is legal.  A segment of no length, an endpoint with a NaN or infinite coordinate, and a t_lo or t_hi
 * that is NaN, negative or infinite all get the rules' own answer, and that answer is "nothing blocks" for: a segment of no
 * length (a zero d makes all three reciprocals infinite, so a box whose slab the origin lies in passes on that axis, and
 * every triangle's b = n . d is 0, below triangle_intersect's 1e-6), a NaN endpoint coordinate (r is NaN), an infinite one
 * (r is NaN, or the root's t_max is 0), a t_lo or t_hi that is NaN, t_hi <= 0, t_lo = +inf, and t_lo >= t_hi.  A negative
 * t_lo is no lower bound beyond the reference's own r >= 0; t_hi = +inf is a ray: no far end.
 *
 * Relation to the ray queries: with t_lo < 0 and t_hi = +inf, for a segment whose blockers all have a finite r, `occluded`
 * equals rt_trace_occluded of (a, b - a) with max_distance = +inf; and where that ray's closest hit has a distance below
 * +inf, the closest form equals rt_trace_closest word for word.
 *
 * The many-to-many form, rt_visibility_masks: segment (i, j) runs from points[i] to targets[j].  out->mask is
 * uint32[np][words] with words = (nt + 31) / 32: bit j & 31 of word j >> 5 of row i is set iff segment (i, j) is occluded;
 * padding bits are 0.  out->count[np] is the row's popcount: the number of targets point i does NOT see.  Either pointer
 * may be NULL (both, or a NULL `out`: nothing is computed).  np * nt <= RT_QUERY_MAX_RAYS.  No array of np * nt rays exists
 * anywhere, on the host or the device: a lane makes its ray from the two point arrays.
 *
 * Coherence: the pair forms order the segments by the ray queries' key of (a, b - a) from RT_QUERY_SORT_MIN segments on,
 * the mask form orders the POINTS by position from RT_QUERY_SORT_MIN points on, unless RT_QUERY_NO_SORT is given.  Results
 * go to the caller's indices; not a bit depends on the order.
 *
 * Leaf indices, what a query leaves alone (the frame's buffers, graph and counters), scratch of the host's own, streams,
 * serialisation per host and rt_last_query_ms are as in rt_hip_query.h.  Not for the hosts of a frame ring: RT_E_STATE.
 *
 * Errors: RT_E_STATE before an upload; RT_E_INVALID for null point arrays with n > 0 (np > 0 and nt > 0), device point
 * arrays not 16-byte aligned, device float / uint32 outputs not 4-byte aligned, n or np * nt > RT_QUERY_MAX_RAYS.  n == 0,
 * np == 0 or nt == 0 succeeds and launches nothing.
 */
#ifndef RT_HIP_SEGMENT_H
#define RT_HIP_SEGMENT_H

#include "rt_hip_query.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rt_visibility_arrays { /* either pointer may be NULL: that output is not written */
	uint32_t *mask;  /* [np][(nt + 31) / 32] bit j of row i: segment (i, j) is occluded */
	uint32_t *count; /* [np] occluded targets of point i */
} rt_visibility_arrays;

/* Host memory, blocking.  from4 / to4 / points4 / targets4: float4[], .w ignored.  `out` may be NULL (nothing is written). */
int rt_segments_occluded(rt_host *h, const float *from4, const float *to4, uint32_t n, float t_lo, float t_hi, uint32_t flags,
                         uint8_t *occluded);
int rt_segments_closest(rt_host *h, const float *from4, const float *to4, uint32_t n, float t_lo, float t_hi, uint32_t flags,
                        const rt_hit_arrays *out);
int rt_visibility_masks(rt_host *h, const float *points4, uint32_t np, const float *targets4, uint32_t nt, float t_lo, float t_hi,
                        uint32_t flags, const rt_visibility_arrays *out);

/* Device memory on the host's device, enqueued on `hip_stream` (NULL: the host's stream); returns without waiting.  The
 * points must stay unchanged until the query has run.  `out` points to host memory that holds device pointers and is read
 * during the call.  The library zeroes the mask rows on the stream. */
int rt_segments_occluded_device(rt_host *h, const float *from4, const float *to4, uint32_t n, float t_lo, float t_hi, uint32_t flags,
                                uint8_t *occluded, void *hip_stream);
int rt_segments_closest_device(rt_host *h, const float *from4, const float *to4, uint32_t n, float t_lo, float t_hi, uint32_t flags,
                               const rt_hit_arrays *out, void *hip_stream);
int rt_visibility_masks_device(rt_host *h, const float *points4, uint32_t np, const float *targets4, uint32_t nt, float t_lo,
                               float t_hi, uint32_t flags, const rt_visibility_arrays *out, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
