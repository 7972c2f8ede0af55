/* rt_hip_instance_segments.h -- instanced segment queries: line of sight between world-space points with every posed copy
 * of the uploaded scene in the way, the first blocker of a segment, and visibility masks of many points against many
 * targets.
 *
 * Beside rt_hip_segment.h and rt_hip_instances.h, and defined by their rules: the segment, its ray and its interval are
 * rt_hip_segment.h's, the instance set, its inverses O_k, its top-level tree and the object ray are rt_hip_instances.h's.
 * Nothing is derived again here.  The arithmetic contract holds (every operation rounded on its own in binary32,
 * in the order written).
 *
 * Ray and interval.  A segment is a pair of WORLD-space points (a, b).  Its world ray is o = a, d = b - a: one binary32
 * subtraction per component, nothing normalised.  A call has two floats t_lo, t_hi, fractions of the segment (0 is a, 1 is
 * b), as in rt_hip_segment.h.  An affine map keeps ray parameters, so the interval means the same in every instance's object
 * space as in the world.
 *
 * Entering an instance.  Instance k is ENTERED iff every top-level box from the root to k's leaf, its own included, passes
 * the reference's aabb_intersect (src/intersect_kernel.cl:21-61) for (o, d) with max_distance = t_hi.
 *
 * Blockers.  The object ray (o', d') of an entered instance is made from the rows of O_k exactly as rt_hip_instances.h
 * states it ("its object ray"): the same products, the same sums, the same order.  The BLOCKERS of the segment in instance
 * k are the scene leaves L that meet all three conditions:
 *   1. every scene box from the root to L, its own included, passes aabb_intersect for (o', d') with max_distance = t_hi;
 *   2. triangle_intersect (:65-114) accepts L's triangle for (o', d');
 *   3. that object-space test's plane parameter r = a / b (:79) satisfies r > t_lo and r < t_hi, compared in binary32.  An r
 *      that is NaN blocks nothing.
 *
 * Occluded form: occluded[i] = 1 iff some entered instance has a blocker of segment i.
 *
 * Closest form: the record of rt_instance_hit_arrays (rt_hip_instances.h).  A blocker's position is o + r d with the WORLD
 * ray, per component o.x + r * d.x; its distance is length(position - o) as the reference computes length (NOT r: for a
 * segment of length l it is about r l); its barycentrics are (1 - s - t, s, t) of the object-space test.  The result is the
 * blocker with the minimum of (distance, instance, leaf): a strictly smaller distance wins, and among equal distances below
 * +inf the lower (instance, leaf) pair.  `hit` is 1 iff there is a blocker.  The normal follows the instanced rule: the raw
 * weighted sum of the leaf's three vertex normals with the returned barycentrics, w = transpose(O) raw, ONE normalisation.
 * No blocker: `hit` 0, instance and leaf 0xFFFFFFFF, distance +inf, the rest 0.  A blocker but none with a distance below
 * +inf: `hit` 1 and the record keeps its entry values -- instance 0, leaf 0, distance +inf, the rest 0 (rt_hip_instances.h).
 *
 * Mask form, rt_instances_visibility_masks: it follows rt_visibility_masks.  Segment (i, j) runs from points[i] to
 * targets[j].  out->mask is uint32[np][words] with words = (nt + 31) / 32: bit j & 31 of word j >> 5 of row i is set iff
 * segment (i, j) is occluded; padding bits are 0.  out->count[np] is the row's popcount: the number of targets point i does
 * NOT see.  Either pointer may be NULL (both, or a NULL `out`: nothing is computed).  np * nt <= RT_QUERY_MAX_RAYS.  No array
 * of np * nt rays exists anywhere, on the host or the device: a lane makes its ray from the two point arrays.
 *
 * Odd inputs.  Every float input is legal and gets the rules' own answer.  Which inputs give "nothing blocks" for EVERY
 * transform the setter accepts follows from two facts.  A blocker needs a plane parameter r with r > t_lo and r < t_hi, and
 * both are false for a NaN.  Every entry of O is finite (rt_set_instances refuses the others), so the product of an entry of
 * O with a NaN is NaN and with an infinity is an infinity, or NaN where the entry is 0: never a finite number; and a sum
 * with a term that is not finite is not finite (inf + x = inf, inf - inf = NaN, NaN + x = NaN).
 *   - A t_lo or t_hi that is NaN: no r passes the comparison with it.  t_lo >= t_hi, and so t_lo = +inf: no r is above the
 *     one and below the other.  t_hi <= 0: triangle_intersect rejects r < 0, and no r >= 0 is below t_hi.  A negative t_lo
 *     is no lower bound beyond the reference's own r >= 0; t_hi = +inf is a ray: no far end.
 *   - A segment of no length, a == b with finite coordinates: d is a zero in every component, every product of an entry of O
 *     with it is a zero, every sum of zeros is a zero, so d' is a zero in every component.  A triangle's b = n . d' is then a
 *     zero, below triangle_intersect's 1e-6: rejected (or, for a normal that is not finite, NaN, and so is r).
 *   - A NaN endpoint coordinate, in column c of a or of b: d.c = b.c - a.c is NaN.  Component k of d' sums three products,
 *     one of them O[k][c] * NaN = NaN -- also where O[k][c] is 0 --, so EVERY component of d' is NaN, whatever the boxes on
 *     the way answered.  b = n . d' is NaN, r = a / b is NaN, and the interval rejects it.
 *   - An infinite coordinate, column c, of a.  d.c = b.c - a.c is the opposite infinity, or NaN where b.c is the same
 *     infinity (the case above).  o.c and d.c are infinite, so by the second fact every component of o' and of d' holds a
 *     product with them and is not finite; so is every component of o' - ta, every product of the plane test's two dot
 *     products, and both sums: the test's numerator and denominator are each an infinity or NaN, and their quotient r is NaN.
 *     Nothing blocks.
 *   - An infinite coordinate, column c, of b alone (the end a finite, no NaN at either end).  o is finite, d.c is infinite,
 *     and every component of d' is not finite, so the plane test's denominator is an infinity or NaN and r is a zero (a
 *     finite numerator) or NaN: nothing blocks for every t_lo >= 0.  For t_lo < 0 it hinges on the top-level root's slab
 *     test, as the plain header's remark about the root's t_max does: 1 / d.c is a zero, and where the root's two differences lo.c - a.c and hi.c - a.c are finite both of axis
 *     c's parameters are zeros, the root's t_max -- a minimum over the axes that returns the other operand for a NaN -- is
 *     at most 0, its `t_max > 0` fails, no instance is entered and nothing blocks.  Where one of the two differences is
 *     not finite (a top-level root box of (-inf, +inf), or a difference that overflows) the axis' parameters are NaN and
 *     decide nothing; this header says nothing for that remainder (t_lo < 0 only), and the tests hold the library to the
 *     oracle there.
 *
 * Relations.
 *   - Identity: with ONE instance whose transform is the identity, for segments whose a and b - a are finite and hold no -0,
 *     `occluded` equals rt_segments_occluded's, and where rt_segments_closest's blocker has a distance below +inf every field
 *     equals it word for word, with instance 0.  (1 * x + 0 * y turns a -0 into +0: rt_hip_instances.h has the reason for
 *     the exclusion.)
 *   - Ray queries: with t_lo < 0 and t_hi = +inf, for a segment whose candidates all have a finite r, `occluded` equals
 *     rt_trace_instances_occluded of (a, b - a) with max_distance = +inf; and where that ray's closest hit has a distance
 *     below +inf, the closest form equals rt_trace_instances_closest word for word.
 *   - Unchanged families: rt_segments_occluded, rt_segments_closest and rt_visibility_masks keep ignoring the set, bit for
 *     bit, before and after these calls.
 *
 * Coherence: the pair forms order the segments by the ray queries' key of (a, b - a), the mask form orders the POINTS by
 * position; both keys are quantised over the top-level root box, as the instanced ray queries' are, from RT_QUERY_SORT_MIN
 * segments (points) on, unless RT_QUERY_NO_SORT is given.  Results go to the caller's indices; not a bit depends on the
 * order.
 *
 * Errors and lifetime: RT_E_STATE before an upload, with no instance set, and on the hosts of a frame ring; RT_E_INVALID as
 * in rt_hip_segment.h (null point arrays with n > 0 -- np > 0 and nt > 0 --, device point arrays not 16-byte aligned, device
 * float / uint32 outputs not 4-byte aligned, n or np * nt > RT_QUERY_MAX_RAYS).  n == 0, np == 0 or nt == 0 succeeds and
 * launches nothing (on a host in a state to be asked: the state is checked first).  The set persists across
 * rt_update_vertices, rt_build_scene and a new upload; its boxes and tree are
 * made again from the new root box before the next of these calls.  rt_last_query_ms covers these calls; frames, graphs
 * and counters are left alone; scratch, streams and serialisation per host are as in rt_hip_query.h.
 */
#ifndef RT_HIP_INSTANCE_SEGMENTS_H
#define RT_HIP_INSTANCE_SEGMENTS_H

#include "rt_hip_instances.h"
#include "rt_hip_segment.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host memory, blocking.  from4 / to4 / points4 / targets4: float4[], .w ignored.  `out` may be NULL (nothing is written). */
int rt_instances_segments_occluded(rt_host *h, const float *from4, const float *to4, uint32_t n, float t_lo, float t_hi, uint32_t flags,
                                   uint8_t *occluded);
int rt_instances_segments_closest(rt_host *h, const float *from4, const float *to4, uint32_t n, float t_lo, float t_hi, uint32_t flags,
                                  const rt_instance_hit_arrays *out);
int rt_instances_visibility_masks(rt_host *h, const float *points4, uint32_t np, const float *targets4, uint32_t nt, float t_lo,
                                  float t_hi, uint32_t flags, const rt_visibility_arrays *out);

/* Device memory on the host's device, enqueued on `hip_stream` (NULL: the host's stream); returns without waiting.  The
 * points must stay unchanged until the query has run.  `out` points to host memory that holds device pointers and is read
 * during the call.  The library zeroes the mask rows on the stream. */
int rt_instances_segments_occluded_device(rt_host *h, const float *from4, const float *to4, uint32_t n, float t_lo, float t_hi,
                                          uint32_t flags, uint8_t *occluded, void *hip_stream);
int rt_instances_segments_closest_device(rt_host *h, const float *from4, const float *to4, uint32_t n, float t_lo, float t_hi,
                                         uint32_t flags, const rt_instance_hit_arrays *out, void *hip_stream);
int rt_instances_visibility_masks_device(rt_host *h, const float *points4, uint32_t np, const float *targets4, uint32_t nt, float t_lo,
                                         float t_hi, uint32_t flags, const rt_visibility_arrays *out, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
