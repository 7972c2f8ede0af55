/* rt_hip_instance_nearest.h -- instanced closest-point queries: for world-space points the caller supplies, the nearest point
 * of the surface among the posed copies of the uploaded scene, how far away it is, and which copy it belongs to.
 *
 * Beside rt_hip_nearest.h (the plain query, whose per-leaf routine this one uses unchanged) and rt_hip_instances.h (the
 * instance set: rt_set_instances, its transforms W = world_from_object, the inverses O, the top-level tree).  A ray's
 * parameter survives an affine map, so the instanced ray queries measure in a copy's object space; a distance does not --
 * a copy that is scaled non-uniformly or sheared keeps none --, so this query measures in WORLD space, against each copy's
 * triangles as the map places them.
 *
 * Arithmetic: IEEE binary32, every operation rounded on its own (no contraction), in the order written
 * (csrc/instance_nearest.h and csrc/nearest_point.h are this text as code, compiled by the kernel and the tests' oracle alike).
 *
 * Candidates.  For a point q and the call's max_distance the candidates are ALL pairs (instance k, leaf L) of the host's
 * set and the uploaded scene.
 *
 * The world triangle of a pair is formed from what the device holds for L -- ta, u = tb - ta, v = tc - ta of rt_hip_nearest.h
 * -- and the rows (w0 w1 w2 w3) of world_from_object of k AS THE CALLER GAVE IT (not from the inverse):
 *     ta'.x = ((w0 ta.x + w1 ta.y) + w2 ta.z) + w3        u'.x = (w0 u.x + w1 u.y) + w2 u.z        v'.x likewise
 * y and z from rows 1 and 2;
 *     uu' = dot(u', u')    uv' = dot(u', v')    vv' = dot(v', v')    dot(a, b) = (ax bx + ay by) + az bz
 *     D'  = uv' uv' - uu' vv'.
 *
 * Per pair: the per-leaf routine of rt_hip_nearest.h for the triangle (ta', u', v', uu', uv', vv', D') and the world point q,
 * unchanged: regions, refinement, p = ta' + (u' s + v' t), e = q - p, d2 = dot(e, e).
 *
 * The answer is the minimum over all pairs of (d2, instance, leaf): a strictly smaller d2 wins, among equal d2 below +inf the
 * lower (instance, leaf) pair; a d2 that is NaN or +inf never replaces the record, which starts at +inf.  The answer depends
 * on neither tree -- not the scene's, not the top-level one -- nor on the order of any walk: the library's trees and bounds
 * decide where it LOOKS, never what it finds.
 *
 * `found` (the `hit` field), the radius and odd inputs follow rt_hip_nearest.h exactly: found iff some pair has
 * sqrt(d2) <= max_distance in binary32; a max_distance that is negative or NaN, and a point with a coordinate that is NaN or
 * infinite, find nothing.
 * Found: the record is in WORLD space -- distance, leaf, barycentric (1 - s - t, s, t), position p, `instance` = k -- and the
 * normal is the instanced record's normal of rt_hip_instances.h: raw = (n0 b0 + n1 b1) + n2 b2 with the leaf's vertex normals
 * and the returned barycentrics, w = transpose(O_k) raw, ONE normalisation of w.
 * Not found: distance +inf, leaf and instance 0xFFFFFFFF, barycentrics, position and normal 0.
 *
 * Relation to rt_hip_nearest.h: with ONE instance whose transform is the identity, on a scene whose vertex coordinates are
 * finite and hold no -0 (nor its vertex normals: 1 * x + 0 * y turns a -0 into +0), every output word equals
 * rt_closest_points', and `instance` is 0 where found.
 *
 * Outputs are rt_instance_hit_arrays (rt_hip_instances.h), any of them NULL: not written.  Everything else follows the other
 * queries: the blocking host-memory form and the enqueued device-memory form, RT_QUERY_MAX_RAYS points per call,
 * RT_QUERY_NO_SORT / RT_QUERY_SORT_MIN (the sort's key is the position alone, quantised over the TOP-LEVEL ROOT BOX; every
 * result goes to its point's own index and not a bit depends on the order), n == 0 succeeds and launches nothing,
 * rt_last_query_ms covers the query, the scratch is the host's queries' own.
 *
 * The set persists across rt_update_vertices, rt_build_scene and uploads as rt_hip_instances.h says; the answer follows the
 * new geometry.  No plain entry point notices a set: rt_closest_points answers for the uploaded scene alone.
 *
 * Errors: those of rt_hip_instances.h -- RT_E_STATE before an upload, with no instances set, on the hosts of a frame ring --
 * and RT_E_INVALID as in rt_hip_nearest.h: null points with n > 0, device points not 16-byte aligned, device float / uint32
 * outputs not 4-byte aligned, n > RT_QUERY_MAX_RAYS.
 */
#ifndef RT_HIP_INSTANCE_NEAREST_H
#define RT_HIP_INSTANCE_NEAREST_H

#include "rt_hip_instances.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host memory, blocking.  points4: float4[n], .w ignored.  `out` may be NULL (nothing is written). */
int rt_instances_closest_points(rt_host *h, const float *points4, uint32_t n, float max_distance, uint32_t flags,
                                const rt_instance_hit_arrays *out);

/* Device memory on the host's device, enqueued on `hip_stream` (NULL: the host's stream); returns without waiting.  The
 * points must stay unchanged until the query has run.  `out` points to host memory that holds device pointers and is read
 * during the call. */
int rt_instances_closest_points_device(rt_host *h, const float *points4, uint32_t n, float max_distance, uint32_t flags,
                                       const rt_instance_hit_arrays *out, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
