/* rt_hip_nearest.h -- closest-point queries on an uploaded scene: for points the caller supplies, the nearest point of the
 * surface and how far away it is.
 *
 * Beside rt_hip_query.h, whose calls need a direction: a point has none.  The scene is the one a render host holds after
 * rt_upload / rt_upload_scene, after rt_update_vertices, or after rt_build_scene.
 *
 * Candidates.  For a point q and the call's max_distance the candidates are ALL leaves of the uploaded scene.  Leaf L is
 * described by the values the device holds for it: ta, u = tb - ta, v = tc - ta (each rounded once), uu = dot(u, u),
 * uv = dot(u, v), vv = dot(v, v), D = uv uv - uu vv.
 *
 * Per-leaf arithmetic, IEEE binary32, every operation rounded on its own (no contraction), in this order
 * (csrc/nearest_point.h is this text as code, compiled by the kernel and by the tests' oracle alike):
 *     w  = q - ta                          d1 = dot(u, w)      d2 = dot(v, w)       dot(a, b) = (ax bx + ay by) + az bz
 *     d3 = d1 - uu     d4 = d2 - uv        d5 = d1 - uv        d6 = d2 - vv
 *   vertex A   d1 <= 0 and d2 <= 0                                          (s, t) = (0, 0)
 *   vertex B   d3 >= 0 and d4 <= d3                                         (s, t) = (1, 0)
 *   edge AB    vc = uu d2 - uv d1;   uu > 0, vc <= 0, d1 >= 0, d3 <= 0      (s, t) = (d1 / uu, 0)
 *   vertex C   d6 >= 0 and d5 <= d6                                         (s, t) = (0, 1)
 *   edge AC    vb = vv d1 - uv d2;   vv > 0, vb <= 0, d2 >= 0, d6 <= 0      (s, t) = (0, d2 / vv)
 *   edge BC    va = d3 d6 - d5 d4;   g = d4 - d3, h = d5 - d6, gh = g + h;
 *              gh > 0, va <= 0, g >= 0, h >= 0                              k = g / gh, (s, t) = (1 - k, k)
 *   face       m = -D; solve(r1, r2): if uu >= vv, t = (uu r2 - uv r1) / m and s = (r1 - uv t) / uu; else s = (vv r1 - uv r2) / m
 *              and t = (r2 - uv s) / vv.  (s0, t0) = solve(d1, d2); p0, e0 of (s0, t0) as below; (ds, dt) = solve(dot(u, e0),
 *              dot(v, e0)); s = s0 + ds, t = t0 + dt (one step of refinement: on a sliver m keeps a few digits only);
 *              taken if m > 0, s >= 0, t >= 0 and s + t <= 1
 *   otherwise  the nearest of the three edges as segments, in the order AB, AC, BC: parameters clamp(d1 / uu), clamp(d2 / vv),
 *              clamp(g / gh) to [0, 1], 0 for an edge of no length; the first of equal d2 stays.
 *   p = ta + (u s + v t) per component,  e = q - p,  d2 = dot(e, e),  distance = sqrt(d2).
 * The first region whose test holds is taken.  Degenerate triangles count as the segment or point they are: an edge of no
 * length is skipped -- its vertices' regions come before it --, a triangle without area fails `m > 0` and falls to its
 * edges; finite inputs (below 1e9 in magnitude, so that no product overflows) never give a NaN.
 *
 * The answer is the minimum over all leaves of (d2, leaf index): among equal d2 the lowest leaf wins.  A d2 that is NaN or
 * +inf never replaces the record, which starts at +inf.  The answer depends on neither the tree nor the order of the walk.
 *
 * `found` (the `hit` field) is 1 iff some leaf has distance <= max_distance, compared in binary32: +inf finds anything at
 * a finite distance, 0 only points on the surface; a max_distance that is negative or NaN, and a point with a coordinate
 * that is NaN or infinite, find nothing.  Found: distance, leaf, barycentric (1 - s - t, s, t), position p, and normal --
 * the smooth normal of rt_hip_query.h for that leaf and those barycentrics.  Not found: distance +inf, leaf 0xFFFFFFFF,
 * barycentrics, position and normal 0.
 *
 * Outputs are rt_hit_arrays (rt_hip_query.h), any of them NULL: not written.  Leaf indices as in rt_hip_query.h.
 * Everything else is rt_hip_query.h's too: the blocking host-memory form and the enqueued device-memory form,
 * RT_QUERY_MAX_RAYS points per call, RT_QUERY_NO_SORT (the points are coherent already; below RT_QUERY_SORT_MIN points
 * nothing is sorted; either way every result goes to its point's own index and not a bit depends on the order),
 * n == 0 succeeds and launches nothing, rt_last_query_ms covers the query, the scratch is the host's queries' own, one
 * host's queries are serialised with each other, and nothing a frame produces or reports is touched.
 *
 * Errors: RT_E_STATE before an upload and for the hosts of a frame ring; RT_E_INVALID for null points with n > 0, device
 * points not 16-byte aligned, device float / uint32 outputs not 4-byte aligned, n > RT_QUERY_MAX_RAYS.
 */
#ifndef RT_HIP_NEAREST_H
#define RT_HIP_NEAREST_H

#include "rt_hip_query.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host memory, blocking.  points4: float4[n], .w ignored.  `out` may be NULL (nothing is written). */
int rt_closest_points(rt_host *h, const float *points4, uint32_t n, float max_distance, uint32_t flags, const rt_hit_arrays *out);

/* Device memory on the host's device, enqueued on `hip_stream` (NULL: the host's stream); returns without waiting.  The
 * points must stay unchanged until the query has run.  `out` points to host memory that holds device pointers and is read
 * during the call. */
int rt_closest_points_device(rt_host *h, const float *points4, uint32_t n, float max_distance, uint32_t flags,
                             const rt_hit_arrays *out, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
