/* rt_hip_instance_directional.h -- instanced directional occlusion queries: WHICH of a world-space point's ambient-occlusion
 * rays were blocked by the posed copies of the uploaded scene, and the sum of the directions of those that were not (bent
 * normals, SH projection and sky visibility of a posed assembly).
 *
 * The composition of rt_hip_directional.h and rt_hip_instance_views.h (rt_trace_instances_ao).  Points and normals are in
 * WORLD space.  The rays of point i are exactly rt_ao_rays's for the same points, normals and seeds -- origin point_i +
 * normal_i * (1.0f / 100000.0f), direction k as rt_hip_directional.h defines it -- and nothing about them involves the set.
 * Each ray is cast as rt_trace_instances_occluded casts it (rt_hip_instances.h: the top-level boxes, the object ray, the
 * scene's own walk) with the host's ao_max_distance.  On those flags the outputs are rt_hip_directional.h's, unchanged; let
 * R, n be what rt_ao_rays_per_point returns and W = ceil(R / 32) (rt_ao_mask_words):
 *   mask      uint32[n_points][W]  bit k & 31 of word k >> 5 of row i is 1 iff ray k of point i is occluded; the bits from R
 *                                  upwards are 0;
 *   occluded  uint32[n_points]     the popcount of the point's row: rt_trace_instances_ao's `occluded`, word for word;
 *   ao        float[n_points]      1.0f - ((float) occluded / (float) n): rt_trace_instances_ao's `ao`, word for word;
 *   bent      float[3 * n_points]  per component, starting from +0.0f: b = b + dir_ik for k = 0, 1, ..., R - 1 IN THAT ORDER
 *                                  over the rays whose bit is 0, every addition rounded to binary32, no fused multiply-add.
 * Any output may be NULL; a call that asks for nothing launches nothing.
 *
 * In UNIFORM mode all four outputs lie inside the bit-exact contract with the CPU oracle; in RANDOM mode the masks equal
 * rt_trace_instances_occluded on the rays rt_ao_rays writes, and `occluded` equals rt_trace_instances_ao's, exactly.  With
 * ONE instance whose transform is the identity, on points whose rays hold no -0 and only finite components, every output
 * equals rt_trace_ao_directional's.
 *
 * Sorting of the POINTS (from RT_QUERY_SORT_MIN rays on; RT_QUERY_NO_SORT; the key's cells over the top-level root box),
 * limits, legal inputs (every float is) and what a query leaves alone are rt_trace_instances_ao's: sorted, unsorted and
 * shuffled calls return identical words by point, and rt_last_query_ms reports the call.
 *
 * Errors: as rt_trace_instances_ao -- RT_E_STATE before an upload, with no instances set, on the hosts of a frame ring and
 * on a host whose options have ambient occlusion off; RT_E_INVALID for null points or normals with n > 0, device float4
 * pointers not 16-byte aligned, other device outputs or seeds not 4-byte aligned, n above RT_QUERY_MAX_RAYS / R.  n == 0
 * succeeds and launches nothing.
 */
#ifndef RT_HIP_INSTANCE_DIRECTIONAL_H
#define RT_HIP_INSTANCE_DIRECTIONAL_H

#include "rt_hip_directional.h"
#include "rt_hip_instances.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host memory, blocking.  points4 / normals4: float4[n], world space; seeds: uint32[n] or NULL; out: rt_hip_directional.h's
 * arrays (a NULL `out` asks for nothing). */
int rt_trace_instances_ao_directional(rt_host *h, const float *points4, const float *normals4, const uint32_t *seeds, uint32_t n,
                                      uint32_t flags, const rt_ao_directional_arrays *out);

/* Device memory on the host's device, enqueued on `hip_stream` (NULL: the host's stream); returns without waiting.  The
 * inputs must stay unchanged until the query has run. */
int rt_trace_instances_ao_directional_device(rt_host *h, const float *points4, const float *normals4, const uint32_t *seeds,
                                             uint32_t n, uint32_t flags, const rt_ao_directional_arrays *out, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
