/* rt_hip_ao.h -- ambient-occlusion queries on an uploaded scene: the AO term at points the caller supplies (per-vertex
 * AO baking, lightmap texels, probe points).
 *
 * Beside the seam (rt_hip.h), like rt_hip_query.h: the reference only computes the term at the hits of its own camera
 * (src/intersect_kernel.cl:305-307).  For point i these entry points return what the reference's
 *     ambient_occlusion(nodes, aabbs, faces, vertices, normals, point_i, normal_i, index_i)        (:214-277)
 * returns with the options the host was created with -- ao_method, ao_num_samples, ao_alpha_min / ao_alpha_max,
 * ao_max_distance -- on the scene the host holds after rt_upload / rt_upload_scene: ao[i] is the float result,
 * occluded[i] its `hits`.  Either output may be NULL.  .w of the float4 inputs is ignored.  index_i is seeds[i], or i
 * when `seeds` is NULL; only the RANDOM method uses it (it seeds the point's generator, :169), UNIFORM ignores it.
 *
 * The rays are made on the device from the point and the normal -- no ray array is passed -- and the reference's rules
 * hold as they are:
 *   - the normal is used AS GIVEN: UNIFORM does not normalise it ("already normalized", :224); RANDOM normalises it
 *     once for the basis (:155) and casts the un-normalised normal as ray 0 (:264);
 *   - the origin is point + normal * (1.0f / 100000.0f), the product and the sum rounded separately (:215);
 *   - the tangent frame is that of :224-236: the smallest |component| of the normal replaced by 1 gives h,
 *     basis_x = normalize(cross(h, basis_y)), basis_z = normalize(cross(basis_x, basis_y));
 *   - ray_dir = (basis_x * xs + basis_y * ys) + basis_z * zs per component, no fused multiply-add (:248; RANDOM
 *     normalises the sum, :182);
 *   - max_distance is ao_max_distance and only culls BOXES (rt_hip_query.h);
 *   - the result is 1.0f - ((float) hits / (float) n) with a correctly rounded division (:256, :275); in RANDOM mode
 *     n is ao_num_samples + 1 while ao_num_samples + 2 rays are cast, so `hits` may exceed n (and ao[i] be negative);
 *   - every float input is legal: zero, tiny or huge normals, NaN or inf anywhere, points far from the scene.  Such a
 *     point gets the reference's answer, usually 1.0 with 0 hits.
 * UNIFORM is inside the bit-exact contract with the CPU oracle; RANDOM depends on the device's libm, as it
 * does for frames.
 *
 * Flags: RT_QUERY_NO_SORT (rt_hip_query.h) -- the points are coherent already (neighbours in the arrays lie near each
 * other): cast them in their own order.  Otherwise the POINTS are ordered by a coherence key before their rays are
 * cast; calls that make fewer than RT_QUERY_SORT_MIN rays are never sorted.  The order decides nothing but the speed:
 * sorted and unsorted calls return identical words.  At most RT_QUERY_MAX_RAYS / rays_per_point points per call.
 *
 * Like a ray query, an AO query changes nothing a frame produces or reports: it reads the scene's arrays and the
 * direction table, uses scratch buffers of its own (grown on demand, freed by rt_destroy) and leaves the frame's
 * buffers, captured graph, counters (rt_get_stats) and timers alone.  rt_last_query_ms (rt_hip_query.h) reports it.
 *
 * Errors: RT_E_STATE before an upload, on the hosts of a frame ring (rt_ring_host), and on a host whose options have
 * ambient occlusion off (enable_ao == 0 or ao_num_samples == 0: there is no direction table on the device);
 * RT_E_INVALID for null points or normals with n > 0, device point or normal pointers not 16-byte aligned, device
 * outputs or seeds not 4-byte aligned, n above the limit.  n == 0 succeeds and launches nothing.
 */
#ifndef RT_HIP_AO_H
#define RT_HIP_AO_H

#include "rt_hip_query.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Rays the reference casts per point with this host's options, and the n of `1 - hits / n` (UNIFORM: table size, table
 * size; RANDOM: ao_num_samples + 2, ao_num_samples + 1).  Either pointer may be NULL.  RT_E_STATE as above. */
int rt_ao_rays_per_point(const rt_host *h, uint32_t *rays, uint32_t *divisor);

/* Host memory, blocking.  points4 / normals4: float4[n]; seeds: uint32[n] or NULL; ao: float[n] or NULL; occluded:
 * uint32[n] or NULL. */
int rt_trace_ao(rt_host *h, const float *points4, const float *normals4, const uint32_t *seeds, uint32_t n, uint32_t flags,
                float *ao, uint32_t *occluded);

/* Device memory on the host's device, enqueued on `hip_stream` (NULL: the host's stream); returns without waiting.  The
 * inputs must stay unchanged until the query has run (they are read twice when sorted). */
int rt_trace_ao_device(rt_host *h, const float *points4, const float *normals4, const uint32_t *seeds, uint32_t n,
                       uint32_t flags, float *ao, uint32_t *occluded, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
