/* rt_hip_directional.h -- directional occlusion queries on an uploaded scene: WHICH of a point's ambient-occlusion rays
 * were blocked, and the sum of the directions of those that were not (bent normals, directional visibility for SH or cone
 * projection, sky visibility: whatever a caller folds over "ray k of point i was blocked").
 *
 * Beside rt_hip_ao.h, whose rules hold here unchanged: the points, normals and seeds are those of rt_trace_ao, the rays
 * are the ones the reference's
 *     ambient_occlusion(nodes, aabbs, faces, vertices, normals, point_i, normal_i, index_i)        (:214-277)
 * casts with the options the host was created with, and they are made on the device.  Let R, n be what
 * rt_ao_rays_per_point returns.  Ray k (0 <= k < R) of point i is the k-th ray that function casts:
 *   - UNIFORM: table direction k in the point's tangent frame, (basis_x * xs + basis_y * ys) + basis_z * zs, not normalised;
 *   - RANDOM:  ray 0 along the normal as given (not normalised), ray k >= 1 the generator's sample k, normalised.
 * Let W = ceil(R / 32) (rt_ao_mask_words).  The outputs, any of which may be NULL:
 *   mask      uint32[n_points][W]  bit k & 31 of word k >> 5 of row i is 1 iff scene_intersect(origin_i, dir_ik,
 *                                  ao_max_distance) is true; the bits from R upwards are 0;
 *   occluded  uint32[n_points]     the popcount of the point's row: rt_trace_ao's `occluded`, word for word;
 *   ao        float[n_points]      1.0f - ((float) occluded / (float) n): rt_trace_ao's `ao`, word for word;
 *   bent      float[3 * n_points]  per component, starting from +0.0f: b = b + dir_ik for k = 0, 1, ..., R - 1 IN THAT
 *                                  ORDER over the rays whose bit is 0, every addition rounded to binary32, no fused
 *                                  multiply-add.  dir_ik is the direction as cast; nothing is normalised afterwards (a
 *                                  caller divides by R - occluded, or normalises, as they like).  A point whose frame
 *                                  is not a number (a zero normal) gets what the arithmetic gives.
 * A call that asks for nothing launches nothing.  The origin of every ray of point i is point_i + normal_i * (1.0f /
 * 100000.0f) (rt_hip_ao.h).
 *
 * The masks are hit flags -- integers -- so in UNIFORM mode all four outputs lie inside the bit-exact contract with the
 * CPU oracle; in RANDOM mode they depend on the device's libm as rt_trace_ao does, and agree with each
 * other, with rt_trace_ao and with rt_ao_rays exactly.
 *
 * Flags, sorting (of the POINTS, from RT_QUERY_SORT_MIN rays on; RT_QUERY_NO_SORT), limits, legal inputs (every float is)
 * and what a query leaves alone (everything of a frame) are rt_hip_ao.h's: sorted, unsorted and shuffled calls return
 * identical words, and rt_last_query_ms reports the call.
 *
 * rt_ao_rays writes the rays themselves, so that a mask can be used without restating the reference's tangent frame and
 * direction table: origins4 float4[n] (.w 0), directions4 float4[n * R], direction k of point i at [i * R + k] (.w 0).
 * Either may be NULL.  No walk is run.
 *
 * Errors: as rt_hip_ao.h -- RT_E_STATE before an upload, on the hosts of a frame ring, and on a host whose options have
 * ambient occlusion off; RT_E_INVALID for null points or normals with n > 0, device float4 pointers (points4, normals4,
 * origins4, directions4) not 16-byte aligned, other device outputs or seeds not 4-byte aligned, n above
 * RT_QUERY_MAX_RAYS / R.  n == 0 succeeds and launches nothing.
 */
#ifndef RT_HIP_DIRECTIONAL_H
#define RT_HIP_DIRECTIONAL_H

#include "rt_hip_ao.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rt_ao_directional_arrays {
	float *ao;          /* float[n] */
	uint32_t *occluded; /* uint32[n] */
	uint32_t *mask;     /* uint32[n][W] */
	float *bent;        /* float[3 n] */
} rt_ao_directional_arrays;

/* W, the words of a point's mask row with this host's options.  RT_E_STATE as rt_ao_rays_per_point. */
int rt_ao_mask_words(const rt_host *h, uint32_t *words);

/* Host memory, blocking.  points4 / normals4: float4[n]; seeds: uint32[n] or NULL; out: the arrays above (a NULL `out` asks
 * for nothing). */
int rt_trace_ao_directional(rt_host *h, const float *points4, const float *normals4, const uint32_t *seeds, uint32_t n,
                            uint32_t flags, const rt_ao_directional_arrays *out);

/* Device memory on the host's device, enqueued on `hip_stream` (NULL: the host's stream); returns without waiting.  The
 * inputs must stay unchanged until the query has run. */
int rt_trace_ao_directional_device(rt_host *h, const float *points4, const float *normals4, const uint32_t *seeds, uint32_t n,
                                   uint32_t flags, const rt_ao_directional_arrays *out, void *hip_stream);

/* The rays of the points.  Host memory, blocking. */
int rt_ao_rays(rt_host *h, const float *points4, const float *normals4, const uint32_t *seeds, uint32_t n, float *origins4,
               float *directions4);

/* Device memory, enqueued on `hip_stream` (NULL: the host's stream). */
int rt_ao_rays_device(rt_host *h, const float *points4, const float *normals4, const uint32_t *seeds, uint32_t n, float *origins4,
                      float *directions4, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
