/* rt_hip_instance_views.h -- the instance set seen and shaded: ambient occlusion at world-space points against the posed
 * copies of the uploaded scene, and multi-view rendering of them -- every frame layer, the instance id and the finished
 * 8-bit image.
 *
 * Beside rt_hip_instances.h, rt_hip_ao.h and rt_hip_views.h, and defined by COMPOSITION of their contracts: nothing below
 * computes a value that one of those headers does not define already.  The set is the host's (rt_set_instances); the plain
 * entry points -- rt_trace_ao, rt_render_layers, rt_render_views, frames -- still ignore it, bit for bit.
 *
 * Instanced ambient occlusion (rt_trace_instances_ao).  Points and normals are in WORLD space, float[n][4] each (the fourth
 * component is not read); `seeds` uint32[n] or NULL (the point's own index), read by the RANDOM method alone.
 *   - The rays of point i are exactly the rays rt_trace_ao makes for it (rt_hip_ao.h; rt_ao_rays writes them out): origin
 *     point + normal * (1.0f / 100000.0f), the tangent frame of the normal, then the table direction (UNIFORM) or the
 *     sampler's (RANDOM, seeded by seeds[i], or by i).  The normal is used as given.
 *   - Each ray is cast as rt_trace_instances_occluded casts it with max_distance = ao_max_distance of the host's options:
 *     entered, mapped into the object's frame and tested by the rules of rt_hip_instances.h, on the tree the library built.
 *   - occluded[i] is the number of its rays that are occluded; ao[i] = 1.0f - ((float) occluded[i] / (float) divisor) with
 *     the divisor of rt_ao_rays_per_point.  Either output may be NULL.
 *   - Every float input is legal; odd points and normals get the rules' own answer.
 *   - Coherence: the ambient-occlusion queries' sort of the POINTS (from as many on as make RT_QUERY_SORT_MIN rays;
 *     RT_QUERY_NO_SORT is honoured), their cells over the top-level root box as in the instanced ray queries.  No output
 *     bit depends on the order.
 *   - Limits: those of rt_hip_ao.h, at most RT_QUERY_MAX_RAYS / rays per point points per call.  n == 0 launches nothing.
 *   - Errors, the union of the two parents': RT_E_STATE before an upload, with no instances set, on the hosts of a frame
 *     ring, and on a host whose options have ambient occlusion off; RT_E_INVALID for NULL points or normals with n > 0,
 *     device points or normals not 16-byte aligned, device seeds or outputs not 4-byte aligned, and n above the limit.
 *
 * Instanced views (rt_render_instance_views).  W, H, N, the sub-pixel index i = y * W + x, `cameras` and the ray of
 * sub-pixel i of view v are those of rt_hip_views.h: always the posed form (rt_hip_camera.h), with the primary pass's
 * bits.  Every non-NULL array holds `views` consecutive blocks.  Per ray (o, d):
 *   hit, distance, leaf, barycentric, position, normal, instance
 *              what rt_trace_instances_closest returns for (o, d) with max_distance = 100000.0f, word for word: the no-hit
 *              record (hit 0, instance and leaf 0xFFFFFFFF, distance +inf, the rest 0) and the "candidate but none below
 *              +inf" record (hit 1, instance 0, leaf 0, distance +inf, the rest 0) included.
 *   direction  d.
 *   shade      where hit is 1: min(max(-dot(normal, d), 0), 1) on the record's own normal words -- the dot product
 *              (normal.x * d.x + normal.y * d.y) + normal.z * d.z, then fmaxf, then fminf, so a NaN operand loses --, or
 *              1.0f on a host with shading off; 0.0f where hit is 0.
 *   ao         what rt_trace_instances_ao returns for (position, normal, seed i) of the record -- the seed is the index
 *              WITHIN THE VIEW, as in rt_hip_views.h --; 1.0f where hit is 0.
 *   value      shade * ao; shade alone on a host whose options have ambient occlusion off.
 *   image      RayTracer::resize (reference src/ray_tracer.cc:3-16) of view v's `value`: the bytes rt_resize_cpu makes.
 * The rest is rt_hip_views.h's: `views` has no limit, the call works in chunks (rt_debug_set_views_chunk applies, and
 * rt_debug_last_views reports chunks and ambient-occlusion points as for a plain views call); the ambient-occlusion step
 * runs over the hit sub-pixels alone, in index order; scratch of the call's own; frames, graphs, counters and timers are
 * left alone; rt_last_query_ms covers it; the host's own pose plays no part; the device form waits once per chunk where it
 * runs the ambient-occlusion step.  Operation order within a chunk: the rays of all its views, the list of the hit
 * sub-pixels, their ambient-occlusion rays, `ao` and `value`, the images.
 * Errors: those of rt_hip_views.h, plus RT_E_STATE with no instances set; `instance` on the device must be 4-byte aligned.
 *
 * Relation to rt_hip_views.h (as rt_hip_instances.h states its own).  With ONE instance whose transform is the identity, at
 * the sub-pixels whose ray's six components are finite and hold no -0 and where rt_render_views' record has a distance
 * below +inf: the record layers, `direction` and `shade` equal rt_render_views' word for word, with instance 0.  `ao`,
 * `value` -- and a pixel of `image` all of whose sub-pixels qualify -- follow wherever, in addition, none of that
 * sub-pixel's ambient-occlusion rays (origin and direction) holds a -0.  The reason is rt_hip_instances.h's:
 * 1 * x + 0 * y turns a -0 into +0, and for a direction component that flips the reference's `inv >= 0` choice of the
 * near plane.
 */
#ifndef RT_HIP_INSTANCE_VIEWS_H
#define RT_HIP_INSTANCE_VIEWS_H

#include "rt_hip_ao.h"
#include "rt_hip_instances.h"
#include "rt_hip_views.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host memory, blocking. */
int rt_trace_instances_ao(rt_host *h, const float *points4, const float *normals4, const uint32_t *seeds, uint32_t n, uint32_t flags,
                          float *ao, uint32_t *occluded);
/* Device memory on the host's device, enqueued on `hip_stream` (NULL: the host's stream); returns without waiting. */
int rt_trace_instances_ao_device(rt_host *h, const float *points4, const float *normals4, const uint32_t *seeds, uint32_t n,
                                 uint32_t flags, float *ao, uint32_t *occluded, void *hip_stream);

typedef struct rt_instance_view_arrays { /* any pointer may be NULL: not written */
	rt_view_arrays views; /* rt_hip_views.h: the layers (`views` blocks each) and the images */
	uint32_t *instance;   /* [views][N]; 0xFFFFFFFF where hit is 0 */
} rt_instance_view_arrays;

/* Host memory, blocking. */
int rt_render_instance_views(rt_host *h, const rt_camera *cameras, uint32_t views, const rt_instance_view_arrays *out);
/* Device memory on the host's device, enqueued on `hip_stream` (NULL: the host's stream).  `out` points to host memory
 * that holds device pointers and is read during the call. */
int rt_render_instance_views_device(rt_host *h, const rt_camera *cameras, uint32_t views, const rt_instance_view_arrays *out,
                                    void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
