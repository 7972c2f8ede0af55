/* rt_hip_views.h -- multi-view rendering: the frame layers and the finished 8-bit image of many camera poses against one
 * uploaded scene.
 *
 * Beside the seam (rt_hip.h), like rt_hip_layers.h: a host renders the one view it was uploaded for (rt_hip_camera.h: the
 * pose is fixed per upload), and a turntable pays an upload per view.  These entry points render `views` poses against
 * the scene a host holds already: no new upload, nothing of the host changed.
 *
 * W, H, N and the sub-pixel index i = y * W + x are those of rt_hip_layers.h; width and height are the options' own.
 * `cameras` is host memory in both forms -- `views` poses, read during the call: it may be freed on return.  Every
 * non-NULL array of `layers` holds `views` consecutive blocks of that layer's size for one frame (rt_hip_layers.h);
 * `image` is uint8[views][height][width].
 *
 *   layers   block v holds, word for word, what rt_render_layers returns on a host with the same options and scene that
 *            was given cameras[v] with rt_set_camera before its upload: always the posed form of the ray (rt_hip_camera.h),
 *            also where cameras[v] is the default pose.  Any float is legal in a pose -- eyes far beyond the scene,
 *            non-finite eyes, bases that are neither unit nor orthogonal --: the walk is the exact form, as for the layers.
 *   image    block v is RayTracer::resize (reference src/ray_tracer.cc:3-16) of view v's `value`: the bytes rt_download_u8
 *            returns on that posed host after rt_render, and what rt_resize_cpu makes of `value`.
 *   seeds    the reference's `index` of a sub-pixel in ambient_occlusion(position, normal, index) is its index WITHIN ITS
 *            VIEW, i -- not its place in the call: the RANDOM method's samples depend on it.
 *
 * The host's own pose plays no part, and the host need not have one.
 *
 * Like a query, the call changes nothing a frame produces or reports: it uses scratch of its own (grown on demand, freed
 * by rt_destroy) and leaves the float image, the hit list, counters and statistics (rt_get_stats), captured graphs and
 * timers alone.  rt_last_query_ms (rt_hip_query.h) reports its time.
 *
 * `views` has no limit: the call works through the views in chunks, sized so that a chunk's ambient-occlusion step stays
 * within RT_QUERY_MAX_RAYS (rt_hip_query.h) were every sub-pixel of the chunk hit, and its scratch grows with the chunk,
 * not with `views`.  That step runs over the sub-pixels that were hit alone; the others get ao = 1, value = 0.  ONE view
 * is limited as rt_render_layers is.  views == 0, or a call that asks for nothing, succeeds and launches nothing.
 *
 * rt_render_views_device enqueues on `hip_stream` and does not wait for its last kernels; where it runs the
 * ambient-occlusion step (`ao`, or `value` / `image` on a host whose options have ambient occlusion on) it waits, once per
 * chunk, for that chunk's own rays: the number of sub-pixels they hit sizes the step.
 *
 * Errors: RT_E_STATE before an upload, on the hosts of a frame ring (rt_ring_host), on a band-partitioned host
 * (nranks > 1), and for `ao` on a host whose options have ambient occlusion off; RT_E_INVALID for a NULL `out`, for NULL
 * `cameras` with views > 0, for device float / uint32 outputs not 4-byte aligned, and for `ao` -- or `value` / `image` on a
 * host with ambient occlusion on -- when N exceeds RT_QUERY_MAX_RAYS / rays per point (rt_hip_ao.h).
 */
#ifndef RT_HIP_VIEWS_H
#define RT_HIP_VIEWS_H

#include "rt_hip_camera.h"
#include "rt_hip_layers.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rt_view_arrays { /* any pointer may be NULL: not written */
	rt_layer_arrays layers; /* `views` blocks each */
	uint8_t *image;         /* [views][height][width] */
} rt_view_arrays;

/* Host memory, blocking. */
int rt_render_views(rt_host *h, const rt_camera *cameras, uint32_t views, const rt_view_arrays *out);

/* Device memory on the host's device, enqueued on `hip_stream` (NULL: the host's stream).  `out` points to host memory
 * that holds device pointers and is read during the call. */
int rt_render_views_device(rt_host *h, const rt_camera *cameras, uint32_t views, const rt_view_arrays *out, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
