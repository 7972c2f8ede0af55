/* rt_hip_layers.h -- frame layers: what lies behind the grey image, per sub-pixel, for the rays the frame itself casts.
 *
 * Beside the seam (rt_hip.h), like rt_hip_query.h: the reference returns one image.  These entry points return, for
 * every sub-pixel of a host's frame, the layers that image is made of -- hit mask, depth, triangle id, barycentrics,
 * hit point, smooth normal, view direction, head-light term, ambient-occlusion factor and their product -- for
 * compositing, denoising, depth and normal maps, segmentation ids and training data.
 *
 * Let W x H be rt_total_width x rt_total_height of the host's options and N = W * H.  Sub-pixel (x, y) has index
 * i = y * W + x.  Its ray is the one the frame casts for it (src/intersect_kernel.cl:279-295):
 *   - a host without a pose: origin (0, 0, 2), direction normalize((cx, cy, -1)) with
 *       cx = (x + 0.5f) / a - W / (2.0f * a),  cy = -((y + 0.5f) / a - H / (2.0f * a)),  a = focal_length * max(W, H);
 *   - a host with a pose (rt_hip_camera.h, rt_set_camera): origin eye, direction
 *       normalize(((right * cx) + (up * cy)) + forward), every product and sum rounded on its own.
 * In both cases the ray has exactly the bits the frame's primary pass makes.  Per ray:
 *
 *   hit, distance, leaf, barycentric, position, normal
 *               what rt_trace_closest (rt_hip_query.h) returns for that ray with max_distance = 100000.0f (the
 *               frame's), word for word -- the no-hit values and the "accepted but never replaced" record included;
 *   direction   float[3N]: the ray's direction (its origin is the host's eye, rt_get_camera);
 *   shade       float[N]: the reference's shade(direction, normal) = min(max(-dot(normal, direction), 0), 1), or 1.0f
 *               on a host whose options have shading off; 0.0f where hit is 0;
 *   ao          float[N]: the reference's ambient_occlusion(position, normal, i) with the host's options -- what
 *               rt_trace_ao (rt_hip_ao.h) returns for those points and normals with seeds i --; 1.0f where hit is 0;
 *   value       float[N]: shade * ao (shade alone on a host whose options have ambient occlusion off): the bits
 *               rt_download returns for the same host after rt_render.
 *
 * Every pointer of rt_layer_arrays may be NULL: that layer is not written.  A call that asks for nothing succeeds.
 *
 * Like a query, the call changes nothing a frame produces or reports: it uses scratch of its own (grown on demand,
 * freed by rt_destroy) and leaves the float image, the hit list, counters and statistics (rt_get_stats), captured
 * graphs and timers alone.  rt_last_query_ms (rt_hip_query.h) reports its time.  The pose is the host's at the time of
 * the call; it is fixed per upload.
 *
 * Errors: RT_E_STATE before an upload, on the hosts of a frame ring (rt_ring_host), on a band-partitioned host
 * (nranks > 1: it renders a part of the image only), and for `ao` on a host whose options have ambient occlusion off;
 * RT_E_INVALID for a NULL `out`, for device float / uint32 outputs not 4-byte aligned, and for `ao` -- or `value` on a
 * host with ambient occlusion on -- when N exceeds RT_QUERY_MAX_RAYS / rays per point (rt_hip_ao.h).
 */
#ifndef RT_HIP_LAYERS_H
#define RT_HIP_LAYERS_H

#include "rt_hip_ao.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rt_layer_arrays { /* any pointer may be NULL: that layer is not written */
	uint8_t *hit;       /* [N] 1 = hit */
	float *distance;    /* [N] +inf when no hit */
	uint32_t *leaf;     /* [N] reference face_id / 3 (leaf order); 0xFFFFFFFF when no hit */
	float *barycentric; /* [3N] (1-s-t, s, t) */
	float *position;    /* [3N] */
	float *normal;      /* [3N] smooth normal (get_smooth_normal) */
	float *direction;   /* [3N] the sub-pixel's ray direction */
	float *shade;       /* [N] head-light term; 0 when no hit */
	float *ao;          /* [N] ambient-occlusion factor; 1 when no hit */
	float *value;       /* [N] shade * ao: rt_download's float image */
} rt_layer_arrays;

/* Host memory, blocking. */
int rt_render_layers(rt_host *h, const rt_layer_arrays *out);

/* Device memory on the host's device, enqueued on `hip_stream` (NULL: the host's stream); returns without waiting.
 * `out` points to host memory that holds device pointers and is read during the call. */
int rt_render_layers_device(rt_host *h, const rt_layer_arrays *out, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
