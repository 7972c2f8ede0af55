/* rt_hip_camera.h -- a posed camera: frames from any eye point and orientation.
 *
 * Beside the seam (rt_hip.h), like rt_hip_ring.h, rt_hip_debug.h and rt_hip_query.h: the reference renders every frame
 * from the eye (0, 0, 2) looking down -z (src/intersect_kernel.cl:284-291).  A host that is given a pose BEFORE its
 * upload renders from there instead; a host that is given none renders the reference's view on the code path it always
 * took, bit for bit.
 *
 * The contract.  A pose is four float triples, used AS GIVEN: not normalised, not orthogonalised, every float value
 * legal.  For sub-pixel (x, y) of the W x H supersampled image the camera-space terms are the reference's,
 *     a  = focal_length * max(W, H)
 *     cx =   ((float) x + 0.5f) / a - W / (2.0f * a)
 *     cy = -(((float) y + 0.5f) / a - H / (2.0f * a))
 * and the ray is, per component k, with every product and sum rounded on its own (no fused multiply-add), in this order,
 *     w_k = ((right_k * cx) + (up_k * cy)) + forward_k        direction = normalize(w)        origin = eye
 * Everything after that is the reference's kernel as it stands: scene_intersect with max_distance 100000, the smooth
 * normal, shade(direction, normal) with this world-space direction, ambient_occlusion(position, normal, y * W + x),
 * the resize.  focal_length, supersampling and every other option keep their meaning.
 * The default pose -- eye (0, 0, 2), right (1, 0, 0), up (0, 1, 0), forward (0, 0, -1) -- gives the reference's rays
 * wherever cx and cy are not zero (the sum turns a cy of -0 into +0: the centre row of an image of odd height).
 *
 * The pose is fixed per upload: what an upload prepares (the walk array's margins and child order, the hit list's size,
 * the tile order, the walk intervals) is made for one view.  An eye the fast form of the walk cannot cover -- a
 * coordinate beyond 2e6, or not a number -- renders the same contract through the exact form, more slowly.
 * Ray queries (rt_hip_query.h) do not depend on the pose.
 */
#ifndef RT_HIP_CAMERA_H
#define RT_HIP_CAMERA_H

#include "rt_hip.h"
#include "rt_hip_ring.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rt_camera {
	float eye[3], right[3], up[3], forward[3];
} rt_camera;

/* The reference's camera. */
void rt_camera_default(rt_camera *out);

/* A pose at `eye` looking at `target`: an orthonormal, right-handed basis (right x up = -forward) with up in the plane of
 * the view direction and `up_hint`, computed in double and rounded to float.  RT_E_INVALID for NULL or non-finite input,
 * eye == target, and an up hint that is zero or parallel to the view direction. */
int rt_camera_look_at(const float eye[3], const float target[3], const float up_hint[3], rt_camera *out);

/* Gives the host its pose.  Before rt_upload / rt_upload_scene only: RT_E_STATE afterwards (set the camera first; a later
 * upload on the same host keeps the pose).  RT_E_INVALID for NULL; no float value is rejected.  RT_E_STATE for the hosts
 * of a frame ring (rt_ring_host): their pose is the ring's. */
int rt_set_camera(rt_host *h, const rt_camera *cam);

/* The host's pose (the reference's camera if none was set) and whether one was set.  `is_set` may be NULL. */
int rt_get_camera(const rt_host *h, rt_camera *out, int *is_set);

/* The pose of all the hosts of a ring, before rt_ring_upload / rt_ring_upload_scene (RT_E_STATE afterwards). */
int rt_ring_set_camera(rt_ring *r, const rt_camera *cam);

#ifdef __cplusplus
}
#endif

#endif
