/* rt_hip_update.h -- vertex updates: an uploaded scene refitted on the device to new vertex positions, without a new upload.
 *
 * Beside the seam (rt_hip.h), like rt_hip_query.h: for meshes that deform with a fixed topology -- skinning, cloth, a
 * simulation step, ambient occlusion or bent normals baked per animation frame.  An upload packs every record, rebuilds
 * the walk tree, makes the walk array and copies it all; an update keeps the tree's shape and makes, on the device, the
 * three arrays every query, frame layer and view walks (the exact node records, the leaf records, the shading normals)
 * for the new positions.
 *
 * What changes.  `vertices4` (four floats per vertex, the fourth ignored) replaces EVERY vertex position; `num_vertices`
 * must be the upload's.  Faces, leaf order, tree shape, `skip` and `leaf` words stay.  Every leaf record is made with the
 * float operations an upload uses (ta, u, v, n, uu, uv, vv, D, inv_d), every leaf's box is the builder's
 * min(a, min(b, c)) / max(a, max(b, c)) of its three vertices, and every inner box is the union of its children's boxes,
 * lo = min(acc, next), hi = max(acc, next) by comparison, started from the first child and taken in index order -- the
 * REFIT RULE, which also says which of two zeros of different sign a bound keeps.  rt_scene_refit applies the same rule
 * to the CPU-side scene; the records after an update carry the bits of a fresh upload of rt_scene_refit's arrays, the
 * boxes the bits of the rule.  (A refitted tree is the old tree around the new positions: after a large deformation it
 * walks more boxes than a rebuilt one.  Results never depend on it; rt_upload is the remedy.)
 *
 * Vertex normals.  `vnormals4` non-NULL: the shading normals are rewritten from it.  NULL: they STAY AS UPLOADED -- the
 * device does not recompute them (the reference's vertex normals are order-dependent float sums over the faces;
 * rt_scene_refit recomputes them on the CPU with that routine, rt_scene_vnormals returns them).
 *
 * Validation.  rt_update_vertices refuses, before anything is written, coordinates that are not finite or exceed 1e37 in
 * magnitude.  rt_update_vertices_device cannot look: such input gives boxes that the exact walk handles like any damaged
 * upload (rt_hip.h), nothing worse.  No index changes, so nothing can be read out of bounds.
 *
 * Ordering.  An update is serialised with this host's queries by the event they are serialised by among themselves, and
 * it waits, on the device, for what the host's frame stream holds: a query, layers or views call made after the update
 * returns sees the whole update, on whatever stream.  rt_update_vertices_device enqueues on `hip_stream` (NULL: the
 * host's stream) and does not wait; the arrays must stay valid until its kernels have run.  The first update of an
 * upload also copies the faces and its schedule to the device (blocking, once; an upload allocates and copies exactly
 * what it did without this header).
 *
 * What an update closes.  rt_render, rt_render_async and everything else that walks the padded walk array or uses what
 * an upload prepares for its one view (hit-list size, claim orders, walk intervals: rt_expect_frames, the calibrations of
 * rt_hip_debug.h) fail with RT_E_STATE after an update until the next rt_upload: remaking that state is the CPU work an
 * update exists to avoid.  rt_render_layers and rt_render_views keep working -- they are the way to images of an
 * updated scene -- and so does every query family.
 *
 * Errors: RT_E_STATE before an upload, and on a host whose scene on the device is shared with another host -- the hosts
 * of a frame ring (rt_ring_host) --: a shared scene stays one copy with many readers; RT_E_INVALID for NULL `vertices4`,
 * a vertex count other than the upload's, device arrays not 16-byte aligned, and (host memory) a refused coordinate.
 */
#ifndef RT_HIP_UPDATE_H
#define RT_HIP_UPDATE_H

#include "rt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host memory, blocking. */
int rt_update_vertices(rt_host *h, const float *vertices4, const float *vnormals4, uint32_t num_vertices);

/* Device memory on the host's device, enqueued on `hip_stream` (NULL: the host's stream). */
int rt_update_vertices_device(rt_host *h, const float *vertices4, const float *vnormals4, uint32_t num_vertices, void *hip_stream);

/* The same refit on the CPU-side scene: `vertices` replaced, `vnormals` recomputed (compute_vertex_normals), `aabbs` refitted
 * by the rule where the scene has a BVH; nodes, triangles, faces and sorted faces untouched.  Refuses what
 * rt_update_vertices refuses.  Keeps the CPU arrays in step with the device. */
int rt_scene_refit(rt_scene *s, const float *vertices4, uint32_t num_vertices);

/* HIP-event time of the last update's kernels in ms (0 before the first). */
float rt_last_update_ms(const rt_host *h);

#ifdef __cplusplus
}
#endif
#endif
