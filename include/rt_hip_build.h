/* rt_hip_build.h -- device-side scene builds: triangles in, a scene on the device out, the tree made by the GPU.
 *
 * Beside the seam (rt_hip.h), like rt_hip_update.h: for meshes whose TOPOLOGY changes -- remeshing, fracture, an
 * iso-surface per step, a mesh that only exists as arrays on the device.  An upload has the CPU build the tree, pack every
 * record, rebuild the walk tree, make the walk array and copy it all; a build takes vertices, vertex normals and faces and
 * makes, on the device, the three arrays every query, frame layer and view walks (exact node records, leaf records, shading
 * normals), plus the options' direction table.  The CPU never sees the tree.  Results do not depend on the tree: the
 * queries of a built scene answer what they answer after an upload of the same triangles, bit for bit, except that `leaf`
 * counts in the build's leaf order (rt_built_faces) and that, of several triangles hit at exactly the same distance, the
 * one with the lowest leaf index is reported, which is another face where the orders differ; and that the signed distance
 * queries' sign table (rt_hip_signed.h) sums a vertex's and an edge's pseudonormal in leaf order, so that its last bits may
 * differ from an upload's -- which can change a sign only for points within the distance tolerance of the surface.
 *
 * What a build is.  It REPLACES the host's scene on the device; it may follow an upload or come first.  The new scene has
 * no padded walk array.  rt_update_vertices works on it unchanged -- the scene keeps its leaf-ordered faces, its leaf ->
 * node map and its schedule on the device, so the first update prepares nothing --, and building again is the repair for
 * a tree that updates have degraded.
 *
 * What a build closes.  Exactly what an update closes (rt_hip_update.h): rt_render, rt_render_async, rt_expect_frames and
 * the calibrations fail with RT_E_STATE until the next rt_upload; every query family, rt_render_layers, rt_render_views
 * and rt_update_vertices work.
 *
 * THE TREE (lbvh.h holds the same text next to the code; rt_scene_build_lbvh makes the same tree on the CPU-side scene).
 *  1. Leaf boxes by the refit rule of rt_hip_update.h: min(a, min(b, c)), max(a, max(b, c)) per axis, by comparison.
 *  2. The root box: per axis the minimum and maximum of the leaf boxes.
 *  3. Keys, per axis in float32, every operation rounded on its own: c = (lo + hi) * 0.5f of the leaf's box,
 *     cell = clamp((c - root_lo) * (1024.0f / (root_hi - root_lo)), 0, 1023) truncated; cell = 0 where the extent is not
 *     positive and finite or the value is not a number.  The key is the 30-bit Morton interleave of the three cells: bit
 *     3 b + 2 is bit b of the x cell, 3 b + 1 of the y cell, 3 b of the z cell.
 *  4. A stable sort of the (key, face id) pairs by key: equal keys stay in rising face id.
 *  5. Leaf i is the i-th pair; its leaf index is i.  The shape is the binary radix tree over the 62-bit keys
 *     key << 32 | i: the node over leaves [l, r] splits behind the last leaf that shares with leaf l the highest bit in
 *     which the keys of l and r differ.
 *  6. Nodes in pre-order, as the walk reads them: skip = 2 (r - l + 1) - 1; leaf = i for leaves, 0xFFFFFFFF for inner
 *     nodes; one zero record behind the last node, where an upload puts one.  (The node over [l, r] has index 2 l + the
 *     number of its proper ancestors in whose first child it lies.)
 *  7. Leaf records and shading records as an update makes them, over the faces in leaf order.
 *  8. Inner boxes by the refit rule, first child first.
 *
 * Vertex normals.  rt_build_scene with `vnormals4` NULL computes them on the CPU with the routine rt_scene_from_arrays and
 * rt_scene_refit use (order-dependent float sums over the faces).  rt_build_scene_device needs them: NULL is RT_E_INVALID.
 *
 * Validation.  rt_build_scene refuses, before anything is launched, a face index >= num_vertices and coordinates an update
 * refuses (not finite, beyond 1e37).  rt_build_scene_device cannot look at its input: its first kernel checks every index
 * BEFORE any read through it -- a bad face is built from vertex 0 and raises a flag in device memory --, the call reads the
 * flag where it waits anyway (below), returns RT_E_INVALID and leaves the host's previous scene as it was.  Nothing is read
 * out of bounds.  Coordinates are not looked at: as for rt_update_vertices_device.
 *
 * Ordering.  As an update: serialised with this host's queries by their event, behind what the host's frame stream holds,
 * and the sort's cached root box is dropped.  rt_build_scene_device enqueues on `hip_stream` (NULL: the host's stream) and
 * BLOCKS its caller: the inner boxes are filled by a schedule made on the host from the tree's `skip` words, which are
 * downloaded once, 4 bytes per node, when the topology's kernels have run; and the scene that is replaced is freed, which
 * waits for the device.  The input arrays may be reused when the call returns.
 *
 * Errors: RT_E_STATE on a host whose scene on the device is shared with another host (the hosts of a frame ring);
 * RT_E_INVALID for NULL pointers, zero faces or vertices, 2^25 faces or more (an upload's bound), device arrays that are
 * not 16-byte aligned (faces: 4-byte), and what "Validation" lists.
 */
#ifndef RT_HIP_BUILD_H
#define RT_HIP_BUILD_H

#include "rt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host memory, blocking.  `vertices4`, `vnormals4`: four floats per vertex, the fourth ignored; `faces`: three vertex ids each. */
int rt_build_scene(rt_host *h, const float *vertices4, const float *vnormals4, uint32_t num_vertices, const uint32_t *faces,
                   uint32_t num_faces);

/* Device memory on the host's device, enqueued on `hip_stream` (NULL: the host's stream); blocks, see "Ordering". */
int rt_build_scene_device(rt_host *h, const float *vertices4, const float *vnormals4, uint32_t num_vertices, const uint32_t *faces,
                          uint32_t num_faces, void *hip_stream);

/* The file-order face of every leaf of the built scene, `num_faces` words: what a query's `leaf` stands for.  RT_E_STATE
 * where the host's scene was not built (an uploaded scene's map is rt_scene_triangles). */
int rt_built_faces(const rt_host *h, uint32_t *face_of_leaf);

/* The same tree on the CPU-side scene: nodes, aabbs, triangles and sorted faces as rt_scene_build_bvh leaves them, the
 * tree steps 1-6 and 8 describe.  rt_upload_scene takes it like any other. */
int rt_scene_build_lbvh(rt_scene *s);

/* HIP-event time of the last build's kernels in ms, the wait between its two runs of launches left out (0 before the first). */
float rt_last_build_ms(const rt_host *h);

#ifdef __cplusplus
}
#endif
#endif
