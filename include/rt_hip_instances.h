/* rt_hip_instances.h -- instanced ray queries: posed copies of the uploaded scene under a top-level tree, closest hit and
 * occlusion for rays the caller supplies.
 *
 * Beside rt_hip_query.h.  A render host holds ONE scene; an INSTANCE SET poses n copies of it in the world, each by an affine
 * map.  The two queries below cast world-space rays against all copies under the arithmetic contract (every
 * operation rounded on its own in binary32, in the order written here).  Every plain entry point -- frames, layers, views,
 * ambient occlusion, segments, multi-hit and closest-point queries -- ignores the set: nothing they compute changes when
 * one is given.  Ambient occlusion, views and segments have instanced forms of their own, defined by the rules below:
 * rt_trace_instances_ao and rt_render_instance_views (rt_hip_instance_views.h), and rt_instances_segments_occluded,
 * rt_instances_segments_closest and rt_instances_visibility_masks (rt_hip_instance_segments.h).  Closest-point queries have
 * one with rules of its own, in world space: rt_instances_closest_points (rt_hip_instance_nearest.h).  Multi-hit and
 * directional occlusion queries have theirs by the same rules: rt_trace_instances_multihit (rt_hip_instance_multihit.h) and
 * rt_trace_instances_ao_directional (rt_hip_instance_directional.h).  A set can also be made on the device, from transforms
 * in device memory: rt_build_instances_device (rt_hip_instance_build.h).
 *
 * Transforms.  world_from_object is twelve floats per instance, the rows of W = [A | t]: p_world = A p + t.  Every entry
 * must be finite, the determinant of A (binary64) non-zero and every entry of the inverse finite after its rounding to
 * binary32; otherwise rt_set_instances returns RT_E_INVALID and the host's set is what it was.
 *
 * The inverse.  The library makes O = object_from_world = [inv(A) | -inv(A) t] in binary64, each operation rounded on its
 * own, no fused multiply-add.  With A = (a b c; d e f; g h i) and t = (x y z):
 *     c00 = e i - f h    c01 = c h - b i    c02 = b f - c e
 *     c10 = f g - d i    c11 = a i - c g    c12 = c d - a f
 *     c20 = d h - e g    c21 = b g - a h    c22 = a e - b d
 *     det = (a c00 + b c10) + c c20
 *     Q[r][k] = c_rk / det                                   (the adjugate over the determinant)
 *     Q[r][3] = -((Q[r][0] x + Q[r][1] y) + Q[r][2] z)       (on the binary64 quotients)
 * and O[r][k] is Q[r][k] rounded ONCE to binary32.  These twelve floats are what the kernel uses and what
 * rt_instances_object_from_world returns.
 *
 * The top-level tree is an array of the node records the exact walk reads (32 bytes: float lo[3]; uint32 skip; float hi[3];
 * uint32 leaf): a full binary tree in pre-order, 2n - 1 records, `skip` the subtree's size in records, `leaf` the instance
 * index (0xFFFFFFFF for an inner node); sibling subtrees tile their parent's range; n == 1 gives one leaf record.  It is
 * built on the host inside rt_set_instances: a median split of the instances' box centres along the widest axis.  WHICH
 * tree is built is the library's choice; the answer below is defined on the tree the library built (rt_instance_nodes
 * reads it back), as a ray query's is on the uploaded tree.  A leaf's box is the bounds of the eight corners of the scene's
 * root box (node 0 as it is on the device) under W, computed in binary64 and pushed outward to binary32 with a margin
 * (csrc/instances.cc, instance_margin, has the bound and its argument: the margin grows with the largest coordinate of the
 * whole SET and covers the roundings of the slab test, of O and of the object ray for every ray whose origin's coordinates
 * stay within FOUR TIMES that largest coordinate in magnitude -- every origin inside the top-level root box, and well around
 * it; farther out the slab test's own rounding grows with the origin's distance, as at the scene's own boxes in every query,
 * and a ray that grazes a copy's box may miss it); an inner box is the exact minimum / maximum of its two children.  A root
 * box with a coordinate that is not finite gives every instance the box (-inf, +inf).  Boxes and tree are made again from the new root box after rt_update_vertices, rt_build_scene and a new upload, before the next
 * instanced query or rt_instance_nodes.  The set itself persists across those; it ends with n == 0 or rt_destroy.
 *
 * A query.  For ray (o, d) and the call's max_distance:
 *   - instance k is ENTERED iff every top-level box from the root to k's leaf passes the reference's aabb_intersect
 *     (src/intersect_kernel.cl:21-61) for (o, d, max_distance);
 *   - its object ray, with the rows (m0 m1 m2 m3) of O_k:  o'.x = ((m0 o.x + m1 o.y) + m2 o.z) + m3,
 *     d'.x = (m0 d.x + m1 d.y) + m2 d.z, y and z from rows 1 and 2.  An affine map keeps ray parameters and the reference
 *     culls boxes by parameter (t_min < max_distance), normalising nothing: max_distance means the same in both spaces;
 *   - its CANDIDATES are the leaves that the reference's scene_intersect walk (:184-213) of the scene's own tree accepts for
 *     (o', d', max_distance): boxes by aabb_intersect, triangles by triangle_intersect (:65-114).  A candidate has the
 *     plane parameter r = a / b (:79) and (s, t) of that object-space test;
 *   - a candidate's record: position = o + r d in WORLD space, per component o.x + r * d.x; distance = length(position - o)
 *     as the reference computes length; barycentrics (1 - s - t, s, t); leaf; instance = k.
 * Closest form: the candidate with the minimum of (distance, instance, leaf): a strictly smaller distance wins, and among
 * equal distances below +inf the lower (instance, leaf) pair.  `hit` is 1 iff there is a candidate.  A candidate but none
 * with a distance below +inf: `hit` 1 and the record keeps its entry values -- instance 0, leaf 0, distance +inf, the rest
 * 0.  No candidate: `hit` 0, instance and leaf 0xFFFFFFFF, distance +inf, the rest 0.
 * Normal: with the returned barycentrics, raw = (n0 b0 + n1 b1) + n2 b2 (get_smooth_normal before its normalisation, the
 * leaf's three vertex normals), w = transpose(O) raw with w.x = (O00 raw.x + O10 raw.y) + O20 raw.z and so on, and ONE
 * normalisation of w.  Without a hit the normal is 0.
 * Occluded form: the same boolean.
 *
 * Every float input is legal; odd rays get the rules' own answer.
 * Relation to rt_hip_query.h: with ONE instance whose transform is the identity, for rays whose six components are finite
 * and hold no -0, `occluded` equals rt_trace_occluded's, and where rt_trace_closest's hit has a distance below +inf every
 * field equals it word for word, with instance 0.  (1 * x + 0 * y turns a -0 into +0, and for a direction component that
 * flips the reference's `inv >= 0` choice of the near plane: hence the exclusion.)
 *
 * Coherence: the ray queries' sort (RT_QUERY_NO_SORT, RT_QUERY_SORT_MIN), origins quantised over the top-level root box;
 * not a bit depends on the order.  rt_last_query_ms covers these queries; frames, graphs and counters are left alone.
 *
 * Errors: RT_E_STATE before an upload, with no instances set, on the hosts of a frame ring; RT_E_INVALID as in
 * rt_hip_query.h (null ray arrays, device ray arrays not 16-byte aligned, device float / uint32 outputs not 4-byte aligned,
 * n > RT_QUERY_MAX_RAYS), for a null transform array and n > RT_INSTANCES_MAX in the setter.  n == 0 rays launches nothing.
 */
#ifndef RT_HIP_INSTANCES_H
#define RT_HIP_INSTANCES_H

#include "rt_hip_query.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_INSTANCES_MAX (1u << 20)

/* Host memory, float[n][12]; n == 0 clears the set.  May be called before an upload: the tree is made at the first use. */
int rt_set_instances(rt_host *h, const float *world_from_object, uint32_t n);
uint32_t rt_instance_count(const rt_host *h);
int rt_instances_object_from_world(rt_host *h, float *out /* [n][12] */);
uint32_t rt_instance_node_count(const rt_host *h); /* 2n - 1; 0 without a set */
/* Waits for the host's queries; makes the tree again first if the scene changed.  RT_E_STATE before an upload. */
int rt_instance_nodes(rt_host *h, void *out /* record[2n - 1] */);

typedef struct rt_instance_hit_arrays { /* any pointer may be NULL: that output is not written */
	rt_hit_arrays record;
	uint32_t *instance; /* [n] */
} rt_instance_hit_arrays;

/* Host memory, blocking.  `out` may be NULL (nothing is written). */
int rt_trace_instances_closest(rt_host *h, const float *origins4, const float *directions4, uint32_t n, float max_distance,
                               uint32_t flags, const rt_instance_hit_arrays *out);
int rt_trace_instances_occluded(rt_host *h, const float *origins4, const float *directions4, uint32_t n, float max_distance,
                                uint32_t flags, uint8_t *occluded);
/* Device memory on the host's device, enqueued on `hip_stream` (NULL: the host's stream); returns without waiting. */
int rt_trace_instances_closest_device(rt_host *h, const float *origins4, const float *directions4, uint32_t n, float max_distance,
                                      uint32_t flags, const rt_instance_hit_arrays *out, void *hip_stream);
int rt_trace_instances_occluded_device(rt_host *h, const float *origins4, const float *directions4, uint32_t n, float max_distance,
                                       uint32_t flags, uint8_t *occluded, void *hip_stream);

/* The planner alone, host only, no device: the inverses and the tree rt_set_instances would make for a scene whose root box
 * is (root_lo, root_hi).  O_out float[n][12], nodes_out record[2n - 1]; either may be NULL.  RT_E_INVALID for n == 0,
 * n > RT_INSTANCES_MAX, null inputs and a refused transform: nothing is written then. */
int rt_instance_plan(const float root_lo[3], const float root_hi[3], const float *world_from_object, uint32_t n, float *O_out,
                     void *nodes_out);

#ifdef __cplusplus
}
#endif
#endif
