/* rt_hip_instance_build.h -- device-side instance sets: transforms in device memory in, the inverses, the closest-point
 * bounds and the top-level tree made on the device.
 *
 * Beside rt_hip_instances.h, whose setter takes host memory and plans on the host.  The two entry points below make the
 * same kind of set -- every instanced query of rt_hip_instances.h, rt_hip_instance_segments.h, rt_hip_instance_views.h,
 * rt_hip_instance_nearest.h, rt_hip_instance_multihit.h and rt_hip_instance_directional.h runs on it unchanged, by its
 * own rules, on the tree the library built -- but the host never sees transforms, inverses, boxes or tree: a simulation
 * whose poses live in a device tensor hands that tensor over.  rt_set_instances and everything it returns are unchanged.
 *
 * Which form to prefer (DESIGN.md 28 has the figures, MI355X): with the poses in device memory, this one at every size
 * measured -- a step of 1000 instances takes 0.13 ms against 1.7 ms for a download and rt_set_instances, 2^20 instances
 * 6.3 ms against 2 s.  It saves the host planner (one thread, O(n log n)) and three uploads; it costs a fixed handful of
 * kernel launches and one small blocking read.  Poses that are already in HOST memory, and sets below 1000, were not
 * measured.  The two trees differ -- a radix tree over Morton keys here, a median split there --; on a 10 x 10 x 10 grid
 * the queries ran 2 to 7 % faster on this one, other sets were not measured.  Where the CPU oracle walks both trees its
 * records are equal word for word for rays with finite components: boxes along a path are unions of the same leaf boxes.
 *
 * Per instance, the numbers are rt_hip_instances.h's, operation for operation in binary64 (csrc/instance_plan.h is the
 * one text both compilers take; no fused multiply-add on either side):
 *   - O = object_from_world by the adjugate formula of rt_hip_instances.h, refused by its three rules (an entry that is
 *     not finite, a zero determinant, an entry of the rounded inverse that is not finite);
 *   - the leaf box by instance_box: the bounds of the eight corners of the scene's root box (node 0 as it lies on the
 *     device) under W, pushed outward by the margin with G = 4 x the SET's reach, then to binary32 outward;
 *   - the four floats of the closest-point walk's bounds (rt_hip_instance_nearest.h) by instance_bound.
 * Every operation involved (+ - * / sqrt, fabs, comparisons, the conversion to binary32, nextafterf) is correctly rounded
 * on both sides: O, boxes and bounds equal rt_instance_plan_lbvh's BIT FOR BIT, and O and the leaf boxes equal what
 * rt_set_instances makes of the same transforms.
 *
 * The tree.  2n - 1 records of rt_hip_instances.h's format in pre-order; n == 1 gives one leaf record.
 *   - The tree's root box is the per-axis minimum and maximum of the leaf boxes.
 *   - Keys (rt_hip_build.h's, csrc/lbvh.h): per axis, in binary32 without contraction, c = (lo + hi) * 0.5f of the leaf box
 *     and cell = clamp((c - root_lo) * (1024.0f / (root_hi - root_lo)), 0, 1023) truncated, 0 where the extent is not
 *     positive and finite or the value is not a number; the key is the 30-bit Morton interleave, x highest.
 *   - The order is the stable sort by key: equal keys in rising instance index.
 *   - The shape is the binary radix tree over the 62-bit words key << 32 | i, i the rank in that order: the node over
 *     ranks [l, r] splits behind the last rank that shares with l the highest bit in which the words of l and r differ.
 *   - The layout is pre-order: skip = 2 (r - l + 1) - 1; a leaf record has skip 1 and `leaf` = the INSTANCE INDEX (not
 *     its rank); an inner record has leaf = 0xFFFFFFFF and, per axis, lo = the smaller of its children's lo and hi = the
 *     larger of their hi, by comparison (equal values: the first child's).
 *   - A scene root box with a coordinate that is not finite gives every leaf (-inf, +inf), as rt_set_instances does; all
 *     keys are then 0 and the order is by index.
 *
 * Refusals.  The first kernel checks every transform and raises a flag in device memory; planning goes into a spare
 * allocation; the call reads the flag and the tree's root record (36 bytes) where it waits anyway.  On a raised flag it
 * returns RT_E_INVALID and the host's set -- on the device and in every getter -- is exactly what it was.  RT_E_INVALID
 * too for a null pointer, a device pointer that is not 16-byte aligned and n > RT_INSTANCES_MAX; RT_E_STATE on the hosts
 * of a frame ring.
 *
 * Sizes at which the device path changes (tests/test_thresholds_gpu.py crosses each; DESIGN.md "Size thresholds").  More
 * than 65 536 instances -- more than 256 workgroups -- reduce the set's reach and the tree's root box in launches of their
 * own; below that every workgroup of the next kernel reduces the partials for itself.  The sort of the (key, index)
 * pairs is rocPRIM's: one block up to 1 024 pairs, block sort and merge up to 2^20.  RT_INSTANCES_MAX IS 2^20: the check
 * above refuses the first size at which that sort would run its third path (onesweep), so an instance set never takes
 * it -- a scene build does (rt_hip_build.h has no such limit).  Raising RT_INSTANCES_MAX puts that path under the stable
 * order above; a test has to cross it then.
 *
 * Ordering.  As a build (rt_hip_build.h): the call is serialised with this host's queries by their event, enqueued on
 * `hip_stream` (NULL: the host's stream), and blocks for the one small read.  The caller's array may be reused on return:
 * the library keeps a copy of the transforms in memory of its own.
 *
 * Lifetime.  Either form REPLACES the host's set, whichever call made it, and rt_set_instances replaces a built one;
 * n == 0 clears the set.  A built set persists across rt_update_vertices, rt_build_scene and uploads: it is planned
 * again ON THE DEVICE, from its device-resident transforms and the new node 0, before the next instanced query or
 * getter -- that refuses nothing, validity does not depend on the root box.  Before an upload the call checks and keeps
 * the transforms; boxes and tree are made at the first use.
 */
#ifndef RT_HIP_INSTANCE_BUILD_H
#define RT_HIP_INSTANCE_BUILD_H

#include "rt_hip_instances.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Device memory on the host's device, float[n][12], 16-byte aligned. */
int rt_build_instances_device(rt_host *h, const float *world_from_object, uint32_t n, void *hip_stream);
/* Host memory: one upload, then the same device path. */
int rt_build_instances(rt_host *h, const float *world_from_object, uint32_t n);

/* What a set holds, whichever call made it (a built set's arrays are read from the device; the calls wait for the host's
 * queries).  world_from_object: the transforms as given.  rt_instance_bounds: the closest-point walk's four floats per
 * instance; RT_E_STATE before an upload or without a set, and the set is planned again first if the scene changed, as for
 * rt_instance_nodes.  `out` NULL: nothing is written. */
int rt_instances_world_from_object(rt_host *h, float *out /* [n][12] */);
int rt_instance_bounds(rt_host *h, float *out /* [n][4] */);
/* HIP-event time of the planning launches of the last device-side plan (a build or a refresh); 0: none yet. */
float rt_last_instance_build_ms(rt_host *h);

/* The same plan on the host, no device: the inverses, the tree above and the bounds for a scene whose root box is
 * (root_lo, root_hi).  O_out float[n][12], nodes_out record[2n - 1], bounds_out float[n][4]; any may be NULL.
 * RT_E_INVALID for n == 0, n > RT_INSTANCES_MAX, null inputs and a refused transform: nothing is written then. */
int rt_instance_plan_lbvh(const float root_lo[3], const float root_hi[3], const float *world_from_object, uint32_t n, float *O_out,
                          void *nodes_out, float *bounds_out);

#ifdef __cplusplus
}
#endif
#endif
