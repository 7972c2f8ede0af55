/* rt_hip_signed.h -- signed distance queries on an uploaded scene: for points the caller supplies, or for the voxels of a
 * regular grid, the distance to the surface with a sign -- negative inside.
 *
 * Beside rt_hip_nearest.h, whose distance has no sign.  The scene is the one a render host holds after rt_upload /
 * rt_upload_scene, after rt_update_vertices, or after rt_build_scene.
 *
 * The unsigned answer is rt_hip_nearest.h's, unchanged: the minimum over all leaves of (d2, leaf), the lowest leaf among
 * equals, `found` iff distance <= max_distance.  The sign is that of the angle-weighted pseudonormal (Baerentzen, Aanaes
 * 2005) of the FEATURE of that leaf on which the nearest point lies -- a vertex, an edge or the face, as the per-leaf
 * routine's own region test names it (csrc/nearest_point.h: np_point::region; never derived from the barycentrics).
 * csrc/signed_point.h is the contract as code, compiled by the kernels and by the tests' oracle alike; in short:
 *     n^ = cross(u, v) / |cross(u, v)| per leaf (zero for a leaf without area); corner angles by sp_angle, a routine of the
 *     header's own (Kahan's form over a fixed-coefficient atan; no library function);
 *     vertex x:    the sequential binary32 sum of angle * n^ over the corners that name x, in rising leaf index, by corner;
 *     edge {x, y}: the sequential sum of n^ over the leaves' edges with that vertex pair, in rising leaf index;
 *     face:        n^.
 *     N = the feature's pseudonormal, e = q - p, g = dot(e, N): inside iff g < 0.  A point on the surface (d2 == 0), a
 *     feature without a normal (N == 0) and g == 0 are outside.
 *     signed distance = found ? (g < 0 ? -distance : distance) : +inf.
 * Incidence is by vertex INDEX, not by position: duplicate vertices that the mesh does not weld are boundaries.  Open and
 * non-manifold meshes get the same rule; "inside" means something only for closed, consistently oriented meshes (outward:
 * counter-clockwise seen from outside).  The sums run in leaf order: see rt_hip_build.h for what that means for a built scene.
 *
 * The sign table.  96 bytes per leaf (six float4: the pseudonormals of the edges AB, AC, BC and of the vertices A, B, C; n^
 * in the .w of the first three, the corner angles in the .w of the others) plus the kept incidence, 24 bytes per leaf:
 * 120 bytes per leaf in all, in device memory of the host's own; while it is being made, another 108 bytes per leaf and the
 * sort's scratch.  It is made by the first signed query after an upload or a build -- or by rt_prepare_signed_distance,
 * which keeps that out of a query's time --; after rt_update_vertices* only the normals, angles and sums are redone, by the
 * next signed query, from the kept incidence; rt_build_scene* and an upload drop all of it.  No float atomics: the words
 * are reproducible and equal to those the contract's loops give on a CPU.  Where the coordinates are no numbers the table is
 * whatever the arithmetic gives (the `coords_flag` rule of the closest-point queries applies to the walk).
 *
 * rt_signed_distance / rt_signed_distance_device are rt_closest_points' forms and rules -- errors, flags, sort,
 * RT_QUERY_MAX_RAYS, serialisation, rt_last_query_ms.  Every rt_hit_arrays field is bit-equal to what rt_closest_points
 * writes, except that `distance` carries the sign.  `feature` (one byte per point): 0 face, 1 2 3 vertex A B C, 4 5 6 edge
 * AB AC BC, 0xFF not found.  `pseudonormal4` (float4 per point): N and g; zeros where not found.
 *
 * rt_signed_distance_grid / rt_signed_distance_grid_device: voxel (i, j, k), i < dims[0], j < dims[1], k < dims[2], is the
 * point origin + (i, j, k) * spacing, each coordinate origin + float(i) * spacing, the product and the sum rounded on their
 * own.  `distance`: float[dims[2]][dims[1]][dims[0]] of signed distances, +inf where nothing lies within max_distance;
 * `leaf`: uint32 of the same shape (0xFFFFFFFF: none), or NULL.  Every voxel equals, bit for bit, what the point form
 * answers for that point.  The points are made on the device, a 4 x 4 x 4 brick per wave: there is no point array and no
 * sort, and no flags.  dims[0] dims[1] dims[2] <= 2^31.  The host form goes through the host's query scratch in slabs of
 * z-slices; rt_last_query_ms is the sum over the slabs.
 *
 * Errors: RT_E_STATE before an upload, for the hosts of a frame ring, and for a scene uploaded without its faces;
 * RT_E_INVALID as in rt_hip_nearest.h, and for a null origin, spacing or dims, a spacing that is not positive and finite, a
 * dimension of 0, more than 2^31 voxels, device outputs not 4-byte aligned (`pseudonormal4`: 16).
 *
 * Not here: the instanced form (a signed rt_instances_closest_points).  It needs only the object-space sign and the sign of
 * the transform's determinant.
 */
#ifndef RT_HIP_SIGNED_H
#define RT_HIP_SIGNED_H

#include "rt_hip_query.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rt_signed_arrays {
	rt_hit_arrays hit;    /* the record of rt_closest_points; `distance` signed */
	uint8_t *feature;     /* [n] */
	float *pseudonormal4; /* float4[n] */
} rt_signed_arrays;

/* Host memory, blocking.  points4: float4[n], .w ignored.  `out` may be NULL (nothing is written), and any of its arrays. */
int rt_signed_distance(rt_host *h, const float *points4, uint32_t n, float max_distance, uint32_t flags, const rt_signed_arrays *out);

/* Device memory on the host's device, enqueued on `hip_stream` (NULL: the host's stream); returns without waiting, except
 * that the call which makes the table waits for it. */
int rt_signed_distance_device(rt_host *h, const float *points4, uint32_t n, float max_distance, uint32_t flags, const rt_signed_arrays *out,
                              void *hip_stream);

/* origin, spacing: float[3]; dims: uint32[3] (x, y, z), all in host memory.  distance, leaf: host memory, either may be NULL. */
int rt_signed_distance_grid(rt_host *h, const float *origin, const float *spacing, const uint32_t *dims, float max_distance, float *distance,
                            uint32_t *leaf);

/* distance, leaf: device memory. */
int rt_signed_distance_grid_device(rt_host *h, const float *origin, const float *spacing, const uint32_t *dims, float max_distance,
                                   float *distance, uint32_t *leaf, void *hip_stream);

/* Makes (or refreshes) the sign table now, blocking; a no-op where it is current. */
int rt_prepare_signed_distance(rt_host *h);

/* HIP-event time of the last build or refresh of the sign table, ms (0.0 before the first). */
float rt_last_sign_build_ms(rt_host *h);

/* For tests: the sign table (made first, if need be) into `table`, 24 floats per leaf, once everything enqueued has finished. */
int rt_debug_sign_table(rt_host *h, float *table);

#ifdef __cplusplus
}
#endif
#endif
