/* instance_nearest.h -- the arithmetic of the instanced closest-point queries (include/rt_hip_instance_nearest.h), written
 * ONCE: the world triangle of a pair (instance, leaf), the three-key order of the answers, and the predicate that lets a walk
 * pass a box of the scene's own tree by while it stands in a copy's object space.  Plain C beside nearest_point.h, for the
 * same three compilers: kernels/instance_nearest.hip.h (the device), tests/instance_nearest_oracle.c (the brute-force
 * oracle) and tests/instance_nearest_margin_check.cc (the proof's sweep and a host-side walk).  Every operation is an IEEE
 * binary32 + - * / sqrt rounded on its own: compile with -ffp-contract=off.  No HIP headers.
 *
 * The world triangle.  With the rows (w0 w1 w2 w3) of world_from_object AS THE CALLER GAVE IT and what the device holds of
 * the leaf (ta, u, v of TriRec):
 *     ta'.x = ((w0 ta.x + w1 ta.y) + w2 ta.z) + w3        u'.x = (w0 u.x + w1 u.y) + w2 u.z        v' as u'
 * y and z from rows 1 and 2; uu' = dot(u', u'), uv' = dot(u', v'), vv' = dot(v', v') (np_dot), D' = uv' uv' - uu' vv'.  The
 * per-pair routine is np_nearest(tri', q) with the world point q, unchanged.
 */
#ifndef OCRT_INSTANCE_NEAREST_H
#define OCRT_INSTANCE_NEAREST_H

#include "nearest_point.h"

/* The rows of one affine map, [A | t]: row r is (m[r][0] m[r][1] m[r][2] | m[r][3]). */
typedef struct inp_rows {
	float m[3][4];
} inp_rows;

/* What the host makes of instance k beside its inverse (instances.cc, instance_bounds), one float4:
 *   scale   <= the smallest singular value of A_k and <= 1 / |N|_2, N the 3 x 3 part of the binary32 inverse O_k; 0 where
 *              either underflows: nothing is passed by in that copy
 *   per_q, fixed   the object point's slack is  per_q max|q_i| + fixed  (inp_slack)
 *   world   the world triangle's own rounding, a length */
typedef struct inp_bounds {
	float scale, per_q, fixed, world;
} inp_bounds;

OCRT_NP_FN np_tri inp_world_tri(const inp_rows w, const np_tri o) {
	np_tri t;
	t.tax = ((w.m[0][0] * o.tax + w.m[0][1] * o.tay) + w.m[0][2] * o.taz) + w.m[0][3];
	t.tay = ((w.m[1][0] * o.tax + w.m[1][1] * o.tay) + w.m[1][2] * o.taz) + w.m[1][3];
	t.taz = ((w.m[2][0] * o.tax + w.m[2][1] * o.tay) + w.m[2][2] * o.taz) + w.m[2][3];
	t.ux = (w.m[0][0] * o.ux + w.m[0][1] * o.uy) + w.m[0][2] * o.uz;
	t.uy = (w.m[1][0] * o.ux + w.m[1][1] * o.uy) + w.m[1][2] * o.uz;
	t.uz = (w.m[2][0] * o.ux + w.m[2][1] * o.uy) + w.m[2][2] * o.uz;
	t.vx = (w.m[0][0] * o.vx + w.m[0][1] * o.vy) + w.m[0][2] * o.vz;
	t.vy = (w.m[1][0] * o.vx + w.m[1][1] * o.vy) + w.m[1][2] * o.vz;
	t.vz = (w.m[2][0] * o.vx + w.m[2][1] * o.vy) + w.m[2][2] * o.vz;
	t.uu = np_dot(t.ux, t.uy, t.uz, t.ux, t.uy, t.uz);
	t.uv = np_dot(t.ux, t.uy, t.uz, t.vx, t.vy, t.vz);
	t.vv = np_dot(t.vx, t.vy, t.vz, t.vx, t.vy, t.vz);
	t.D = t.uv * t.uv - t.uu * t.vv;
	return t;
}

/* The object-space point of q in a copy: rt_hip_instances.h's formula for the object origin, with the rows of O. */
OCRT_NP_FN void inp_object_point(const inp_rows o, float qx, float qy, float qz, float *ox, float *oy, float *oz) {
	*ox = ((o.m[0][0] * qx + o.m[0][1] * qy) + o.m[0][2] * qz) + o.m[0][3];
	*oy = ((o.m[1][0] * qx + o.m[1][1] * qy) + o.m[1][2] * qz) + o.m[1][3];
	*oz = ((o.m[2][0] * qx + o.m[2][1] * qy) + o.m[2][2] * qz) + o.m[2][3];
}

/* The answer is the minimum of (d2, instance, leaf) over all pairs: whether (d2, instance, leaf) replaces the record.  The
 * record starts at (+inf, anything): a d2 of +inf or NaN never replaces it. */
OCRT_NP_FN int inp_better(float d2, uint32_t instance, uint32_t leaf, float best_d2, uint32_t best_instance, uint32_t best_leaf) {
	const int lower = instance < best_instance || (instance == best_instance && leaf < best_leaf);
	return d2 < best_d2 || (d2 == best_d2 && lower && d2 < INFINITY);
}

/* The pruning bound, in two spaces.  u = 2^-24; reals unless fl() says otherwise.
 *
 * World space: the REACH r of a lane is the r of np_limit2 before its squaring, for the d2 a pair must not exceed to matter
 * (the record's, or max_distance's) and the magnitude M_w of q and the TOP-LEVEL ROOT BOX:
 *     r = sqrt(bound_d2) (1 + 2^-18) + (2^-16 M_w + 2^-60).
 * nearest_point.h proves: a triangle INSIDE a box, with d2f <= bound_d2 by np_nearest, has box distance B <= sqrt(bound_d2)
 * (1 + 8u) + 33u M + 2^-73 =: R <= r (1 - 50u), so a box with np_box_d2 > r r holds none.
 *
 * (W) A top-level box is passed by on np_prune(np_box_d2(box, q), r r), with no further margin.  The world triangle tri' is
 *     not the exact image of the object triangle: per component ta' is 4 roundings off -- at most 4.01u S_k with S_k = sum_j
 *     |W_kj| max(|lo_j|, |hi_j|) + |W_k3| over the scene's root box --, u' carries the 2u max|coordinate| of u = fl(tb - ta)
 *     through A and adds 3 roundings: at most 8.02u S_k, v' the same.  A point ta' + u' s + v' t, s + t <= 1 + 2u, is hence
 *     within 12.1u S_k of the exact image per component.  The exact image lies in the exact bounds of the root box's eight
 *     corners under W, and a top-level leaf box is those bounds pushed out by instance_margin >= 2^-20 G = 64u max_k S_k
 *     (instances.cc): tri' -- with ta' + u' and ta' + v' as its other two vertices, so that nearest_point.h's "stored u is
 *     fl(tb - ta)" term is 0 -- lies INSIDE the top-level leaf box and every box above it.  The proof applies as it stands.
 *
 * (O) Inside copy k the walk holds the binary32 object point q'_f = fl(O q) (inp_object_point) against the scene's own boxes.
 *     Let N, m be the 3 x 3 part and the offset of the binary32 O, q'' = N q + m in exact arithmetic, E = N A - I.  For a
 *     point x of the object triangle and its exact image p = A x + t:
 *         N (q - p) = (q'' - x) - E x - (m + N t),   so   |q - p| >= (|q'' - x| - |E x| - |m + N t|) / |N|_2.
 *     |q'_f - q''| <= sqrt(3) 4.01u max_j (sum_l |N_jl| |q_l| + |m_j|): three rounded products and three rounded sums per
 *     component.  With   slack >= |q'_f - q''| + max_x |E x| + |m + N t|   and   scale <= 1 / |N|_2:
 *         every world distance into an object box is at least  scale (B_o - slack),  B_o the distance from q'_f to the box;
 *     tri' is within sqrt(3) 12.1u S = 21u S of the exact image (S = max_k S_k), which takes `world` >= 21u S off.  A box
 *     may be passed by when  scale (B_o - slack) - world > R,  i.e.  B_o > (R + world) / scale + slack.  inp_object_limit2
 *     squares  r_o = ((r + world) / scale) (1 + 2^-18) + (slack + 2^-60):  r >= R (1 + 50u), its own five roundings cost 6u
 *     relative, and np_box_d2's bf <= B_o^2 (1 + 6u) + 3 2^-149 (nearest_point.h, (i)) another 3u and 2^-73 -- the 64u and the
 *     2^-60 pay for all of it, and the host's figures are generous on their own: per_q = 2^-20 max_j sum_l |N_jl| and the
 *     2^-20 max_j |m_j| inside `fixed` are 16u where sqrt(3) 4.01u = 6.95u is needed, world = 2^-19 S is 32u for 21u.
 *     scale = 0 gives r_o = +inf: nothing is passed by.  A NaN anywhere gives a NaN limit, and `x > NaN` passes nothing by.
 * The margins only decide where a walk looks; tests/instance_nearest_margin_check.cc sweeps them. */
OCRT_NP_FN float inp_reach(float bound_d2, float magnitude) {
	return sqrtf(bound_d2) * (1.0f + 0x1.0p-18f) + (magnitude * 0x1.0p-16f + 0x1.0p-60f);
}
/* ... with the bound given as a distance (max_distance). */
OCRT_NP_FN float inp_reach_of_distance(float distance, float magnitude) {
	return distance * (1.0f + 0x1.0p-18f) + (magnitude * 0x1.0p-16f + 0x1.0p-60f);
}
/* The object point's slack for a lane: q_max = max |q_i| of the WORLD point. */
OCRT_NP_FN float inp_slack(const inp_bounds b, float q_max) { return b.per_q * q_max + b.fixed; }
/* What np_box_d2 of q'_f against a box of the scene's own tree is held against inside copy k (np_prune). */
OCRT_NP_FN float inp_object_limit2(float reach, const inp_bounds b, float slack) {
	const float r = ((reach + b.world) / b.scale) * (1.0f + 0x1.0p-18f) + (slack + 0x1.0p-60f);
	return r * r;
}

#endif
