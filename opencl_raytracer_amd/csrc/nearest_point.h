/* nearest_point.h -- the arithmetic of the closest-point queries (include/rt_hip_nearest.h), written ONCE: the nearest point
 * of one leaf's triangle, the distance from a point to a box, and the predicate that lets a walk pass a box by.  Plain C that
 * three compilers take: kernels/nearest.hip.h (the device), tests/nearest_oracle.c (the brute-force oracle) and
 * tests/nearest_margin_check.cc (the proof's sweep and a host-side walk).  Every operation is an IEEE binary32 + - * / sqrt
 * rounded on its own: compile with -ffp-contract=off.  No HIP headers.
 *
 * The per-leaf routine, in the order it is evaluated (include/rt_hip_nearest.h states the same text):
 *     w  = q - ta                          d1 = dot(u, w)      d2 = dot(v, w)       dot(a, b) = (ax bx + ay by) + az bz
 *     d3 = d1 - uu     d4 = d2 - uv        d5 = d1 - uv        d6 = d2 - vv
 *   vertex A   d1 <= 0 and d2 <= 0                                          (s, t) = (0, 0)
 *   vertex B   d3 >= 0 and d4 <= d3                                         (s, t) = (1, 0)
 *   edge AB    vc = uu d2 - uv d1;   uu > 0, vc <= 0, d1 >= 0, d3 <= 0      (s, t) = (d1 / uu, 0)
 *   vertex C   d6 >= 0 and d5 <= d6                                         (s, t) = (0, 1)
 *   edge AC    vb = vv d1 - uv d2;   vv > 0, vb <= 0, d2 >= 0, d6 <= 0      (s, t) = (0, d2 / vv)
 *   edge BC    va = d3 d6 - d5 d4;   g = d4 - d3, h = d5 - d6, gh = g + h;
 *              gh > 0, va <= 0, g >= 0, h >= 0                              k = g / gh, (s, t) = (1 - k, k)
 *   face       m = -D; solve(r1, r2): if uu >= vv, t = (uu r2 - uv r1) / m and s = (r1 - uv t) / uu; else s = (vv r1 - uv r2) / m
 *              and t = (r2 - uv s) / vv.  (s0, t0) = solve(d1, d2); p0, e0 of (s0, t0) as below; (ds, dt) = solve(dot(u, e0),
 *              dot(v, e0)); s = s0 + ds, t = t0 + dt -- one step of refinement: on a sliver m keeps a few digits only --;
 *              taken if m > 0, s >= 0, t >= 0 and s + t <= 1
 *   otherwise  (a face without area, or one whose vb, vc, D are rounding noise) the nearest of the three edges as segments,
 *              tried in the order AB, AC, BC, an edge of no length standing for its first vertex; the first of equals stays.
 *   p = ta + (u s + v t) per component,  e = q - p,  d2 = dot(e, e),  distance = sqrt(d2).
 * The first region whose test holds is taken.  Every region's (s, t) has s, t >= 0 and, up to one rounding, s + t <= 1:
 * whatever the tests decide on a sliver, p is a point OF the triangle, and d2 can err towards "farther" only by the choice
 * of region, never by leaving the surface.  Degenerate triangles need nothing else: an edge of no length (uu, vv or gh = 0)
 * is skipped and its vertices' regions, tried before it, stand; a triangle of no area (D = 0, or of the wrong sign) fails
 * `m > 0` and falls to its edges.  For finite inputs below 1e9 in magnitude no product overflows and d2 is a number.
 * A triangle with a coordinate that is no number, or infinite, gives a d2 that is NaN or +inf: u s + v t multiplies every
 * component of u and v, so no (s, t) hides one.  Such a d2 never replaces a record (np_better).
 */
#ifndef OCRT_NEAREST_POINT_H
#define OCRT_NEAREST_POINT_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define OCRT_NP_FN __host__ __device__ inline
#elif defined(__cplusplus)
#define OCRT_NP_FN inline
#else
#define OCRT_NP_FN static inline
#endif

/* What the routine reads of a leaf: TriRec's ta, u, v, uu, uv, vv, D (device_types.h). */
typedef struct np_tri {
	float tax, tay, taz, ux, uy, uz, vx, vy, vz, uu, uv, vv, D;
} np_tri;

/* `region`: the feature of the triangle the point lies on, as the test that was taken names it -- never derived from
 * (s, t): in the BC region 1 - s - t is not exactly 0.  The signed queries read it (signed_point.h); no distance does. */
enum { NP_FACE = 0, NP_VERTEX_A = 1, NP_VERTEX_B = 2, NP_VERTEX_C = 3, NP_EDGE_AB = 4, NP_EDGE_AC = 5, NP_EDGE_BC = 6 };

typedef struct np_point {
	float s, t, px, py, pz, d2;
	int region;
} np_point;

OCRT_NP_FN float np_dot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

/* p, e and d2 for the parameters (s, t). */
OCRT_NP_FN np_point np_at(const np_tri tri, float qx, float qy, float qz, float s, float t) {
	np_point r;
	r.s = s;
	r.t = t;
	r.region = NP_FACE;
	r.px = tri.tax + (tri.ux * s + tri.vx * t);
	r.py = tri.tay + (tri.uy * s + tri.vy * t);
	r.pz = tri.taz + (tri.uz * s + tri.vz * t);
	{
		const float ex = qx - r.px, ey = qy - r.py, ez = qz - r.pz;
		r.d2 = np_dot(ex, ey, ez, ex, ey, ez);
	}
	return r;
}

/* A projection's parameter on an edge as a segment: num / den within [0, 1]; 0 for an edge of no length or a NaN. */
OCRT_NP_FN float np_clamped(float num, float den) {
	float k;
	if (!(den > 0.0f))
		return 0.0f;
	k = num / den;
	if (!(k >= 0.0f))
		return 0.0f;
	return k > 1.0f ? 1.0f : k;
}

/* Parameters, and whether they are a region's. */
typedef struct np_params {
	float s, t;
	int found, region;
} np_params;

/* The parameters of the vertex or edge region whose test holds first; found = 0 where none did (np_face then). */
OCRT_NP_FN np_params np_region(const np_tri tri, float d1, float d2) {
	const float uu = tri.uu, uv = tri.uv, vv = tri.vv;
	const float d3 = d1 - uu, d4 = d2 - uv, d5 = d1 - uv, d6 = d2 - vv;
	const float vc = uu * d2 - uv * d1, vb = vv * d1 - uv * d2, va = d3 * d6 - d5 * d4;
	const float g = d4 - d3, h = d5 - d6, gh = g + h;
	np_params r;
	r.s = 0.0f;
	r.t = 0.0f;
	r.found = 1;
	r.region = NP_FACE;
	if (d1 <= 0.0f && d2 <= 0.0f) {
		r.s = 0.0f, r.t = 0.0f, r.region = NP_VERTEX_A;
	} else if (d3 >= 0.0f && d4 <= d3) {
		r.s = 1.0f, r.t = 0.0f, r.region = NP_VERTEX_B;
	} else if (uu > 0.0f && vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
		r.s = d1 / uu, r.t = 0.0f, r.region = NP_EDGE_AB;
	} else if (d6 >= 0.0f && d5 <= d6) {
		r.s = 0.0f, r.t = 1.0f, r.region = NP_VERTEX_C;
	} else if (vv > 0.0f && vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
		r.s = 0.0f, r.t = d2 / vv, r.region = NP_EDGE_AC;
	} else if (gh > 0.0f && va <= 0.0f && g >= 0.0f && h >= 0.0f) {
		const float k = g / gh;
		r.s = 1.0f - k, r.t = k, r.region = NP_EDGE_BC;
	} else {
		r.found = 0;
	}
	return r;
}

/* The face's normal equations  uu s + uv t = r1,  uv s + vv t = r2:  the unknown of the SHORTER edge by Cramer's rule, the
 * other one from the longer edge's own equation -- on a sliver (uu vv next to uv uv: m keeps a few digits) the error of the
 * first then moves the point across the sliver only, not along it.  (`found` is not set.) */
OCRT_NP_FN np_params np_solve(const np_tri tri, float m, float r1, float r2) {
	np_params r;
	r.found = 0;
	r.region = NP_FACE;
	if (tri.uu >= tri.vv) {
		const float t = (tri.uu * r2 - tri.uv * r1) / m;
		r.t = t;
		r.s = (r1 - tri.uv * t) / tri.uu;
	} else {
		const float s = (tri.vv * r1 - tri.uv * r2) / m;
		r.s = s;
		r.t = (r2 - tri.uv * s) / tri.vv;
	}
	return r;
}

/* The face region: np_solve for (d1, d2), then ONE step of refinement -- the residual e = q - p of that point, the same solve
 * for (dot(u, e), dot(v, e)), added --; found: the result is a point of the face. */
OCRT_NP_FN np_params np_face(const np_tri tri, float qx, float qy, float qz, float d1, float d2) {
	const float m = -tri.D;
	const np_params first = np_solve(tri, m, d1, d2);
	const np_point at = np_at(tri, qx, qy, qz, first.s, first.t);
	const float ex = qx - at.px, ey = qy - at.py, ez = qz - at.pz;
	const np_params step = np_solve(tri, m, np_dot(tri.ux, tri.uy, tri.uz, ex, ey, ez), np_dot(tri.vx, tri.vy, tri.vz, ex, ey, ez));
	np_params r;
	r.s = first.s + step.s;
	r.t = first.t + step.t;
	r.region = NP_FACE;
	r.found = m > 0.0f && r.s >= 0.0f && r.t >= 0.0f && r.s + r.t <= 1.0f;
	return r;
}

/* The feature a clamped parameter k of an edge stands for: the edge, or its end vertex where the clamp hit 0 or 1 (an edge
 * of no length has k = 0: its first vertex). */
OCRT_NP_FN int np_edge_region(float k, int edge, int first, int second) { return k == 0.0f ? first : k == 1.0f ? second : edge; }

/* The nearest of the three edges as segments, in the order AB, AC, BC; the first of equals stays, a NaN never replaces. */
OCRT_NP_FN np_point np_edges(const np_tri tri, float qx, float qy, float qz, float d1, float d2) {
	const float d3 = d1 - tri.uu, d4 = d2 - tri.uv, d5 = d1 - tri.uv, d6 = d2 - tri.vv;
	const float g = d4 - d3, h = d5 - d6;
	const float k = np_clamped(g, g + h), kab = np_clamped(d1, tri.uu), kac = np_clamped(d2, tri.vv);
	np_point best = np_at(tri, qx, qy, qz, kab, 0.0f);
	np_point ac = np_at(tri, qx, qy, qz, 0.0f, kac);
	np_point bc = np_at(tri, qx, qy, qz, 1.0f - k, k);
	best.region = np_edge_region(kab, NP_EDGE_AB, NP_VERTEX_A, NP_VERTEX_B);
	ac.region = np_edge_region(kac, NP_EDGE_AC, NP_VERTEX_A, NP_VERTEX_C);
	bc.region = np_edge_region(k, NP_EDGE_BC, NP_VERTEX_B, NP_VERTEX_C);
	if (ac.d2 < best.d2)
		best = ac;
	if (bc.d2 < best.d2)
		best = bc;
	return best;
}

/* The routine: the nearest point of the leaf's triangle to q. */
OCRT_NP_FN np_point np_nearest(const np_tri tri, float qx, float qy, float qz) {
	const float wx = qx - tri.tax, wy = qy - tri.tay, wz = qz - tri.taz;
	const float d1 = np_dot(tri.ux, tri.uy, tri.uz, wx, wy, wz), d2 = np_dot(tri.vx, tri.vy, tri.vz, wx, wy, wz);
	np_params r = np_region(tri, d1, d2);
	if (!r.found)
		r = np_face(tri, qx, qy, qz, d1, d2);
	if (r.found) {
		np_point p = np_at(tri, qx, qy, qz, r.s, r.t);
		p.region = r.region;
		return p;
	}
	return np_edges(tri, qx, qy, qz, d1, d2);
}

/* The answer is the minimum of (d2, leaf) over all leaves: whether (d2, leaf) replaces the record (best_d2, best_leaf).
 * The record starts at (+inf, anything): a d2 of +inf or NaN never replaces it. */
OCRT_NP_FN int np_better(float d2, uint32_t leaf, float best_d2, uint32_t best_leaf) {
	return d2 < best_d2 || (d2 == best_d2 && leaf < best_leaf && d2 < INFINITY);
}

/* Whether a query looks at anything at all: a radius that is a number >= 0 and a point of three finite coordinates. */
OCRT_NP_FN int np_radius_ok(float max_distance) { return max_distance >= 0.0f; }
OCRT_NP_FN int np_point_ok(float qx, float qy, float qz) {
	return fabsf(qx) < INFINITY && fabsf(qy) < INFINITY && fabsf(qz) < INFINITY;
}

/* The squared distance from q to the box [lo, hi]: per axis max(lo - q, q - hi, 0) -- fmaxf drops a NaN, so a bound that
 * is no number constrains nothing --, then dot.  Monotone in the box: a box inside another is never nearer. */
OCRT_NP_FN float np_box_d2(float lox, float loy, float loz, float hix, float hiy, float hiz, float qx, float qy, float qz) {
	const float dx = fmaxf(fmaxf(lox - qx, qx - hix), 0.0f);
	const float dy = fmaxf(fmaxf(loy - qy, qy - hiy), 0.0f);
	const float dz = fmaxf(fmaxf(loz - qz, qz - hiz), 0.0f);
	return np_dot(dx, dy, dz, dx, dy, dz);
}

/* The pruning bound.  A walk may pass by a box whose np_box_d2 exceeds np_limit2(bound_d2, magnitude), where bound_d2 is the
 * d2 a triangle must not exceed to matter -- the record's, or max_distance squared -- and `magnitude` bounds every
 * coordinate in play: |q|'s and those of the box (of the scene's root box, which holds every nested box).
 *
 * Proof (u = 2^-24; reals unless fl() says otherwise).  Let a triangle lie in the box, T its true distance from q, B the
 * box's, so T >= B; let d2f be the routine's result for it, bf its np_box_d2, M the magnitude.
 *  (i)  bf <= B^2 (1 + 6u) + 3 2^-149.  Each axis term is fl of ONE difference (or an exact 0), relative error <= u; its
 *       square adds u, the two sums add u each; a square that underflows loses at most 2^-149.
 *  (ii) T <= sqrt(d2f) (1 + 4u) + 32u M.  The routine's (s, t) has s, t >= 0 and s + t <= 1 + 2u, so P = ta + (tb - ta) s +
 *       (tc - ta) t is a point of the triangle but for 2u |extent| <= 4u M per component: |q - P| >= T - 7u M.  The stored
 *       u, v are fl(tb - ta), fl(tc - ta): per component u (|u_k| s + |v_k| t) <= 2u M off.  p adds two products (u each),
 *       their sum (u) and the sum with ta (u): <= u (2 + 1 + 1) 2M = 8u M.  e = fl(q - p): relative u.  So per component
 *       e_k = (q - P)_k (1 + delta) + eta with |eta| <= 10.1u M, i.e. |e| >= (T - 7u M)(1 - u) - 17.5u M, and d2f =
 *       fl(dot(e, e)) >= |e|^2 (1 - u)^5.  Together sqrt(d2f) >= (1 - 3.6u)(T - 25u M).
 *  So a triangle of the box with d2f <= bound_d2 has  sqrt(bf - 3 2^-149) (1 - 3u) <= B <= T <= sqrt(bound_d2)(1 + 4u) + 32u M:
 *  passing the box by is safe whenever  sqrt(bf) > sqrt(bound_d2)(1 + 8u) + 33u M + 2^-73.  np_limit2 squares a right-hand
 *  side that is generous instead -- a = 2^-18 = 64u, b = 2^-16 M + 2^-60 = 256u M + ... --, which also pays for its own four
 *  roundings (4u relative) and for max_distance standing in for a bound: sqrtf(d2f) <= max_distance implies sqrt(d2f) <=
 *  max_distance (1 + u).  The margin only decides where the walk looks; tests/nearest_margin_check.cc sweeps it.
 *  (+inf in, +inf out: nothing is passed by.  A NaN magnitude or bound gives NaN, and `x > NaN` passes nothing by.) */
OCRT_NP_FN float np_limit2(float bound_d2, float magnitude) {
	const float r = sqrtf(bound_d2) * (1.0f + 0x1.0p-18f) + (magnitude * 0x1.0p-16f + 0x1.0p-60f);
	return r * r;
}
/* ... with the bound given as a distance (max_distance). */
OCRT_NP_FN float np_limit2_of_distance(float distance, float magnitude) {
	const float r = distance * (1.0f + 0x1.0p-18f) + (magnitude * 0x1.0p-16f + 0x1.0p-60f);
	return r * r;
}
/* The predicate: true = no triangle inside this box can replace or tie the record, nor lie within the radius. */
OCRT_NP_FN int np_prune(float box_d2, float limit2) { return box_d2 > limit2; }

/* max |coordinate| of a point and a box: the `magnitude` above. */
OCRT_NP_FN float np_magnitude(float lox, float loy, float loz, float hix, float hiy, float hiz, float qx, float qy, float qz) {
	const float b = fmaxf(fmaxf(fmaxf(fabsf(lox), fabsf(hix)), fmaxf(fabsf(loy), fabsf(hiy))), fmaxf(fabsf(loz), fabsf(hiz)));
	return fmaxf(b, fmaxf(fmaxf(fabsf(qx), fabsf(qy)), fabsf(qz)));
}

#endif
