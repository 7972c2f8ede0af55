/* signed_point.h -- the sign of the signed distance queries (include/rt_hip_signed.h), written ONCE beside nearest_point.h:
 * plain C that the kernels (kernels/signed.hip.h) and the tests' brute-force oracle (tests/signed_oracle.c) both compile.
 * Every operation is an IEEE binary32 + - * / sqrt rounded on its own: compile with -ffp-contract=off.  No libm function
 * whose result may differ between host and device is called: the corner angles come from sp_angle below.
 *
 * The unsigned answer is nearest_point.h's and stays what it is: (d2, leaf) minimal, lowest leaf among equals.  The sign is
 * that of the angle-weighted pseudonormal (Baerentzen, Aanaes: "Signed distance computation using the angle weighted
 * pseudonormal", 2005) of the FEATURE of the winning leaf on which the nearest point lies: np_point::region, as the test
 * that was taken names it (vertex A, B, C; edge AB, AC, BC; face).
 *
 * Per leaf, from the values the device holds (ta, u = tb - ta, v = tc - ta):
 *     n  = cross(u, v) = (uy vz - uz vy,  uz vx - ux vz,  ux vy - uy vx)
 *     nn = dot(n, n);   n^ = n / sqrt(nn) per component, and (0, 0, 0) where nn is not positive and finite
 *     w  = v - u  (edge BC, rounded once)
 *     the corner angles  A = sp_angle(u, v),  B = sp_angle(-u, w),  C = sp_angle(v, w)   (-v and -w enclose what v and w do)
 * sp_angle(a, b) is Kahan's form  2 atan(|a |b| - b |a|| / |a |b| + b |a||)  with la = sqrt(dot(a, a)), lb = sqrt(dot(b, b)),
 * x = a lb - b la, y = a lb + b la per component, r = sqrt(dot(x, x)) / sqrt(dot(y, y)), and sp_atan: for r > tan(3 pi / 8)
 * pi/2 + P(-1 / r), for r > tan(pi / 8) pi/4 + P((r - 1) / (r + 1)), else P(r), P(z) = z + z z^2 (c0 + z^2 (c1 + z^2 (c2 +
 * z^2 c3))) evaluated by Horner's rule with the four constants below (the classic single-precision minimax fit, good to
 * 2 ulp or so).  A denominator that is not positive gives pi (a and b opposed) where the numerator is positive, else 0.
 *
 * Pseudonormals.  Incidence is by vertex INDEX, not by position: two vertices at one place that the mesh does not weld are
 * two vertices, and the edges between them are boundaries.
 *   vertex x            the sequential binary32 sum, from (0, 0, 0), of angle * n^ (per component) over the corners that name
 *                       x, in rising leaf index and by corner (A, B, C) within a leaf
 *   edge {x, y}         undirected, x != y or not: the sequential sum of n^ over the edges (AB, AC, BC of every leaf) whose
 *                       vertex pair is {x, y}, in rising leaf index, by edge within a leaf -- both leaves of a shared edge
 *                       read the same words
 *   face                n^
 * The sums run in LEAF order: a scene built on the device orders its leaves otherwise than an upload of the same triangles,
 * and the last bits of the sums may differ between the two (include/rt_hip_build.h).
 *
 * Sign.  N = the feature's pseudonormal, e = q - p per component as np_at forms it, g = np_dot(e, N).  The point is inside
 * (negative) iff g < 0; d2 == 0, N == 0 and g == 0 (and a g that is no number) are outside.  Signed distance =
 * found ? (g < 0 ? -distance : distance) : +inf.  Open and non-manifold meshes get the same rule; "inside" MEANS something
 * only for closed, consistently oriented meshes (outward normals: counter-clockwise seen from outside).
 */
#ifndef OCRT_SIGNED_POINT_H
#define OCRT_SIGNED_POINT_H

#include "nearest_point.h"

typedef struct sp_vec {
	float x, y, z;
} sp_vec;

/* What the sign reads of a leaf: n^ and the three corner angles. */
typedef struct sp_leaf {
	sp_vec n;
	float angle[3];
} sp_leaf;

OCRT_NP_FN sp_vec sp_make(float x, float y, float z) {
	sp_vec r;
	r.x = x; r.y = y; r.z = z;
	return r;
}

OCRT_NP_FN float sp_length(const sp_vec a) { return sqrtf(np_dot(a.x, a.y, a.z, a.x, a.y, a.z)); }

/* P(z) on |z| <= tan(pi / 8). */
OCRT_NP_FN float sp_atan_poly(float z) {
	const float zz = z * z;
	float p = 8.05374449538e-2f;
	p = p * zz + -1.38776856032e-1f;
	p = p * zz + 1.99777106478e-1f;
	p = p * zz + -3.33329491539e-1f;
	return z + (z * zz) * p;
}

/* atan(r) for r >= 0 (+inf: pi / 2). */
OCRT_NP_FN float sp_atan(float r) {
	if (r > 2.414213562373095f)
		return 1.5707963267948966f + sp_atan_poly(-1.0f / r);
	if (r > 0.4142135623730950f)
		return 0.7853981633974483f + sp_atan_poly((r - 1.0f) / (r + 1.0f));
	return sp_atan_poly(r);
}

/* The angle a and b enclose, in [0, pi]; 0 where either has no length. */
OCRT_NP_FN float sp_angle(const sp_vec a, const sp_vec b) {
	const float la = sp_length(a), lb = sp_length(b);
	const sp_vec x = sp_make(a.x * lb - b.x * la, a.y * lb - b.y * la, a.z * lb - b.z * la);
	const sp_vec y = sp_make(a.x * lb + b.x * la, a.y * lb + b.y * la, a.z * lb + b.z * la);
	const float num = sp_length(x), den = sp_length(y);
	if (!(den > 0.0f))
		return num > 0.0f ? 3.14159265358979f : 0.0f;
	return 2.0f * sp_atan(num / den);
}

OCRT_NP_FN sp_leaf sp_leaf_of(const np_tri tri) {
	const sp_vec u = sp_make(tri.ux, tri.uy, tri.uz), v = sp_make(tri.vx, tri.vy, tri.vz);
	const sp_vec w = sp_make(v.x - u.x, v.y - u.y, v.z - u.z);
	const sp_vec n = sp_make(u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x);
	const float nn = np_dot(n.x, n.y, n.z, n.x, n.y, n.z);
	sp_leaf r;
	r.n = sp_make(0.0f, 0.0f, 0.0f);
	if (nn > 0.0f && nn < INFINITY) {
		const float len = sqrtf(nn);
		r.n = sp_make(n.x / len, n.y / len, n.z / len);
	}
	r.angle[0] = sp_angle(u, v);
	r.angle[1] = sp_angle(sp_make(-u.x, -u.y, -u.z), w);
	r.angle[2] = sp_angle(v, w);
	return r;
}

/* One more term of a vertex's sum, and of an edge's. */
OCRT_NP_FN sp_vec sp_add_corner(const sp_vec sum, const sp_leaf leaf, int corner) {
	const float a = corner == 0 ? leaf.angle[0] : corner == 1 ? leaf.angle[1] : leaf.angle[2];  /* (no indexed array on the device) */
	return sp_make(sum.x + a * leaf.n.x, sum.y + a * leaf.n.y, sum.z + a * leaf.n.z);
}
OCRT_NP_FN sp_vec sp_add_normal(const sp_vec sum, const sp_leaf leaf) {
	return sp_make(sum.x + leaf.n.x, sum.y + leaf.n.y, sum.z + leaf.n.z);
}

/* The vertex pair of edge 0, 1, 2 = AB, AC, BC of a face (three vertex ids) as one key: (min, max). */
OCRT_NP_FN uint64_t sp_edge_key(const uint32_t *face, int edge) {
	const uint32_t x = face[edge == 2 ? 1 : 0], y = face[edge == 0 ? 1 : 2];
	return x < y ? ((uint64_t) x << 32) | y : ((uint64_t) y << 32) | x;
}

/* The sign table's record of a leaf: six float4.  xyz: the pseudonormals of the edges AB, AC, BC and of the vertices A, B, C;
 * .w of the edges: n^ x, y, z (the face's own); .w of the vertices: the corner angles. */
enum { SP_REC_FLOATS = 24 };

/* The float4 of a record that holds the pseudonormal of a vertex or edge `region`: NP_EDGE_AB .. BC = 4 .. 6 are float4
 * 0 .. 2, NP_VERTEX_A .. C = 1 .. 3 are float4 3 .. 5. */
OCRT_NP_FN int sp_slot(int region) { return region >= NP_EDGE_AB ? region - NP_EDGE_AB : region + 2; }

/* The pseudonormal of `region` (NP_*) out of a record. */
OCRT_NP_FN sp_vec sp_pseudonormal(const float *rec, int region) {
	if (region == NP_FACE)
		return sp_make(rec[3], rec[7], rec[11]);
	return sp_make(rec[4 * sp_slot(region)], rec[4 * sp_slot(region) + 1], rec[4 * sp_slot(region) + 2]);
}

/* g: negative iff q lies inside. */
OCRT_NP_FN float sp_side(float qx, float qy, float qz, float px, float py, float pz, const sp_vec n) {
	const float ex = qx - px, ey = qy - py, ez = qz - pz;
	return np_dot(ex, ey, ez, n.x, n.y, n.z);
}

#endif
