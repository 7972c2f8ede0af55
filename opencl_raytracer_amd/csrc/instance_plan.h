// instance_plan.h -- the arithmetic of an instance set, per instance (include/rt_hip_instances.h, include/rt_hip_instance_build.h):
// the inverse of a transform and what refuses it, an instance's reach, the margin and the leaf box of the top-level tree, the
// closest-point walk's bounds (instance_nearest.h, inp_bounds) and the outward roundings.  Written ONCE here, as functions both
// compilers take: instances.cc and instance_build.cc call them with a loop, kernels/instance_build.hip.h with a lane per
// instance.  Every operation is an IEEE binary64 + - * / sqrt, fabs, a comparison, the conversion to binary32 or nextafterf,
// each rounded on its own (both compilers run without contraction): the device's numbers are the host's.  No HIP headers.
#pragma once
#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#define OCRT_INSTANCE_FN __host__ __device__ inline
#define OCRT_INSTANCE_UNROLL _Pragma("unroll")
#else
#define OCRT_INSTANCE_FN inline
#define OCRT_INSTANCE_UNROLL
#endif

namespace ocrt {

// (std::min / std::max / std::isfinite, spelled out: the second argument wins only where it is strictly beyond the first)
OCRT_INSTANCE_FN double instance_min(double a, double b) { return b < a ? b : a; }
OCRT_INSTANCE_FN double instance_max(double a, double b) { return a < b ? b : a; }
OCRT_INSTANCE_FN bool instance_finite(float v) { return ::fabsf(v) <= 3.4028234663852886e38f; }  // (false for a NaN too)
OCRT_INSTANCE_FN bool instance_finite(double v) { return ::fabs(v) <= 1.7976931348623157e308; }
OCRT_INSTANCE_FN float instance_infinity() { return __builtin_inff(); }

// object_from_world of one transform by the header's formula, operation by operation in binary64; false where the header
// refuses the transform (`O` untouched).
OCRT_INSTANCE_FN bool instance_inverse(const float W[12], float O[12]) {
	for (int k = 0; k < 12; ++k)
		if (!instance_finite(W[k]))
			return false;
	const double a = W[0], b = W[1], c = W[2], x = W[3];
	const double d = W[4], e = W[5], f = W[6], y = W[7];
	const double g = W[8], h = W[9], i = W[10], z = W[11];
	const double adj[3][3] = { { e * i - f * h, c * h - b * i, b * f - c * e },
		                       { f * g - d * i, a * i - c * g, c * d - a * f },
		                       { d * h - e * g, b * g - a * h, a * e - b * d } };
	const double det = (a * adj[0][0] + b * adj[1][0]) + c * adj[2][0];
	if (!(det != 0.0))  // (a NaN cannot arise from finite binary32 entries: the products stay far below binary64's range)
		return false;
	float out[12];
	OCRT_INSTANCE_UNROLL
	for (int r = 0; r < 3; ++r) {
		const double q0 = adj[r][0] / det, q1 = adj[r][1] / det, q2 = adj[r][2] / det;
		const double q3 = -((q0 * x + q1 * y) + q2 * z);
		out[4 * r + 0] = (float) q0;
		out[4 * r + 1] = (float) q1;
		out[4 * r + 2] = (float) q2;
		out[4 * r + 3] = (float) q3;
	}
	for (int k = 0; k < 12; ++k)
		if (!instance_finite(out[k]))
			return false;
	for (int k = 0; k < 12; ++k)
		O[k] = out[k];
	return true;
}

// The largest magnitude a coordinate of the root box's image under W, or a partial sum of it, can have:
// max_k (sum_j |A_kj| max(|root_lo_j|, |root_hi_j|) + |t_k|).
OCRT_INSTANCE_FN double instance_reach(const float root_lo[3], const float root_hi[3], const float W[12]) {
	double S = 0.0;
	OCRT_INSTANCE_UNROLL
	for (int k = 0; k < 3; ++k) {
		double T = ::fabs((double) W[4 * k + 3]);
		OCRT_INSTANCE_UNROLL
		for (int j = 0; j < 3; ++j)
			T += ::fabs((double) W[4 * k + j]) * instance_max(::fabs((double) root_lo[j]), ::fabs((double) root_hi[j]));
		S = instance_max(S, T);
	}
	return S;
}

// The outward margin of an instance's leaf box on axis k, in world units.
//
// What the box must do: a ray / triangle pair that the float64 judge of the tests calls clearly accepted -- the EXACT world
// ray (o, d) meets the triangle's exact image at a point x = o + r d, r >= 0, strictly inside it -- must not be culled at
// this box by the binary32 slab test of the reference (src/intersect_kernel.cl:21-61).  x lies in the exact image of the
// scene's root box (the root box holds every triangle), hence inside the exact bounds [lo, hi] of its eight corners.
// With u = 2^-24, S the instance's reach (instance_reach: no coordinate of a corner's image and no partial sum of it exceeds
// S) and G = 4 max(S over the whole SET) -- the margin scales with the set, not with the copy, so that a copy near the world's
// origin is covered for rays that start at the far end of a wide set --, for rays with |o|_inf <= G (every point of the
// top-level root box, and of that box grown 1.25 x about its centre, is such an origin: its coordinates stay below 2.25 G / 4):
//  1. The corners in binary64.  The products of two binary32 numbers are exact in binary64; the three sums round once each:
//     a corner's coordinate is off by at most 3 * 2^-53 S <= 2^-27 u G.
//  2. The slab test.  A plane's parameter is fl(fl(P - o_k) * fl(1 / d_k)): three roundings, so the computed value is the
//     exact (P - o_k) / d_k times a factor within 1 +- 3.01 u, its sign kept.  On an axis whose exact near parameter is
//     <= 0 the computed one is <= 0 <= r.  Otherwise the exact near parameter of the plane pushed out by m is at most
//     r - m / |d_k|, and its computed value stays <= r when m >= 3.01 u r |d_k| = 3.01 u |x_k - o_k|; the far plane
//     likewise stays >= r, and > 0 because m > 0.  Every computed near value <= r <= every computed far value: none of
//     the test's `near > far` comparisons fires, t_max > 0 holds, and t_min < max_distance holds because the judge asks for
//     the entry parameter of the triangle's OWN box -- which the ray reaches no sooner than this box, a superset of that
//     box's image -- to be below max_distance (1 - 1e-4) - 1e-6.  |x_k - o_k| <= S + |o_k| <= 2 G: m >= 6.02 u G.
//  3. The rounding of O and of the object ray.  The lane does not walk the exact object ray.  Component j of its origin is
//     ((O_j0 o.x + O_j1 o.y) + O_j2 o.z) + O_j3 with every O_jl within u |O_jl| of the exact inverse's entry and three
//     rounded sums: off by at most 4.01 u (sum_l |O_jl| |o_l| + |O_j3|) <= 4.01 u q_j, q_j = (|O_j0| + |O_j1| + |O_j2|) G +
//     |O_j3|.  Its direction is off by 3.01 u sum_l |O_jl| |d_l|, which at the parameter r moves the point by at most
//     3.01 u sum_l |O_jl| |r d|_inf <= 3.01 u 2 q_j.  Mapped back by A, the point the lane's ray reaches at r lies within
//     e_k = sum_j |A_kj| (4.01 + 6.02) u q_j <= 10.03 u sum_j |A_kj| q_j of x on axis k: a hit the lane finds belongs to a
//     world point that far from the exact ray at most, and the box holds that point's neighbourhood too.
// m_k = 2^-20 (G + sum_j |A_kj| q_j) = 16 u (...) covers 1, 2 and 3 with room to spare: four parts in a million of the SET's
// reach.  The bounds then go to binary32 OUTWARD: the conversion rounds to nearest, one step further out undoes it.
// Beyond |o|_inf <= G the slab test's own rounding grows with the origin's distance, as it does at the scene's own boxes in
// every query of this library and in the reference: no box of a fixed size covers it (include/rt_hip_instances.h says so).
OCRT_INSTANCE_FN double instance_margin(const float W[12], const float O[12], int k, double G) {
	double sum = G;
	OCRT_INSTANCE_UNROLL
	for (int j = 0; j < 3; ++j) {
		const double q = (::fabs((double) O[4 * j + 0]) + ::fabs((double) O[4 * j + 1]) + ::fabs((double) O[4 * j + 2])) * G +
		                 ::fabs((double) O[4 * j + 3]);
		sum += ::fabs((double) W[4 * k + j]) * q;
	}
	return sum * 0x1.0p-20;
}

OCRT_INSTANCE_FN float outward_down(double v) {
	const float f = (float) v;
	return ::nextafterf(f, -instance_infinity());
}
OCRT_INSTANCE_FN float outward_up(double v) {
	const float f = (float) v;
	return ::nextafterf(f, instance_infinity());
}

// The leaf box of one instance: the bounds of the root box's eight corners under W, pushed out by the margin (G: four times
// the SET's reach).  A root box that is not finite: (-inf, +inf).
OCRT_INSTANCE_FN void instance_box(const float root_lo[3], const float root_hi[3], const float W[12], const float O[12], double G, float lo_out[3],
                                   float hi_out[3]) {
	const float inf = instance_infinity();
	bool finite = true;
	for (int k = 0; k < 3; ++k)
		finite = finite && instance_finite(root_lo[k]) && instance_finite(root_hi[k]);
	if (!finite) {
		for (int k = 0; k < 3; ++k)
			lo_out[k] = -inf, hi_out[k] = inf;
		return;
	}
	OCRT_INSTANCE_UNROLL
	for (int k = 0; k < 3; ++k) {
		double lo = (double) inf, hi = -lo;
		OCRT_INSTANCE_UNROLL
		for (int corner = 0; corner < 8; ++corner) {
			const double x = (corner & 1) ? root_hi[0] : root_lo[0], y = (corner & 2) ? root_hi[1] : root_lo[1];
			const double z = (corner & 4) ? root_hi[2] : root_lo[2];
			const double p = (((double) W[4 * k + 0] * x + (double) W[4 * k + 1] * y) + (double) W[4 * k + 2] * z) + (double) W[4 * k + 3];
			lo = instance_min(lo, p);
			hi = instance_max(hi, p);
		}
		const double m = instance_margin(W, O, k, G);
		lo_out[k] = outward_down(lo - m);
		hi_out[k] = outward_up(hi + m);
	}
}

// An upper bound of the largest eigenvalue of the symmetric S, and a lower bound of the smallest (not below 0): cyclic Jacobi
// sweeps, then Gershgorin's discs of what is left -- exact for the matrix the sweeps arrived at, whose spectrum is S's but
// for the rotations' roundings (a few 2^-53 of the largest entry per rotation: the 2^-40 below).
OCRT_INSTANCE_FN void eigen_bounds(double S[3][3], double &largest, double &smallest) {
	double peak = 0.0;
	OCRT_INSTANCE_UNROLL
	for (int i = 0; i < 3; ++i) {
		OCRT_INSTANCE_UNROLL
		for (int j = 0; j < 3; ++j)
			peak = instance_max(peak, ::fabs(S[i][j]));
	}
	for (int sweep = 0; sweep < 8; ++sweep) {
		OCRT_INSTANCE_UNROLL
		for (int p = 0; p < 2; ++p) {
			OCRT_INSTANCE_UNROLL
			for (int q = p + 1; q < 3; ++q) {
				if (S[p][q] == 0.0)
					continue;
				const double theta = (S[q][q] - S[p][p]) / (2.0 * S[p][q]);
				const double t = (theta >= 0.0 ? 1.0 : -1.0) / (::fabs(theta) + ::sqrt(theta * theta + 1.0));
				const double c = 1.0 / ::sqrt(t * t + 1.0), s = t * c;
				OCRT_INSTANCE_UNROLL
				for (int k = 0; k < 3; ++k) {  // S <- S J
					const double kp = S[k][p], kq = S[k][q];
					S[k][p] = c * kp - s * kq;
					S[k][q] = s * kp + c * kq;
				}
				OCRT_INSTANCE_UNROLL
				for (int k = 0; k < 3; ++k) {  // S <- J^T S
					const double pk = S[p][k], qk = S[q][k];
					S[p][k] = c * pk - s * qk;
					S[q][k] = s * pk + c * qk;
				}
			}
		}
	}
	largest = -(double) instance_infinity();
	smallest = (double) instance_infinity();
	OCRT_INSTANCE_UNROLL
	for (int i = 0; i < 3; ++i) {
		double off = 0.0;
		OCRT_INSTANCE_UNROLL
		for (int j = 0; j < 3; ++j)
			if (j != i)
				off += 0.5 * (::fabs(S[i][j]) + ::fabs(S[j][i]));
		largest = instance_max(largest, S[i][i] + off);
		smallest = instance_min(smallest, S[i][i] - off);
	}
	largest += peak * 0x1.0p-40;
	smallest = instance_max(0.0, smallest - peak * 0x1.0p-40);
}

OCRT_INSTANCE_FN float rounded_down(double v) {  // a binary32 number <= v, not below 0
	const float f = (float) v;
	return v > 0.0 && f > 0.0f ? ::nextafterf(f, 0.0f) : 0.0f;
}

// inp_bounds of one instance (instance_nearest.h has the proof these figures serve).
OCRT_INSTANCE_FN void instance_bound(const float root_lo[3], const float root_hi[3], const float W[12], const float O[12], float out[4]) {
	double R[3];  // the root box's largest coordinate per axis
	bool finite = true;
	OCRT_INSTANCE_UNROLL
	for (int j = 0; j < 3; ++j) {
		finite = finite && instance_finite(root_lo[j]) && instance_finite(root_hi[j]);
		R[j] = instance_max(::fabs((double) root_lo[j]), ::fabs((double) root_hi[j]));
	}
	// scale: min(sigma_min(A), 1 / |N|_2), from the eigenvalues of A^T A and N^T N
	double AtA[3][3], NtN[3][3];
	OCRT_INSTANCE_UNROLL
	for (int i = 0; i < 3; ++i) {
		OCRT_INSTANCE_UNROLL
		for (int j = 0; j < 3; ++j) {
			AtA[i][j] = NtN[i][j] = 0.0;
			OCRT_INSTANCE_UNROLL
			for (int k = 0; k < 3; ++k) {
				AtA[i][j] += (double) W[4 * k + i] * W[4 * k + j];
				NtN[i][j] += (double) O[4 * k + i] * O[4 * k + j];
			}
		}
	}
	double a_hi, a_lo, n_hi, n_lo;
	eigen_bounds(AtA, a_hi, a_lo);
	eigen_bounds(NtN, n_hi, n_lo);
	const double sigma = ::sqrt(a_lo) * (1.0 - 0x1.0p-40), by_inverse = n_hi > 0.0 ? (1.0 - 0x1.0p-40) / ::sqrt(n_hi) : 0.0;
	out[0] = finite ? rounded_down(instance_min(sigma, by_inverse)) : 0.0f;
	// the object point's slack: the roundings of fl(O q) (16u, 6.95u needed), |E x| over the root box, |m + N t|
	double per_q = 0.0, offset = 0.0, e1 = 0.0, e2 = 0.0;
	OCRT_INSTANCE_UNROLL
	for (int i = 0; i < 3; ++i) {
		per_q = instance_max(per_q, ::fabs((double) O[4 * i]) + ::fabs((double) O[4 * i + 1]) + ::fabs((double) O[4 * i + 2]));
		offset = instance_max(offset, ::fabs((double) O[4 * i + 3]));
		double row = 0.0;  // sum_j |E_ij| R_j, the binary64 evaluation's own error (2^-50 of the absolute sums) included
		OCRT_INSTANCE_UNROLL
		for (int j = 0; j < 3; ++j) {
			double e = i == j ? -1.0 : 0.0, mass = i == j ? 1.0 : 0.0;
			OCRT_INSTANCE_UNROLL
			for (int l = 0; l < 3; ++l) {
				e += (double) O[4 * i + l] * W[4 * l + j];
				mass += ::fabs((double) O[4 * i + l] * W[4 * l + j]);
			}
			row += (::fabs(e) + mass * 0x1.0p-50) * R[j];
		}
		e1 += row * row;
		double r = O[4 * i + 3], mass = ::fabs(r);  // (m + N t)_i
		OCRT_INSTANCE_UNROLL
		for (int l = 0; l < 3; ++l) {
			r += (double) O[4 * i + l] * W[4 * l + 3];
			mass += ::fabs((double) O[4 * i + l] * W[4 * l + 3]);
		}
		r = ::fabs(r) + mass * 0x1.0p-50;
		e2 += r * r;
	}
	out[1] = outward_up(per_q * 0x1.0p-20);
	out[2] = outward_up(offset * 0x1.0p-20 + (::sqrt(e1) + ::sqrt(e2)) * (1.0 + 0x1.0p-40));
	// the world triangle's rounding: 32u S (21u needed), S the instance's reach
	out[3] = outward_up(instance_reach(root_lo, root_hi, W) * 0x1.0p-19);
	for (int k = 1; k < 4; ++k)
		if (!finite || !instance_finite(out[k]))
			out[0] = 0.0f;  // (nothing is passed by)
}

}  // namespace ocrt
