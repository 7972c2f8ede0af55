// instances.cc -- the planner of an instance set (instances.h, include/rt_hip_instances.h).  Host only.
#include "instances.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "../../include/rt_hip_instances.h"

namespace ocrt {

// The header's formula, operation by operation in binary64 (this file is compiled without contraction).
bool instance_inverse(const float W[12], float O[12]) {
	for (int k = 0; k < 12; ++k)
		if (!std::isfinite(W[k]))
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
	for (int r = 0; r < 3; ++r) {
		const double q0 = adj[r][0] / det, q1 = adj[r][1] / det, q2 = adj[r][2] / det;
		const double q3 = -((q0 * x + q1 * y) + q2 * z);
		out[4 * r + 0] = (float) q0;
		out[4 * r + 1] = (float) q1;
		out[4 * r + 2] = (float) q2;
		out[4 * r + 3] = (float) q3;
	}
	for (int k = 0; k < 12; ++k)
		if (!std::isfinite(out[k]))
			return false;
	std::copy(out, out + 12, O);
	return true;
}

bool instance_inverses(const float *W, uint32_t n, std::vector<float> &O) {
	std::vector<float> made((size_t) n * 12u);
	for (uint32_t k = 0; k < n; ++k)
		if (!instance_inverse(W + 12u * (size_t) k, made.data() + 12u * (size_t) k))
			return false;
	O.swap(made);
	return true;
}

namespace {

// The largest magnitude a coordinate of the root box's image under W, or a partial sum of it, can have:
// max_k (sum_j |A_kj| max(|root_lo_j|, |root_hi_j|) + |t_k|).
double instance_reach(const float root_lo[3], const float root_hi[3], const float W[12]) {
	double S = 0.0;
	for (int k = 0; k < 3; ++k) {
		double T = std::fabs((double) W[4 * k + 3]);
		for (int j = 0; j < 3; ++j)
			T += std::fabs((double) W[4 * k + j]) * std::max(std::fabs((double) root_lo[j]), std::fabs((double) root_hi[j]));
		S = std::max(S, T);
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
double instance_margin(const float W[12], const float O[12], int k, double G) {
	double sum = G;
	for (int j = 0; j < 3; ++j) {
		const double q = (std::fabs((double) O[4 * j + 0]) + std::fabs((double) O[4 * j + 1]) + std::fabs((double) O[4 * j + 2])) * G +
		                 std::fabs((double) O[4 * j + 3]);
		sum += std::fabs((double) W[4 * k + j]) * q;
	}
	return sum * 0x1.0p-20;
}

float outward_down(double v) {
	const float f = (float) v;
	return std::nextafterf(f, -std::numeric_limits<float>::infinity());
}
float outward_up(double v) {
	const float f = (float) v;
	return std::nextafterf(f, std::numeric_limits<float>::infinity());
}

void instance_box(const float root_lo[3], const float root_hi[3], const float W[12], const float O[12], double G, InstanceNode &node) {
	const float inf = std::numeric_limits<float>::infinity();
	bool finite = true;
	for (int k = 0; k < 3; ++k)
		finite = finite && std::isfinite(root_lo[k]) && std::isfinite(root_hi[k]);
	if (!finite) {
		for (int k = 0; k < 3; ++k)
			node.lo[k] = -inf, node.hi[k] = inf;
		return;
	}
	for (int k = 0; k < 3; ++k) {
		double lo = std::numeric_limits<double>::infinity(), hi = -lo;
		for (int corner = 0; corner < 8; ++corner) {
			const double x = (corner & 1) ? root_hi[0] : root_lo[0], y = (corner & 2) ? root_hi[1] : root_lo[1];
			const double z = (corner & 4) ? root_hi[2] : root_lo[2];
			const double p = (((double) W[4 * k + 0] * x + (double) W[4 * k + 1] * y) + (double) W[4 * k + 2] * z) + (double) W[4 * k + 3];
			lo = std::min(lo, p);
			hi = std::max(hi, p);
		}
		const double m = instance_margin(W, O, k, G);
		node.lo[k] = outward_down(lo - m);
		node.hi[k] = outward_up(hi + m);
	}
}

// A box's centre on an axis as a sort key: a number whatever the box holds.
double centre_key(const InstanceNode &leaf, int axis) {
	const double c = 0.5 * (double) leaf.lo[axis] + 0.5 * (double) leaf.hi[axis];
	return std::isfinite(c) ? c : 0.0;
}

// The subtree over order[first, first + count) into nodes[at, at + 2 count - 1): a median split of the centres along
// their widest axis (equal centres: by instance index), the first child behind its parent, the second behind the first.
void split(const std::vector<InstanceNode> &leaves, std::vector<uint32_t> &order, uint32_t first, uint32_t count, std::vector<InstanceNode> &nodes,
           uint32_t at) {
	if (count == 1u) {
		nodes[at] = leaves[order[first]];
		return;
	}
	int axis = 0;
	double widest = -1.0;
	for (int k = 0; k < 3; ++k) {
		double lo = std::numeric_limits<double>::infinity(), hi = -lo;
		for (uint32_t i = first; i < first + count; ++i) {
			const double c = centre_key(leaves[order[i]], k);
			lo = std::min(lo, c);
			hi = std::max(hi, c);
		}
		if (hi - lo > widest)
			widest = hi - lo, axis = k;
	}
	const uint32_t half = count / 2u;
	std::nth_element(order.begin() + first, order.begin() + first + half, order.begin() + first + count, [&](uint32_t p, uint32_t q) {
		const double cp = centre_key(leaves[p], axis), cq = centre_key(leaves[q], axis);
		return cp < cq || (cp == cq && p < q);
	});
	const uint32_t left = at + 1u, right = at + 2u * half;
	split(leaves, order, first, half, nodes, left);
	split(leaves, order, first + half, count - half, nodes, right);
	InstanceNode &node = nodes[at];
	for (int k = 0; k < 3; ++k) {
		node.lo[k] = std::min(nodes[left].lo[k], nodes[right].lo[k]);
		node.hi[k] = std::max(nodes[left].hi[k], nodes[right].hi[k]);
	}
	node.skip = 2u * count - 1u;
	node.leaf = INSTANCE_INNER;
}

// An upper bound of the largest eigenvalue of the symmetric S, and a lower bound of the smallest (not below 0): cyclic Jacobi
// sweeps, then Gershgorin's discs of what is left -- exact for the matrix the sweeps arrived at, whose spectrum is S's but
// for the rotations' roundings (a few 2^-53 of the largest entry per rotation: the 2^-40 below).
void eigen_bounds(double S[3][3], double &largest, double &smallest) {
	double peak = 0.0;
	for (int i = 0; i < 3; ++i)
		for (int j = 0; j < 3; ++j)
			peak = std::max(peak, std::fabs(S[i][j]));
	for (int sweep = 0; sweep < 8; ++sweep)
		for (int p = 0; p < 2; ++p)
			for (int q = p + 1; q < 3; ++q) {
				if (S[p][q] == 0.0)
					continue;
				const double theta = (S[q][q] - S[p][p]) / (2.0 * S[p][q]);
				const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
				const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
				for (int k = 0; k < 3; ++k) {  // S <- S J
					const double kp = S[k][p], kq = S[k][q];
					S[k][p] = c * kp - s * kq;
					S[k][q] = s * kp + c * kq;
				}
				for (int k = 0; k < 3; ++k) {  // S <- J^T S
					const double pk = S[p][k], qk = S[q][k];
					S[p][k] = c * pk - s * qk;
					S[q][k] = s * pk + c * qk;
				}
			}
	largest = -std::numeric_limits<double>::infinity();
	smallest = std::numeric_limits<double>::infinity();
	for (int i = 0; i < 3; ++i) {
		double off = 0.0;
		for (int j = 0; j < 3; ++j)
			if (j != i)
				off += 0.5 * (std::fabs(S[i][j]) + std::fabs(S[j][i]));
		largest = std::max(largest, S[i][i] + off);
		smallest = std::min(smallest, S[i][i] - off);
	}
	largest += peak * 0x1.0p-40;
	smallest = std::max(0.0, smallest - peak * 0x1.0p-40);
}

float rounded_down(double v) {  // a binary32 number <= v, not below 0
	const float f = (float) v;
	return v > 0.0 && f > 0.0f ? std::nextafterf(f, 0.0f) : 0.0f;
}

// inp_bounds of one instance (instance_nearest.h has the proof these figures serve).
void instance_bound(const float root_lo[3], const float root_hi[3], const float W[12], const float O[12], float out[4]) {
	double R[3];  // the root box's largest coordinate per axis
	bool finite = true;
	for (int j = 0; j < 3; ++j) {
		finite = finite && std::isfinite(root_lo[j]) && std::isfinite(root_hi[j]);
		R[j] = std::max(std::fabs((double) root_lo[j]), std::fabs((double) root_hi[j]));
	}
	// scale: min(sigma_min(A), 1 / |N|_2), from the eigenvalues of A^T A and N^T N
	double AtA[3][3], NtN[3][3];
	for (int i = 0; i < 3; ++i)
		for (int j = 0; j < 3; ++j) {
			AtA[i][j] = NtN[i][j] = 0.0;
			for (int k = 0; k < 3; ++k) {
				AtA[i][j] += (double) W[4 * k + i] * W[4 * k + j];
				NtN[i][j] += (double) O[4 * k + i] * O[4 * k + j];
			}
		}
	double a_hi, a_lo, n_hi, n_lo;
	eigen_bounds(AtA, a_hi, a_lo);
	eigen_bounds(NtN, n_hi, n_lo);
	const double sigma = std::sqrt(a_lo) * (1.0 - 0x1.0p-40), by_inverse = n_hi > 0.0 ? (1.0 - 0x1.0p-40) / std::sqrt(n_hi) : 0.0;
	out[0] = finite ? rounded_down(std::min(sigma, by_inverse)) : 0.0f;
	// the object point's slack: the roundings of fl(O q) (16u, 6.95u needed), |E x| over the root box, |m + N t|
	double per_q = 0.0, offset = 0.0, e1 = 0.0, e2 = 0.0;
	for (int i = 0; i < 3; ++i) {
		per_q = std::max(per_q, std::fabs((double) O[4 * i]) + std::fabs((double) O[4 * i + 1]) + std::fabs((double) O[4 * i + 2]));
		offset = std::max(offset, std::fabs((double) O[4 * i + 3]));
		double row = 0.0;  // sum_j |E_ij| R_j, the binary64 evaluation's own error (2^-50 of the absolute sums) included
		for (int j = 0; j < 3; ++j) {
			double e = i == j ? -1.0 : 0.0, mass = i == j ? 1.0 : 0.0;
			for (int l = 0; l < 3; ++l) {
				e += (double) O[4 * i + l] * W[4 * l + j];
				mass += std::fabs((double) O[4 * i + l] * W[4 * l + j]);
			}
			row += (std::fabs(e) + mass * 0x1.0p-50) * R[j];
		}
		e1 += row * row;
		double r = O[4 * i + 3], mass = std::fabs(r);  // (m + N t)_i
		for (int l = 0; l < 3; ++l) {
			r += (double) O[4 * i + l] * W[4 * l + 3];
			mass += std::fabs((double) O[4 * i + l] * W[4 * l + 3]);
		}
		r = std::fabs(r) + mass * 0x1.0p-50;
		e2 += r * r;
	}
	out[1] = outward_up(per_q * 0x1.0p-20);
	out[2] = outward_up(offset * 0x1.0p-20 + (std::sqrt(e1) + std::sqrt(e2)) * (1.0 + 0x1.0p-40));
	// the world triangle's rounding: 32u S (21u needed), S the instance's reach
	out[3] = outward_up(instance_reach(root_lo, root_hi, W) * 0x1.0p-19);
	for (int k = 1; k < 4; ++k)
		if (!finite || !std::isfinite(out[k]))
			out[0] = 0.0f;  // (nothing is passed by)
}

}  // namespace

void instance_bounds(const float root_lo[3], const float root_hi[3], const float *W, const float *O, uint32_t n, std::vector<float> &bounds) {
	bounds.assign((size_t) n * 4u, 0.0f);
	for (uint32_t k = 0; k < n; ++k)
		instance_bound(root_lo, root_hi, W + 12u * (size_t) k, O + 12u * (size_t) k, bounds.data() + 4u * (size_t) k);
}

void instance_tree(const float root_lo[3], const float root_hi[3], const float *W, const float *O, uint32_t n, std::vector<InstanceNode> &nodes) {
	std::vector<InstanceNode> leaves(n);
	std::vector<uint32_t> order(n);
	double reach = 0.0;  // (of the whole set: the margin's G, instance_margin)
	for (uint32_t k = 0; k < n; ++k)
		reach = std::max(reach, instance_reach(root_lo, root_hi, W + 12u * (size_t) k));
	for (uint32_t k = 0; k < n; ++k) {
		instance_box(root_lo, root_hi, W + 12u * (size_t) k, O + 12u * (size_t) k, 4.0 * reach, leaves[k]);
		leaves[k].skip = 1u;
		leaves[k].leaf = k;
		order[k] = k;
	}
	nodes.assign(2u * (size_t) n - 1u, InstanceNode{});
	split(leaves, order, 0u, n, nodes, 0u);
}

}  // namespace ocrt

extern "C" int rt_instance_plan(const float root_lo[3], const float root_hi[3], const float *world_from_object, uint32_t n, float *O_out,
                                void *nodes_out) {
	if (!root_lo || !root_hi || !world_from_object || n == 0u || n > RT_INSTANCES_MAX)
		return RT_E_INVALID;
	try {
		std::vector<float> O;
		if (!ocrt::instance_inverses(world_from_object, n, O))
			return RT_E_INVALID;
		if (nodes_out) {
			std::vector<ocrt::InstanceNode> nodes;
			ocrt::instance_tree(root_lo, root_hi, world_from_object, O.data(), n, nodes);
			std::memcpy(nodes_out, nodes.data(), nodes.size() * sizeof(ocrt::InstanceNode));
		}
		if (O_out)
			std::copy(O.begin(), O.end(), O_out);
		return RT_OK;
	} catch (...) {
		return RT_E_INVALID;
	}
}
