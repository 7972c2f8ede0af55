// reference_tests.h -- what the CPU check programs of the walk's margins and of the pruning bound share (prune_check.cc,
// camera_margin_check.cc, prune_bound_sweep.cc): the reference's slab and triangle tests restated operation for operation
// in float (the build: -ffp-contract=off), and the kernel's own node test on a walk record.  Header only.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>

#include "device_types.h"

namespace reference_tests {

using ocrt::NodeRec;
using ocrt::TriRec;

// reference src/intersect_kernel.cl:21-61, straight
inline bool reference_slab(const float lo[3], const float hi[3], const float o[3], const float d[3], float max_distance) {
	float t_min, t_max, ty_min, ty_max, tz_min, tz_max;
	float div = 1.0f / d[0];
	if (div >= 0) { t_min = (lo[0] - o[0]) * div; t_max = (hi[0] - o[0]) * div; }
	else { t_min = (hi[0] - o[0]) * div; t_max = (lo[0] - o[0]) * div; }
	div = 1 / d[1];
	if (div >= 0) { ty_min = (lo[1] - o[1]) * div; ty_max = (hi[1] - o[1]) * div; }
	else { ty_min = (hi[1] - o[1]) * div; ty_max = (lo[1] - o[1]) * div; }
	if (t_min > ty_max || ty_min > t_max) return false;
	t_min = std::fmax(t_min, ty_min);
	t_max = std::fmin(t_max, ty_max);
	div = 1 / d[2];
	if (div >= 0) { tz_min = (lo[2] - o[2]) * div; tz_max = (hi[2] - o[2]) * div; }
	else { tz_min = (hi[2] - o[2]) * div; tz_max = (lo[2] - o[2]) * div; }
	if (t_min > tz_max || tz_min > t_max) return false;
	t_min = std::fmax(t_min, tz_min);
	t_max = std::fmin(t_max, tz_max);
	return t_min < max_distance && t_max > 0;
}

// the reference's triangle test on a TriRec (src/intersect_kernel.cl:65-114), float operations in its order
struct Accepted {
	bool ok;
	float distance;
	float ip[3];
};
inline Accepted reference_triangle(const TriRec &t, const float o[3], const float d[3]) {
	Accepted none{ false, 0.0f, { 0, 0, 0 } };
	const float w0[3] = { o[0] - t.ta[0], o[1] - t.ta[1], o[2] - t.ta[2] };
	const float a = -((t.n[0] * w0[0] + t.n[1] * w0[1]) + t.n[2] * w0[2]);
	const float b = (t.n[0] * d[0] + t.n[1] * d[1]) + t.n[2] * d[2];
	if (std::fabs(b) < 0.000001f)
		return none;
	const float r = a / b;
	if (r < 0.0f)
		return none;
	const float ip[3] = { o[0] + d[0] * r, o[1] + d[1] * r, o[2] + d[2] * r };
	const float w[3] = { ip[0] - t.ta[0], ip[1] - t.ta[1], ip[2] - t.ta[2] };
	const float wu = (t.u[0] * w[0] + t.u[1] * w[1]) + t.u[2] * w[2];
	const float wv = (w[0] * t.v[0] + w[1] * t.v[1]) + w[2] * t.v[2];
	const float s = (t.uv * wv - t.vv * wu) / t.D;
	if (s < -0.00001f || (double) s > 1.00001)
		return none;
	const float q = (t.uv * wu - t.uu * wv) / t.D;
	if (q < -0.00001f || (double) (s + q) > 1.00001)
		return none;
	const float e[3] = { ip[0] - o[0], ip[1] - o[1], ip[2] - o[2] };
	return { true, std::sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]), { ip[0], ip[1], ip[2] } };
}

// What the kernel keeps per lane (kernels/common.hip.h, WalkRay) and its node test on a padded record (kernels/walk.hip.h,
// OCRT_TEST_COHERENT / OCRT_TEST_MIXED): near = max3(x, y, max(z, tiny)), far = min3(x, y, min(z, limit)), near <= far.
struct KernelRay {
	float wi[3], oi[3];
	bool positive[3];
};
inline KernelRay kernel_ray(const float o[3], const float d[3]) {
	const float INF = std::numeric_limits<float>::infinity();
	KernelRay r;
	for (int k = 0; k < 3; ++k) {
		const float inv = 1.0f / d[k];
		r.wi[k] = std::fabs(inv) == INF ? std::copysign(0x1.0p+100f, inv) : inv;
		r.oi[k] = -(o[k] * r.wi[k]);
		r.positive[k] = inv >= 0;
	}
	return r;
}
inline float kernel_near(const NodeRec &n, const KernelRay &r, float *far_out) {
	float near[3], far[3];
	for (int k = 0; k < 3; ++k) {
		const float a = std::fmaf(n.lo[k], r.wi[k], r.oi[k]), b = std::fmaf(n.hi[k], r.wi[k], r.oi[k]);
		near[k] = r.positive[k] ? a : b;
		far[k] = r.positive[k] ? b : a;
	}
	const float tiny = std::numeric_limits<float>::denorm_min();
	*far_out = std::fmin(std::fmin(far[0], far[1]), far[2]);
	return std::fmax(std::fmax(near[0], near[1]), std::fmax(near[2], tiny));  // (fmax / fmin drop NaN like v_max3 / v_min3)
}
// the kernel's own condition for taking the fast form (kernels/common.hip.h, ray_is_selectable)
inline bool selectable(const float o[3], const float d[3], float origin_limit) {
	const float INF = std::numeric_limits<float>::infinity();
	bool origin_ok = true, numbers = true, some_finite = false;
	float smallest = INF;
	for (int k = 0; k < 3; ++k) {
		origin_ok = origin_ok && std::fabs(o[k]) <= origin_limit;
		const float a = std::fabs(1.0f / d[k]);
		numbers = numbers && (a <= 1.0e30f || a == INF);
		some_finite = some_finite || a <= 1.0e30f;
		smallest = std::fmin(smallest, a);
	}
	return origin_ok && numbers && smallest >= 0.5f && some_finite;
}

// near distance of a box along a ray, in double
inline bool box_near(const float lo[3], const float hi[3], const float o[3], const float d[3], double *near_out) {
	double near = 0.0, far = std::numeric_limits<double>::infinity();
	for (int k = 0; k < 3; ++k) {
		if (d[k] == 0.0f) {
			if (o[k] < lo[k] || o[k] > hi[k])
				return false;
			continue;
		}
		const double a = ((double) lo[k] - o[k]) / d[k], b = ((double) hi[k] - o[k]) / d[k];
		near = std::fmax(near, std::fmin(a, b));
		far = std::fmin(far, std::fmax(a, b));
	}
	*near_out = near;
	return near <= far;
}

}  // namespace reference_tests
