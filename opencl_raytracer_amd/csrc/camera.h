// camera.h -- making a camera pose (device_types.h: CameraPose) from an eye point, a target and an up hint.  Host only,
// header only: the C ABI (rt_camera_look_at, include/rt_hip_camera.h) and the `render` CLI (--eye / --look-at / --up) share it.
#pragma once
#include <cmath>

#include "device_types.h"

namespace ocrt {

// An orthonormal, right-handed basis (right x up = -forward, as the reference's camera: x to the right, y up, looking
// down -z) with forward = the direction from `eye` to `target` and up in the plane of forward and `up_hint`, computed in
// double and rounded to float once.  False -- and *out untouched -- for input that is not finite, eye == target, and an
// up hint that is zero or parallel to the view direction.
inline bool camera_look_at(const float eye[3], const float target[3], const float up_hint[3], CameraPose *out) {
	double f[3], h[3];
	for (int k = 0; k < 3; ++k) {
		if (!std::isfinite(eye[k]) || !std::isfinite(target[k]) || !std::isfinite(up_hint[k]))
			return false;
		f[k] = (double) target[k] - (double) eye[k];
		h[k] = up_hint[k];
	}
	const double fl = std::sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]), hl = std::sqrt(h[0] * h[0] + h[1] * h[1] + h[2] * h[2]);
	if (!(fl > 0.0) || !(hl > 0.0))
		return false;
	for (int k = 0; k < 3; ++k) {
		f[k] /= fl;
		h[k] /= hl;
	}
	double r[3] = { f[1] * h[2] - f[2] * h[1], f[2] * h[0] - f[0] * h[2], f[0] * h[1] - f[1] * h[0] };
	const double rl = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);  // (the sine of the angle between the two)
	if (!(rl > 1.0e-9))
		return false;
	for (int k = 0; k < 3; ++k)
		r[k] /= rl;
	const double u[3] = { r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0] };
	for (int k = 0; k < 3; ++k) {  // (+ 0.0: a component that came out as -0 is +0)
		out->eye[k] = eye[k];
		out->right[k] = (float) (r[k] + 0.0);
		out->up[k] = (float) (u[k] + 0.0);
		out->forward[k] = (float) (f[k] + 0.0);
	}
	return true;
}

}  // namespace ocrt
