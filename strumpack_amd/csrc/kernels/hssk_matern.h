// The finish of the Matern kernels (types 3 and 4): from the squared Euclidean distance of a pair to the kernel
// value or to its derivative in the width h.  With s = sqrt(2 nu) r / h:
//   type 3, nu = 3/2:   k = (1 + s) e^-s             dk/dh = s^2 e^-s / h
//   type 4, nu = 5/2:   k = (1 + s + s^2 / 3) e^-s   dk/dh = s^2 (1 + s) e^-s / (3 h)
// Neither form divides by r: a pair at distance 0 gives k = 1 and dk/dh = 0 exactly.  Every kernel that evaluates a Matern
// entry -- construction, FP64 sums, the exact products, the FP32 routes -- ends in one of the two functions below, so that
// the arithmetic of an entry is one piece of code.  The distance loop in front of them is the Gauss one.
#pragma once
#include "hssk_device.h"

namespace {

// the squared distance q becomes s^2 = c q
__host__ __device__ inline double hssk_matern_c(int type, double h) { return (type == 3 ? 3. : 5.) / (h * h); }

// FP64: q = sum_j (x_j - y_j)^2, c = 2 nu / h^2
template <int TYPE, int DERIV>
__device__ inline double hssk_matern(double q, double c, double h) {
  static_assert(TYPE == 3 || TYPE == 4, "Matern32 is type 3, Matern52 type 4");
  const double s = sqrt(c * q), e = exp(-s);
  if (DERIV == 0) return TYPE == 3 ? (1. + s) * e : (1. + s + s * s / 3.) * e;
  return TYPE == 3 ? s * s * e / h : s * s * (1. + s) * e / (3. * h);
}
// The factor f of the derivative in a point, dk(x, t)/dt_j = f (x_j - t_j): dk/ds = -s e^-s (nu = 3/2), -s (1 + s) e^-s / 3
// (nu = 5/2) and ds/dt_j = -c (x_j - t_j) / s, so the s cancels and nothing divides by the distance:
//   type 3:  f = c e^-s        type 4:  f = (c / 3) (1 + s) e^-s        with the s and the exponential of hssk_matern above
template <int TYPE>
__device__ inline double hssk_matern_dt_factor(double q, double c) {
  static_assert(TYPE == 3 || TYPE == 4, "Matern32 is type 3, Matern52 type 4");
  const double s = sqrt(c * q), e = exp(-s);
  return TYPE == 3 ? c * e : (c / 3.) * ((1. + s) * e);
}
// the same with the type known only at run time (kernels that are not instantiated per type)
__device__ inline double hssk_matern_rt(int type, double q, double c, double h) {
  return type == 3 ? hssk_matern<3, 0>(q, c, h) : hssk_matern<4, 0>(q, c, h);
}

// FP32 value from u = s^2 of points already scaled by sqrt(2 nu) / h.  The clamp is part of the contract: on the matrix-core
// route u is |x~|^2 + |y~|^2 - 2 x~.y~, which cancellation makes negative for near-duplicate points, and the square root of a
// negative number would poison a whole sum.
template <int TYPE>
__device__ inline float hssk_matern_f32(float u) {
  static_assert(TYPE == 3 || TYPE == 4, "Matern32 is type 3, Matern52 type 4");
  const float s = sqrtf(fmaxf(u, 0.f)), e = exp2f(-(s * 1.44269504088896341f));
  return TYPE == 3 ? (1.f + s) * e : (1.f + s + s * s * (1.f / 3.f)) * e;
}

}  // namespace
