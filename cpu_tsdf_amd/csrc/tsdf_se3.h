/* The host arithmetic of tsdf_hip_align, in plain C and fp64, so that every binding gets the same answer: the closed-form
 * SE(3) exponential, the 6 x 6 Cholesky solve of the normal equations, and the pose update.  Header-only (static inline):
 * tsdf_align.hip includes it, and so does the small program tests/test_align_abi.py compiles to check it on the host.
 * Poses are 12 doubles: the rows of [R | t]. */
#ifndef TSDF_SE3_H
#define TSDF_SE3_H

#include <math.h>

/* exp of the twist xi = (omega, v):  R = I + a K + b K^2,  t = (I + b K + c K^2) v  with K = [omega]x, theta = |omega|,
 * a = sin(theta) / theta, b = (1 - cos(theta)) / theta^2, c = (theta - sin(theta)) / theta^3 (Rodrigues); below
 * theta = 1e-12 the coefficients come from their series (1 - theta^2/6, 1/2 - theta^2/24, 1/6 - theta^2/120). */
static inline void tsdf_se3_exp(const double xi[6], double T[12]) {
  const double wx = xi[0], wy = xi[1], wz = xi[2];
  const double th2 = wx * wx + wy * wy + wz * wz, th = sqrt(th2);
  double a, b, c;
  if (th < 1e-12) {
    a = 1.0 - th2 / 6.0;
    b = 0.5 - th2 / 24.0;
    c = 1.0 / 6.0 - th2 / 120.0;
  } else {
    const double sh = sin(0.5 * th);
    a = sin(th) / th;
    b = 2.0 * sh * sh / th2; /* 1 - cos without the cancellation */
    c = (th - sin(th)) / (th2 * th); /* absolute error ~ eps / theta^2, and c only ever multiplies K^2 ~ theta^2 */
  }
  const double K[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
  double K2[9];
  for (int r = 0; r < 3; ++r)
    for (int s = 0; s < 3; ++s) K2[3 * r + s] = K[3 * r] * K[s] + K[3 * r + 1] * K[3 + s] + K[3 * r + 2] * K[6 + s];
  for (int r = 0; r < 3; ++r) {
    double t = 0.0;
    for (int s = 0; s < 3; ++s) {
      const double id = r == s ? 1.0 : 0.0;
      T[4 * r + s] = id + a * K[3 * r + s] + b * K2[3 * r + s];
      t += (id + b * K[3 * r + s] + c * K2[3 * r + s]) * xi[3 + s];
    }
    T[4 * r + 3] = t;
  }
}

/* out = A * B for two poses (out may not alias) */
static inline void tsdf_se3_mul(const double A[12], const double B[12], double out[12]) {
  for (int r = 0; r < 3; ++r) {
    for (int s = 0; s < 4; ++s)
      out[4 * r + s] = A[4 * r] * B[s] + A[4 * r + 1] * B[4 + s] + A[4 * r + 2] * B[8 + s];
    out[4 * r + 3] += A[4 * r + 3];
  }
}

/* Solve  A x = -b  for the step of Gauss-Newton: sys = the 29 numbers of tsdf_hip_align_system (21 upper-triangle entries
 * of A = sum J J^T row-major, then b = sum J r).  Cholesky A = L L^T.  Returns 0, or 1 where A is not positive definite
 * TO WORKING PRECISION: a pivot that is not above 1e-10 of the largest diagonal entry (a cloud that leaves a freedom
 * unconstrained -- one plane -- gives pivots of rounding noise, ~1e-13 relative, not exact zeros). */
static inline int tsdf_solve_step(const double sys[29], double x[6]) {
  double L[36], dmax = 0.0;
  int k = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j, ++k) L[6 * j + i] = L[6 * i + j] = sys[k];
  for (int i = 0; i < 6; ++i)
    if (L[7 * i] > dmax) dmax = L[7 * i];
  if (!(dmax > 0.0) || !(dmax < INFINITY)) return 1;
  for (int j = 0; j < 6; ++j) {
    double d = L[7 * j];
    for (int m = 0; m < j; ++m) d -= L[6 * j + m] * L[6 * j + m];
    if (!(d > 1e-10 * dmax)) return 1;
    d = sqrt(d);
    L[7 * j] = d;
    for (int i = j + 1; i < 6; ++i) {
      double s = L[6 * i + j];
      for (int m = 0; m < j; ++m) s -= L[6 * i + m] * L[6 * j + m];
      L[6 * i + j] = s / d;
    }
  }
  double y[6];
  for (int i = 0; i < 6; ++i) {
    double s = -sys[21 + i];
    for (int m = 0; m < i; ++m) s -= L[6 * i + m] * y[m];
    y[i] = s / L[7 * i];
  }
  for (int i = 5; i >= 0; --i) {
    double s = y[i];
    for (int m = i + 1; m < 6; ++m) s -= L[6 * m + i] * x[m];
    x[i] = s / L[7 * i];
  }
  return 0;
}

#endif /* TSDF_SE3_H */
