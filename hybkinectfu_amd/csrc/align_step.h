// align_step.h -- the host side of aligning two maps (align.hip, kf_align_brick_store; no reference counterpart): one Gauss-Newton step from the 29 sums to
// the updated transform.  Plain host C++, fp64: the library and the stand-alone test program (tests/map_align_main.cpp) both include it.  The rule is
// written out above kf_align_brick_store in include/hybkf.h.
//
// sums: [0, 21) the upper triangle of A = sum J J^T, row by row ((0,0), (0,1) .. (0,5), (1,1) .. (5,5)); [21, 27) b = sum J e; [27] sum e e; [28] the pair
// count.  J = (x cross gd, gd): the first three unknowns are the rotation vector omega (radians, about `centre`), the last three the translation v (voxels).
#pragma once
#include <math.h>

#define KF_ALIGN_SUMS 29

// A xi = b by Cholesky, A = L L^T, in place.  False on a pivot that is not > 0 (also what is not a number): A is not positive definite.
static inline bool kf_align_solve6(const double* sums, double xi[6]) {
  double L[6][6];
  for (int a = 0, k = 0; a < 6; ++a)
    for (int b = a; b < 6; ++b, ++k) L[b][a] = sums[k];          // the lower triangle
  for (int j = 0; j < 6; ++j) {
    double d = L[j][j];
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    if (!(d > 0.0) || !isfinite(d)) return false;
    const double p = sqrt(d);
    L[j][j] = p;
    for (int i = j + 1; i < 6; ++i) {
      double s = L[i][j];
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
      L[i][j] = s / p;
    }
  }
  double y[6];
  for (int i = 0; i < 6; ++i) {                                  // L y = b
    double s = sums[21 + i];
    for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
    y[i] = s / L[i][i];
  }
  for (int i = 5; i >= 0; --i) {                                 // L^T xi = y
    double s = y[i];
    for (int k = i + 1; k < 6; ++k) s -= L[k][i] * xi[k];
    xi[i] = s / L[i][i];
  }
  for (int i = 0; i < 6; ++i) if (!isfinite(xi[i])) return false;
  return true;
}

// exp of the twist xi = (omega, v): E = exp(omega^) (Rodrigues) and V v with V = I + B W + C W^2, W = omega^, B = (1 - cos th) / th^2, C = (th - sin th) / th^3;
// below th = 1e-4 the series A = 1 - th^2/6, B = 1/2 - th^2/24, C = 1/6 - th^2/120 (their next terms are below 1e-18)
static inline void kf_align_exp(const double xi[6], double E[9], double u[3]) {
  const double wx = xi[0], wy = xi[1], wz = xi[2];
  const double t2 = wx * wx + wy * wy + wz * wz, th = sqrt(t2);
  double A, B, C;
  if (th < 1e-4) { A = 1.0 - t2 / 6.0; B = 0.5 - t2 / 24.0; C = 1.0 / 6.0 - t2 / 120.0; }
  else { A = sin(th) / th; B = (1.0 - cos(th)) / t2; C = (th - sin(th)) / (t2 * th); }
  const double W[9] = {0, -wz, wy, wz, 0, -wx, -wy, wx, 0};
  double W2[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) W2[3 * i + j] = W[3 * i] * W[j] + W[3 * i + 1] * W[3 + j] + W[3 * i + 2] * W[6 + j];
  for (int i = 0; i < 3; ++i) {
    u[i] = 0.0;
    for (int j = 0; j < 3; ++j) {
      const double I = i == j ? 1.0 : 0.0;
      E[3 * i + j] = I + A * W[3 * i + j] + B * W2[3 * i + j];
      u[i] += (I + B * W[3 * i + j] + C * W2[3 * i + j]) * xi[3 + j];
    }
  }
}

// One step: solves (sum J J^T) xi = sum J e and applies xf <- T(centre) exp(xi) T(-centre) xf, that is R <- E R, t <- E (t - centre) + centre + V v.
// Returns 0, or 1 with xf and step untouched: a NULL pointer, a pivot <= 0, a step or a transform that is not finite.
static inline int kf_align_step_host(const double* sums, const double* centre, double* xf, double* step) {
  if (!sums || !centre || !xf || !step) return 1;
  double xi[6], E[9], u[3], out[12];
  if (!kf_align_solve6(sums, xi)) return 1;
  kf_align_exp(xi, E, u);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) out[4 * i + j] = E[3 * i] * xf[j] + E[3 * i + 1] * xf[4 + j] + E[3 * i + 2] * xf[8 + j];
    out[4 * i + 3] = (E[3 * i] * (xf[3] - centre[0]) + E[3 * i + 1] * (xf[7] - centre[1]) + E[3 * i + 2] * (xf[11] - centre[2])) + centre[i] + u[i];
  }
  for (int i = 0; i < 12; ++i) if (!isfinite(out[i])) return 1;
  for (int i = 0; i < 12; ++i) xf[i] = out[i];
  for (int i = 0; i < 6; ++i) step[i] = xi[i];
  return 0;
}
