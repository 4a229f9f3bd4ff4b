// align_step.h -- the host side of aligning two maps (align.hip, kf_align_brick_store) and of refining poses in the map (relocal.hip, kf_map_refine_poses); no
// reference counterpart: one Gauss-Newton step from the 29 sums to the updated transform, and one turn of the loop around it -- the only place that gives
// a verdict (kf_align_loop_turn).  Plain host C++, fp64: the library and the stand-alone test program (tests/map_align_main.cpp) both include it.  The rule
// is written out above kf_align_brick_store in include/hybkf.h.
//
// sums: [0, 21) the upper triangle of A = sum J J^T, row by row ((0,0), (0,1) .. (0,5), (1,1) .. (5,5)); [21, 27) b = sum J e; [27] sum e e; [28] the pair
// count.  J = (x cross gd, gd): the first three unknowns are the rotation vector omega (radians, about `centre`), the last three the translation v (voxels).
#pragma once
#include <math.h>
#include <string.h>
#include "../../include/hybkf.h"
#include "rigid_keys.h"

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

// eps_rot and eps_trans finite and >= 0, the n centres (3 doubles each) finite: what both loops ask of their stopping rule
static inline bool kf_align_stop_valid(double eps_rot, double eps_trans, const double* centres, size_t n) {
  if (!isfinite(eps_rot) || !isfinite(eps_trans) || eps_rot < 0.0 || eps_trans < 0.0) return false;
  for (size_t i = 0; i < 3 * n; ++i) if (!isfinite(centres[i])) return false;
  return true;
}

// One pose's loop.  cur: where the next evaluation is taken.  good: the result so far -- the last pose evaluated with enough pairs (the guess, if none), and the
// stepped pose once the verdict is CONVERGED.  rep: the steps taken, the last evaluation's sums and rms, the last step; its verdict counts once a turn said stop.
struct KfAlignLoop { double cur[12], good[12]; kf_align_report rep; };

static inline void kf_align_loop_begin(KfAlignLoop& s, const double* xf) {
  memcpy(s.cur, xf, sizeof(s.cur)); memcpy(s.good, xf, sizeof(s.good));
  memset(&s.rep, 0, sizeof(s.rep));
}

// One turn: `sums` are the 29 sums evaluated at s.cur.  True: s.cur is stepped and wants an evaluation; false: s.rep.verdict says why the loop ends, s.good is
// the result.  require_rigid: a stepped transform that is no longer rigid (kf_rigid_valid) ends the loop like a refused step, iterations and step as they were.
static inline bool kf_align_loop_turn(KfAlignLoop& s, const double* sums, const double* centre, uint32_t max_iter, uint32_t min_pairs, double eps_rot,
                                      double eps_trans, bool require_rigid) {
  kf_align_report& rep = s.rep;
  memcpy(rep.sums, sums, sizeof(rep.sums));
  rep.rms = sums[28] > 0.0 ? sqrt(sums[27] / sums[28]) : 0.0;
  if (!(sums[28] > 0.0) || sums[28] < (double)min_pairs) { rep.verdict = KF_ALIGN_FEW_PAIRS; return false; }
  memcpy(s.good, s.cur, sizeof(s.good));                         // evaluated successfully
  if (rep.iterations >= max_iter) { rep.verdict = KF_ALIGN_ITER_LIMIT; return false; }
  double step[6];
  if (kf_align_step_host(sums, centre, s.cur, step) || (require_rigid && !kf_rigid_valid(s.cur))) { rep.verdict = KF_ALIGN_SINGULAR; return false; }
  rep.iterations += 1u;
  memcpy(rep.step, step, sizeof(step));
  const double rot = sqrt(step[0] * step[0] + step[1] * step[1] + step[2] * step[2]), tr = sqrt(step[3] * step[3] + step[4] * step[4] + step[5] * step[5]);
  if (rot <= fmax(eps_rot, KF_ALIGN_EPS_ROT_MIN) && tr <= fmax(eps_trans, KF_ALIGN_EPS_TRANS_MIN)) {
    rep.verdict = KF_ALIGN_CONVERGED; memcpy(s.good, s.cur, sizeof(s.good)); return false;
  }
  return true;
}
