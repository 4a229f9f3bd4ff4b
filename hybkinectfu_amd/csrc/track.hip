// track.hip -- camera tracking: projective point-to-plane ICP and the direct SDF tracker, with the whole Gauss-Newton
// loop resident on the device.
//
// Reference: computeGbufKernel / findCorrs / buildPointToPlaneSolverRows (src/cuda/CalPointToPlaneErrSolverParams.cu:7-129),
// reduceGbufKernel (src/cuda/device_functions.h:17-55), computeSDFSolverbufKernel / buildSDFSolverRows
// (src/cuda/CalSDFErrSolverParams.cu:7-138), CameraPoseFinderICP (src/CameraPoseFinderICP.cpp:12-145),
// CameraPoseFinderSDF (src/CameraPoseFinderSDF.cpp:25-106), direct_exponential_map (src/utils/eigen_utils.cpp:60-127).
//
// gfx950 design.  The reference builds the 6x6 system with 27 sequential 256-wide shared-memory tree reductions
// (54 barriers) per launch, a second 27-block launch, a device sync and a 108-byte read-back, 19 times per frame; the
// loop is latency-bound.  Here a Gauss-Newton step is ONE launch and the host never sees the 27 floats:
//   * every lane keeps the 27 partial sums of its pixels in registers (no MFMA: a 6x6 outer product is far too small);
//     a wave64 __shfl_down tree folds them, LDS holds the four per-wave partials, 27 lanes write the workgroup partial;
//   * there is no second "reduce" launch, no atomic and no fence: the NEXT step's launch starts by having every workgroup
//     sum the previous step's workgroup partials (<= 512 x 27 floats, L2 resident) in the same fixed order and run the same
//     6x6 determinant test / Cholesky solve / shake test / pose composition on one lane, so all workgroups hold the
//     identical new transform (bitwise) and go straight on to their pixels.  Partials and the running transform are
//     double-buffered by step parity; the kernel boundary is the only synchronisation (1.5-2 us, MI355X_MICROARCH.md
//     'boundary') -- cheaper than a ticket on one contended word plus a release/acquire pair per step;
//   * a last 1-workgroup launch folds the final step and commits CameraPoseFinder::_pose.
// Sums are fp32 in a fixed (reproducible) association that differs from the reference's tree, so parity for this stage is
// by tolerance (pose within 1e-4 m / 1e-4 rad), as SURVEY.md section 8a row a6 states.
#include "kf_internal.h"
#include "cull.h"
#include "bilateral_tile.h"
#include "sdf_rows.h"
#include <string.h>

#define TRK_THREADS 256
#define TRK_PX 2                   // 8x8 tiles per wave of the SDF step (grid-stride beyond that): the lookups want many waves, not long lanes

// the Gauss-Newton thresholds of one tracking call, in every form the kernels use (track_thresholds)
struct TrackThresholds {
  float dist_thres, sin_thres, dist_shake, angle_shake;
  float cos_shake, dist_shake2;                  // cos(angle_shake), dist_shake^2: the shake test without acos / sqrt
  float dist_thres2, sin_thres2;                 // the correspondence gates' squares (gate_square: a negative threshold rejects everything, as `norm > t` does)
};
struct TrackArgs {
  const float4* new_v; const float4* new_n; const float4* model_v; const float4* model_n;
  KfCam cam;
  KfMat cur_val, linv_val;                       // host-supplied transforms (per-call wrappers only)
  int use_state;                                 // 1: transforms come from the device-resident KfTrackState
  TrackThresholds th;
  float* partials;                               // 2 x KF_ICP_MAX_WG x 32 floats, indexed by step parity
  KfTrackState* track;
  int step;                                      // index of this Gauss-Newton step within the frame (buffer parity)
  int consume;                                   // 1: first fold + apply the previous step's system
  int n_prev_wg;                                 // workgroups that wrote the previous step's partials
  int fold_group;                                // > 0: fold them in groups g, g + fold_group, ... first (fold_partials: the batched loop's publishers)
  int sdf;                                       // consume with the SDF tracker's update rule (exp map, convergence test)
  // pixel-partitioned ICP (multi-GPU): this context sums only pixels [px_begin, px_end) (0,0 = all); the previous step's
  // system arrives all-reduced in ext_prev (27 floats) instead of workgroup partials; fold_out receives this step's 27 sums
  int px_begin, px_end;
  // replicated ICP, one launch per step: the persistent loop's pixel dealing (icp_level_geometry) -- px_l pixels per lane dealt in
  // 64-pixel chunks round robin over deal_grid workgroups -- so that both launch forms add the same numbers in the same order
  // (px_l == 0: a contiguous pixel range per workgroup, the pixel-partitioned form)
  int px_l, deal_grid;
  const float* ext_prev;
  float* fold_out;
  // SDF tracker only
  KfVolume vol; const float* depth;
  int slab_pixels;                               // 1: sum only pixels whose own voxel (pworld0) lies in the layers this context OWNS (z-slab partition)
#ifdef KF_EXPERIMENTS
  unsigned long long* dbg;                       // KF_ICP_EXP=11: where workgroup 0 accumulates the solve's sub-phase times (10 ns ticks)
  int exp_nodet;                                 // KF_ICP_EXP=12: skip the determinant (timing only)
#endif
};

// ---- 6x6 dense algebra on one lane (stands in for Eigen); every index is static after unrolling -> registers only ----
// src/CameraPoseFinderICP.cpp:119-136
__device__ __forceinline__ void unpack27(const float* in, float A[36], float b[6]) {
  int s = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = i; j < 7; ++j) {
      float v = in[s++];
      if (j == 6) b[i] = v; else { A[i * 6 + j] = v; A[j * 6 + i] = v; }
    }
}
// determinant by partial-pivot LU (Eigen's path for a 6x6 `determinant()`), fp32; destroys m
__device__ __forceinline__ float det6(float m[36]) {
  float det = 1.f;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    int p = k; float best = fabsf(m[k * 6 + k]);
#pragma unroll
    for (int r = k + 1; r < 6; ++r) { float v = fabsf(m[r * 6 + k]); if (v > best) { best = v; p = r; } }
    if (best == 0.f) return 0.f;
#pragma unroll
    for (int r = k + 1; r < 6; ++r)
      if (p == r) {
#pragma unroll
        for (int c = 0; c < 6; ++c) { float t = m[k * 6 + c]; m[k * 6 + c] = m[r * 6 + c]; m[r * 6 + c] = t; }
        det = -det;
      }
    const float piv = m[k * 6 + k];
    det *= piv;
#ifndef KF_SOLVE_EXACT
    const float rp = __builtin_amdgcn_rcpf(piv);             // 1-ulp reciprocal, as in llt_solve6 below: the result only meets a threshold
#else
    const KfRecip rp = kf_recip(piv);                        // one reciprocal refinement per pivot, exact quotients (kf_div)
#endif
#pragma unroll
    for (int r = k + 1; r < 6; ++r) {
#ifndef KF_SOLVE_EXACT
      const float f = m[r * 6 + k] * rp;
#else
      const float f = kf_div(m[r * 6 + k], rp);
#endif
#pragma unroll
      for (int c = k + 1; c < 6; ++c) m[r * 6 + c] -= f * m[k * 6 + c];
    }
  }
  return det;
}
// x = LLT(A) \ b, fp32 (ICP.cpp:143, SDF.cpp:79: Eigen's llt().solve in float).  The solve is one chain of dependent operations on
// one lane (about 1 us of the 1.7 us a Gauss-Newton step spends between two pixel phases), so its square roots, reciprocals and
// quotients are the hardware's 1-ulp v_sqrt_f32 / v_rcp_f32 and a product with the reciprocal, not the correctly rounded forms:
// -7.5 us per frame.  What that costs in fidelity is below what is there anyway -- the 27 sums the solve starts from differ from
// the reference's in their last bits (fp32 sums in another association order, asserted <= 1e-5), the tracked pose is asserted to
// 1e-4 against an exactly rounded CPU restatement of Eigen's chain on identical inputs and stays there, and every
// workgroup, rank and context runs the same instructions, so poses stay bitwise reproducible.  -DKF_SOLVE_EXACT restores the
// correctly rounded chain.
__device__ __forceinline__ void llt_solve6(const float A[36], const float b[6], float x[6]) {
#ifndef KF_SOLVE_EXACT
  float L[36], rd[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    float s = A[j * 6 + j];
#pragma unroll
    for (int k = 0; k < j; ++k) s -= L[j * 6 + k] * L[j * 6 + k];
#ifndef KF_SOLVE_SQRT_RCP
    rd[j] = __builtin_amdgcn_rsqf(s);                        // 1 / L_jj in ONE transcendental (L_jj itself is never used: every use divides by it)
#else
    const float d = __builtin_amdgcn_sqrtf(s);
    L[j * 6 + j] = d;
    rd[j] = __builtin_amdgcn_rcpf(d);
#endif
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      float t = A[i * 6 + j];
#pragma unroll
      for (int k = 0; k < j; ++k) t -= L[i * 6 + k] * L[j * 6 + k];
      L[i * 6 + j] = t * rd[j];
    }
  }
  float y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    float t = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) t -= L[i * 6 + k] * y[k];
    y[i] = t * rd[i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    float t = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) t -= L[k * 6 + i] * x[k];
    x[i] = t * rd[i];
  }
#else
  float L[36]; KfRecip rd[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    float s = A[j * 6 + j];
#pragma unroll
    for (int k = 0; k < j; ++k) s -= L[j * 6 + k] * L[j * 6 + k];
    const float d = sqrtf(s);
    L[j * 6 + j] = d;
    rd[j] = kf_recip(d);                                     // every division by L_jj (3 per column) shares this reciprocal
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      float t = A[i * 6 + j];
#pragma unroll
      for (int k = 0; k < j; ++k) t -= L[i * 6 + k] * L[j * 6 + k];
      L[i * 6 + j] = kf_div(t, rd[j]);
    }
  }
  float y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    float t = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) t -= L[i * 6 + k] * y[k];
    y[i] = kf_div(t, rd[i]);
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    float t = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) t -= L[k * 6 + i] * x[k];
    x[i] = kf_div(t, rd[i]);
  }
#endif
}
// The same 6x6 system solved by a WAVE: lane i (< 6) holds row i of the symmetric matrix and b_i; a right-looking Cholesky -- column j is scaled by
// rsq(pivot), then every lane takes l_i * l_k off its trailing entries, l_k by v_readlane -- with the forward substitution carried along as a seventh
// column, then a column-oriented back substitution on wave-uniform values.  About 110 instructions on a dependent chain of six (readlane, rsq, product,
// fused update) links instead of ~430 instructions and two transcendentals per pivot on one lane: the Gauss-Newton step's solve phase was that chain.
// The pivots come for free, and with them the determinant the reference tests (ICP.cpp:138 `determinant() < 1e-10` on the float matrix): for the
// symmetric positive (semi-)definite J^T J it is the product of the Cholesky pivots, so the second 6x6 factorization (det6: partial-pivot LU on a lane of
// another wave, the longer of the two chains) is not run at all; a pivot <= 0 means the product has no business being positive: singular.  Same inputs
// in every workgroup / launch form -> same bits everywhere; against the reference's Eigen chain the increment agrees as before to the asserted 1e-4
// (1-ulp rsq and fused updates instead of sqrt / divide: DESIGN.md section 2.4).  -DKF_SOLVE_ONE_LANE restores the one-lane solve + LU determinant.
__device__ __forceinline__ void llt_solve6_wave(const float* s_tot, float x[6], bool& singular, float& det) {
  const int i = min((int)(threadIdx.x & 63u), 5);
  float a[6], bb;
#pragma unroll
  for (int j = 0; j < 6; ++j) { const int r = i < j ? i : j, c = i < j ? j : i; a[j] = s_tot[7 * r - (r * (r - 1)) / 2 + (c - r)]; }   // the packing of unpack27
  bb = s_tot[7 * i - (i * (i - 1)) / 2 + (6 - i)];
  float Lc[6], y[6], rd[6];
  bool bad = false; float prod = 1.f;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const float sj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a[j]), j));      // the pivot: row j's diagonal after the earlier columns' updates
    bad = bad || (sj <= 0.f);
    prod *= sj;
    const float r = __builtin_amdgcn_rsqf(sj);
    rd[j] = r;
    const float l = a[j] * r;                                                                  // lane i >= j: L[i][j]
    Lc[j] = l;
#pragma unroll
    for (int k = j + 1; k < 6; ++k) a[k] = __builtin_fmaf(-l, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(l), k)), a[k]);
    const float yj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(bb), j)) * r;     // forward substitution, as column 7
    y[j] = yj;
    bb = __builtin_fmaf(-l, yj, bb);
  }
#pragma unroll
  for (int k = 5; k >= 0; --k) {
    const float xk = y[k] * rd[k];
    x[k] = xk;
#pragma unroll
    for (int r = 0; r < k; ++r) y[r] = __builtin_fmaf(-__int_as_float(__builtin_amdgcn_readlane(__float_as_int(Lc[r]), k)), xk, y[r]);   // L[k][r] lives in lane k
  }
  singular = bad; det = prod;
}
__device__ __forceinline__ void mat3_mul(const float a[9], const float b[9], float o[9]) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) o[r * 3 + c] = a[r * 3] * b[c] + a[r * 3 + 1] * b[3 + c] + a[r * 3 + 2] * b[6 + c];
}
// Mat.h:240-262
__device__ __forceinline__ void mat44_mul(const float* a, const float* b, float* out) {
  float r[16];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) r[i * 4 + j] = a[i * 4] * b[j] + a[i * 4 + 1] * b[4 + j] + a[i * 4 + 2] * b[8 + j] + a[i * 4 + 3] * b[12 + j];
#pragma unroll
  for (int i = 0; i < 16; ++i) out[i] = r[i];
}
// vector6ToTransformMatrix (ICP.cpp:95-111, SDF.cpp:25-43): R = Rx Ry Rz, shake test on the rotation angle and |t|
__device__ __forceinline__ bool transform_from_sincos(const float x[6], float c0, float s0, float c1, float s1, float c2, float s2,
                                                      float dist_shake2, float cos_shake, float t[16]) {
  // R = Rx Ry Rz with Rx = {1,0,0, 0,c0,-s0, 0,s0,c0}, Ry = {c1,0,s1, 0,1,0, -s1,0,c1}, Rz = {c2,-s2,0, s2,c2,0, 0,0,1} (ICP.cpp:98-100).
  // The general 3x3 products spend most of their 90 operations on the literal zeros and ones; written out, every element is the same
  // sum of the same products in the same order with the x * 0, x * 1 and + 0 terms dropped -- equal values for every finite input
  // (only the sign of an exact zero can differ, and a NaN angle still poisons R0 / R4 / R8, i.e. the shake verdict).
  const float xy3 = s0 * s1, xy5 = -s0 * c1, xy6 = -c0 * s1, xy8 = c0 * c1;            // Rx Ry = {c1, 0, s1,  xy3, c0, xy5,  xy6, s0, xy8}
  const float R[9] = {c1 * c2, c1 * -s2, s1,
                      xy3 * c2 + c0 * s2, xy3 * -s2 + c0 * c2, xy5,
                      xy6 * c2 + s0 * s2, xy6 * -s2 + s0 * c2, xy8};
  // the reference compares AngleAxisf(R).angle() = acos(ca) with angle_shake and |t| with dist_shake (ICP.cpp:101-107); acos is
  // decreasing and the square root increasing, so the same verdicts come from ca >= cos(angle_shake) and |t|^2 <= dist_shake^2
  // (thresholds prepared once per call) -- without an acos and a square root on the one-lane chain of every Gauss-Newton step
  float ca = (R[0] + R[4] + R[8] - 1.f) * 0.5f;
  ca = fminf(1.f, fmaxf(-1.f, ca));
  const float d2 = x[3] * x[3] + x[4] * x[4] + x[5] * x[5];
  if (!(ca >= cos_shake) || !(d2 <= dist_shake2)) return false;        // a NaN increment counts as shaking: never applied
  const float o[16] = {R[0], R[1], R[2], x[3], R[3], R[4], R[5], x[4], R[6], R[7], R[8], x[5], 0, 0, 0, 1};
#pragma unroll
  for (int i = 0; i < 16; ++i) t[i] = o[i];
  return true;
}
// sine and cosine of an Euler-angle increment: the angles that survive the shake test are below angle_shake (0.3 rad stock), where
// the Taylor polynomials through x^9 / x^8 are exact to the last bit or two of fp32; larger arguments take the library routine
__device__ __forceinline__ void kf_sincos_small(float x, float* sn, float* cs) {
  if (fabsf(x) < 0.5f) {
    const float x2 = x * x;
    *sn = x * (1.f + x2 * (-1.f / 6.f + x2 * (1.f / 120.f + x2 * (-1.f / 5040.f + x2 * (1.f / 362880.f)))));
    *cs = 1.f + x2 * (-0.5f + x2 * (1.f / 24.f + x2 * (-1.f / 720.f + x2 * (1.f / 40320.f))));
  } else sincosf(x, sn, cs);
}
__device__ __forceinline__ bool vector6_to_transform(const float x[6], float dist_shake2, float cos_shake, float t[16]) {
  float c0, s0, c1, s1, c2, s2;
  kf_sincos_small(x[0], &s0, &c0); kf_sincos_small(x[1], &s1, &c1); kf_sincos_small(x[2], &s2, &c2);
  return transform_from_sincos(x, c0, s0, c1, s1, c2, s2, dist_shake2, cos_shake, t);
}

// The parts' sums of a fold (s_tot[part * 32 + k], all parts written, no barrier yet) -> s_tot[0..26]: four lanes per total add a quarter
// of the parts each, two DPP shifts combine them -- a chain of parts/4 + 2 dependent adds instead of parts, in ONE fixed order that the
// per-step fold (fold_partials) and the persistent loop's fold (fold_partials_tagged) share: the two launch forms of the ICP add the
// same numbers in the same order and therefore arrive at the same bits.  Needs blockDim.x >= 108.
__device__ __forceinline__ void fold_combine_parts(float* s_tot, int parts) {
  __syncthreads();
  float t = 0.f;
  if (threadIdx.x < 27 * 4) {
    const int kk = threadIdx.x >> 2, quarter = threadIdx.x & 3, per = (parts + 3) >> 2;
    for (int p = quarter * per; p < min(parts, (quarter + 1) * per); ++p) t += s_tot[p * 32 + kk];
    t += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(t), 0x111, 0xf, 0xf, true));   // row_shr:1
    t += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(t), 0x112, 0xf, 0xf, true));   // row_shr:2
  }
  __syncthreads();
  if (threadIdx.x < 27 * 4 && (threadIdx.x & 3) == 3) s_tot[threadIdx.x >> 2] = t;
  __syncthreads();
}

// ---- fold the previous step's partial sums: identical order in every workgroup ------------------------------------------
// s_tot must hold 8 x 32 floats; on return s_tot[0..26] are the totals (all threads, after the barrier)
// (blockDim/32 interleaved chains per sum; the loads of a chain are issued four at a time so the chain costs
// ceil(n/4) memory round trips instead of n; the additions keep their fixed order.)  s_tot: 32 x 32 floats.
// n_group (0: none): workgroups g, g + n_group, g + 2 n_group, ... are first added up in that order and count as ONE publisher g -- what the batched
// persistent loop's resident workgroup g publishes after playing exactly those workgroups of the dealing (k_icp_loop_batched): the same numbers in the same order
__device__ __forceinline__ float fold_group_sum(const float* __restrict__ partials, int w, int n_wg, int n_group, int k) {
  float v = partials[w * 32 + k];
  if (n_group > 0) for (int u = w + n_group; u < n_wg; u += n_group) v += partials[u * 32 + k];
  return v;
}
__device__ __forceinline__ void fold_partials(const float* __restrict__ partials, int n_wg, float* s_tot, int n_group = 0) {
  const int k = threadIdx.x & 31, part = threadIdx.x >> 5, parts = blockDim.x >> 5;
  const int n_pub = (n_group > 0 && n_group < n_wg) ? n_group : n_wg;
  if (n_pub == n_wg) n_group = 0;
  float s = 0.f;
  if (k < 27) {
    for (int w = part; w < n_pub; w += 4 * parts) {
      const int w1 = w + parts, w2 = w + 2 * parts, w3 = w + 3 * parts;
      const float v0 = fold_group_sum(partials, w, n_wg, n_group, k);
      const float v1 = (w1 < n_pub) ? fold_group_sum(partials, w1, n_wg, n_group, k) : 0.f;
      const float v2 = (w2 < n_pub) ? fold_group_sum(partials, w2, n_wg, n_group, k) : 0.f;
      const float v3 = (w3 < n_pub) ? fold_group_sum(partials, w3, n_wg, n_group, k) : 0.f;
      s += v0; s += v1; s += v2; s += v3;
    }
  }
  s_tot[part * 32 + k] = s;
  fold_combine_parts(s_tot, parts);
}

// direct_exponential_map (eigen_utils.cpp:84-127) in double, then SDF.cpp:92-100: R' = R_exp^T R_cur, t' = t_cur - R_exp^T t_exp
__device__ __forceinline__ void sdf_apply_increment(const float x[6], const float* cur, float ncur[16]) {
  const double u0 = (double)x[0], u1 = (double)x[1], u2 = (double)x[2], t3 = (double)x[3], t4 = (double)x[4], t5 = (double)x[5];
  const double theta = sqrt(u0 * u0 + u1 * u1 + u2 * u2);
  const double si = sin(theta), co = cos(theta);
  const double sinc = fabs(theta) < 1.0e-8 ? 1.0 : si / theta;
  const double mcosc = fabs(theta) < 2.5e-4 ? 0.5 : (1.0 - co) / theta / theta;
  const double msinc = fabs(theta) < 2.5e-4 ? (1. / 6.0) : (1.0 - si / theta) / theta / theta;
  double R[9];
  R[0] = co + mcosc * u0 * u0;         R[1] = -sinc * u2 + mcosc * u0 * u1; R[2] = sinc * u1 + mcosc * u0 * u2;
  R[3] = sinc * u2 + mcosc * u1 * u0;  R[4] = co + mcosc * u1 * u1;         R[5] = -sinc * u0 + mcosc * u1 * u2;
  R[6] = -sinc * u1 + mcosc * u2 * u0; R[7] = sinc * u0 + mcosc * u2 * u1;  R[8] = co + mcosc * u2 * u2;
  double dt[3];
  dt[0] = t3 * (sinc + u0 * u0 * msinc) + t4 * (u0 * u1 * msinc - u2 * mcosc) + t5 * (u0 * u2 * msinc + u1 * mcosc);
  dt[1] = t3 * (u0 * u1 * msinc + u2 * mcosc) + t4 * (sinc + u1 * u1 * msinc) + t5 * (u1 * u2 * msinc - u0 * mcosc);
  dt[2] = t3 * (u0 * u2 * msinc - u1 * mcosc) + t4 * (u1 * u2 * msinc + u0 * mcosc) + t5 * (sinc + u2 * u2 * msinc);
  float Rt[9], tf[3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) Rt[r * 3 + c] = (float)R[c * 3 + r];
#pragma unroll
  for (int k = 0; k < 3; ++k) tf[k] = (float)dt[k];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) ncur[r * 4 + c] = Rt[r * 3] * cur[c] + Rt[r * 3 + 1] * cur[4 + c] + Rt[r * 3 + 2] * cur[8 + c];
    ncur[r * 4 + 3] = cur[r * 4 + 3] - (Rt[r * 3] * tf[0] + Rt[r * 3 + 1] * tf[1] + Rt[r * 3 + 2] * tf[2]);
  }
  ncur[12] = 0.f; ncur[13] = 0.f; ncur[14] = 0.f; ncur[15] = 1.f;
}

enum { STEP_APPLIED = 0, STEP_LOST_DET = 1, STEP_LOST_SHAKE = 2, STEP_CONVERGED = 3 };

// Apply one Gauss-Newton update from the folded sums in s_tot to s_cur (in place).  Runs on lane 0 of every workgroup with
// identical inputs -> identical outputs.  Returns STEP_* through *s_code (LDS).
//   ICP: minimizePointToPlaneErrFunc (ICP.cpp:117-143) + loop body of estimateCameraPose (:71-82)
//   SDF: loop body of CameraPoseFinderSDF::estimateCameraPose (SDF.cpp:62-101)
// s_next (ICP only, may be null): write the new transform THERE instead of over s_cur and return after ONE workgroup barrier -- the caller flips
// between two buffers (the persistent loop: the copy back and its second barrier were 0.33 us of every Gauss-Newton step); the returned code
// is the one *s_code would carry.
__device__ __forceinline__ int apply_step(const TrackArgs& a, const float* s_tot, float* s_cur, int* s_code, float* s_next = nullptr) {
  if (!a.sdf) {
    // ICP: the determinant test (ICP.cpp:138) and the solve + increment (:143, :71-82) do not depend on each other, so two
    // lanes of DIFFERENT waves run them side by side and lane 0 keeps the solve's result only if the determinant passed.
    // LDS scratch behind the 27 totals (s_tot + 32): [0..15] candidate transform, [16] solve verdict, [17] det verdict.
    float* scratch = const_cast<float*>(s_tot) + 32;
    const unsigned det_lane = blockDim.x > 64u ? 64u : 1u;
#ifdef KF_EXPERIMENTS
#define KF_SOLVE_STAMP(i) do { if (a.dbg) { const unsigned long long t_ = __builtin_amdgcn_s_memrealtime(); atomicAdd(a.dbg + (i), t_ - t_prev_); t_prev_ = t_; } } while (0)
    unsigned long long t_prev_ = a.dbg ? __builtin_amdgcn_s_memrealtime() : 0ull;
#else
#define KF_SOLVE_STAMP(i) do { } while (0)
#endif
#ifdef KF_SOLVE_ONE_LANE
    if (threadIdx.x == det_lane) {
      float A[36], b[6];
      unpack27(s_tot, A, b);
#ifdef KF_EXPERIMENTS
      if (a.exp_nodet) scratch[17] = 0.f; else            // timing experiment (KF_ICP_EXP=12): what does the determinant lane cost the step?
#endif
      scratch[17] = ((double)det6(A) < 1E-10) ? 1.f : 0.f;
      KF_SOLVE_STAMP(6);                                                     // determinant lane: entry -> done
    }
#else
    (void)det_lane;
#endif
    // wave 0 runs the solve, the trigonometry and the increment as ONE chain without touching LDS in between: lane 0 solves; the increment
    // goes to the whole wave as scalars (v_readfirstlane: lane 0 is the wave's first lane); lanes 0-2 take the sine / cosine of one angle
    // each and hand them back the same way (v_readlane); then EVERY lane forms the rotation and the shake verdict from those scalars -- the
    // same expressions, hence the same bits, in all of them -- and twelve lanes compute one element each of T * cur (ICP.cpp:81) instead of
    // lane 0 computing all twelve.  (A third of the instructions of the LDS hand-off form it replaces and no wavefront fences -- and the same
    // 1.2 us per Gauss-Newton step: the phase is the solve's dependent chain plus two workgroup barriers, not instruction issue.)  The
    // determinant (the longer of the two 6x6 factorizations, 1.1 us) runs on a lane of another wave and is joined at the workgroup barrier
    // below; it holds the step back by 0.15 us (KF_ICP_EXP=12 on the experiments build skips it: 145.5 -> 142.7 us per frame).
    if (threadIdx.x < 64) {
      float* vs = scratch;
      float x[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#ifdef KF_SOLVE_ONE_LANE
      if (threadIdx.x == 0) {
        float A[36], b[6];
        unpack27(s_tot, A, b);
        llt_solve6(A, b, x);
        KF_SOLVE_STAMP(0);                                                   // unpack + Cholesky solve
      }
#pragma unroll
      for (int i = 0; i < 6; ++i) x[i] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x[i])));
#else
      {
        bool singular; float det;
        llt_solve6_wave(s_tot, x, singular, det);                            // the whole wave: the increment is wave-uniform, the pivots give the determinant
        if (threadIdx.x == 0) { vs[17] = (singular || (double)det < 1E-10) ? 1.f : 0.f; KF_SOLVE_STAMP(0); }
#ifdef KF_EXPERIMENTS
        if (a.exp_nodet && threadIdx.x == 0) vs[17] = 0.f;
#endif
      }
#endif
      const float ang = threadIdx.x == 0 ? x[0] : (threadIdx.x == 1 ? x[1] : x[2]);
      float sn, cs; kf_sincos_small(ang, &sn, &cs);
      const int sni = __float_as_int(sn), csi = __float_as_int(cs);
      const float c0 = __int_as_float(__builtin_amdgcn_readlane(csi, 0)), s0 = __int_as_float(__builtin_amdgcn_readlane(sni, 0));
      const float c1 = __int_as_float(__builtin_amdgcn_readlane(csi, 1)), s1 = __int_as_float(__builtin_amdgcn_readlane(sni, 1));
      const float c2 = __int_as_float(__builtin_amdgcn_readlane(csi, 2)), s2 = __int_as_float(__builtin_amdgcn_readlane(sni, 2));
      if (threadIdx.x == 0) KF_SOLVE_STAMP(1);                               // increment broadcast + sin/cos + hand-back
      float T[16];
      const bool still = transform_from_sincos(x, c0, s0, c1, s1, c2, s2, a.th.dist_shake2, a.th.cos_shake, T);
      if (threadIdx.x == 0) vs[16] = still ? 0.f : 1.f;
      if (still && threadIdx.x < 16) {
        // ICP.cpp:81 cur = T * cur; T's last row is (0, 0, 0, 1): that row of the product is cur's own last row, bit for bit
        const int i = (int)threadIdx.x >> 2, j = (int)threadIdx.x & 3;
        const float t0 = i == 0 ? T[0] : (i == 1 ? T[4] : T[8]), t1 = i == 0 ? T[1] : (i == 1 ? T[5] : T[9]);
        const float t2 = i == 0 ? T[2] : (i == 1 ? T[6] : T[10]), t3 = i == 0 ? T[3] : (i == 1 ? T[7] : T[11]);
        const float prod = t0 * s_cur[j] + t1 * s_cur[4 + j] + t2 * s_cur[8 + j] + t3 * s_cur[12 + j];
        (s_next ? s_next : vs)[threadIdx.x] = i < 3 ? prod : s_cur[12 + j];
      }
      if (threadIdx.x == 0) KF_SOLVE_STAMP(2);                               // rotation, shake test, T * cur
    }
    __syncthreads();
    if (threadIdx.x == 0) KF_SOLVE_STAMP(3);                                 // workgroup barrier (waits for the determinant lane)
    {
      int code = STEP_APPLIED;                                             // every lane reads the two verdicts (LDS broadcast); sixteen lanes copy
      if (scratch[17] != 0.f) code = STEP_LOST_DET;
      else if (scratch[16] != 0.f) code = STEP_LOST_SHAKE;
      if (s_next) return code;                                             // ping-pong form: every lane holds the verdict, the transform lies in s_next
      if (code == STEP_APPLIED && threadIdx.x < 16) s_cur[threadIdx.x] = scratch[threadIdx.x];
      if (threadIdx.x == 0) *s_code = code;
    }
    __syncthreads();
    if (threadIdx.x == 0) KF_SOLVE_STAMP(4);                                 // verdict + copy + barrier
    return *s_code;
  }
  if (threadIdx.x == 0) {
    float A[36], b[6], x[6], T[16], ncur[16];
    unpack27(s_tot, A, b);
    int code = STEP_APPLIED;
    llt_solve6(A, b, x);
    if (!vector6_to_transform(x, a.th.dist_shake2, a.th.cos_shake, T)) code = STEP_LOST_SHAKE;
    else {
      const float nx = sqrtf(x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3] + x[4] * x[4] + x[5] * x[5]);
      if (nx < 0.001f) code = STEP_CONVERGED;                              // SDF.cpp:87-90: stop before applying x
      else { sdf_apply_increment(x, s_cur, ncur); for (int i = 0; i < 16; ++i) s_cur[i] = ncur[i]; }
    }
    *s_code = code;
  }
  __syncthreads();
  return *s_code;
}

// Common prologue of a step launch: load the running transform, fold + apply the previous step if asked.
// Returns false when the loop has ended (lost / converged); workgroup 0 records that in the track state.
__device__ __forceinline__ bool step_prologue(const TrackArgs& a, float* s_cur, float* s_linv, float* s_tot, int* s_code) {
  KfTrackState* st = a.track;
  if (a.use_state) {
    if (st->status != KF_TRACK_OK || st->converged) return false;          // uniform: written by an earlier launch
    if (threadIdx.x < 16) s_cur[threadIdx.x] = st->cur[a.step & 1][threadIdx.x];
    else if (threadIdx.x < 32) s_linv[threadIdx.x - 16] = st->last_inv[threadIdx.x - 16];
  } else {
    if (threadIdx.x < 16) s_cur[threadIdx.x] = a.cur_val.m[threadIdx.x];
    else if (threadIdx.x < 32) s_linv[threadIdx.x - 16] = a.linv_val.m[threadIdx.x - 16];
  }
  __syncthreads();
  if (!a.consume) {
    if (a.use_state && blockIdx.x == 0 && threadIdx.x < 16) st->cur[(a.step + 1) & 1][threadIdx.x] = s_cur[threadIdx.x];
    return true;
  }
  if (a.ext_prev) fold_partials(a.ext_prev, 1, s_tot);
  else fold_partials(a.partials + (size_t)((a.step + 1) & 1) * KF_ICP_MAX_WG * 32, a.n_prev_wg, s_tot, a.fold_group);
  apply_step(a, s_tot, s_cur, s_code);
  const int code = *s_code;
  if (blockIdx.x == 0) {
    if (threadIdx.x < 27) st->reduced[threadIdx.x] = s_tot[threadIdx.x];
    if (code == STEP_APPLIED) {
      if (threadIdx.x < 16) st->cur[(a.step + 1) & 1][threadIdx.x] = s_cur[threadIdx.x];
      if (threadIdx.x == 0) st->iterations += 1;
    } else if (threadIdx.x == 0) {
      if (code == STEP_CONVERGED) { st->converged = 1; for (int i = 0; i < 16; ++i) st->pose[i] = s_cur[i]; kf_mat44_inverse(s_cur, st->pose_inv); st->tracked = 1; }
      else { st->status = code; st->tracked = 0; }                          // KF_TRACK_LOST_* share the STEP_LOST_* values
    }
  }
  return code == STEP_APPLIED;
}

// workgroup reduction of the 27 sums (DPP row totals -> LDS -> fixed-order adds), written as this workgroup's partial for the
// NEXT launch to fold.  s_rows: 27 x (blockDim / 16) floats.
__device__ __forceinline__ void store_partial(float acc[27], float* partials_out, float* s_rows) {
  const int rows = blockDim.x >> 4, row = threadIdx.x >> 4;
#pragma unroll
  for (int k = 0; k < 27; ++k) {
    const float s = kf_row_scan_sum(acc[k]);
    if ((threadIdx.x & 15) == 15) s_rows[k * rows + row] = s;
  }
  __syncthreads();
  if (threadIdx.x < 27) {
    float s = s_rows[threadIdx.x * rows];
    for (int w = 1; w < rows; ++w) s += s_rows[threadIdx.x * rows + w];
    partials_out[blockIdx.x * 32 + threadIdx.x] = s;
  }
}

// ---- ICP ------------------------------------------------------------------------------------------------------------
// findCorrs (:17-60) + buildPointToPlaneSolverRows (:7-16), split so the ICP_PX pixels of a lane overlap their memory round trips:
// stage A (icp_project) needs only the lane's own vertex/normal and yields the model-map index; stage B (icp_finish)
// consumes the gathered model vertex/normal.  Both are straight-line code: every gate is a boolean, there is no early exit.  A pixel
// without a correspondence gets index 0 and `false`; its projection is computed all the same (vcp.z may be zero, tiny or negative:
// kf_project's two `/` and the saturating conversion give a number for every input, NaN included, and the bounds test judges it).
__device__ __forceinline__ bool icp_project(const TrackArgs& a, const float* cur, const float* linv, float4 iv, float4 in_,
                                            float4& vg, float4& ng, int& mi) {
  const bool own = !kf_is_zero4(in_);
  vg = kf_mat_vec(cur, iv);
  ng = kf_mat_vec(cur, in_);
  const float4 vcp = kf_mat_vec(linv, vg);
  const int2 sp = kf_project(kf3(vcp.x, vcp.y, vcp.z), a.cam);
  const bool in_x = (sp.x >= 0) & (sp.x < a.cam.cols), in_y = (sp.y >= 0) & (sp.y < a.cam.rows);
  const bool ok = own & in_x & in_y;
  mi = ok ? (int)((unsigned)sp.y * (unsigned)a.cam.cols + (unsigned)sp.x) : 0;   // (unsigned: a saturated row's product wraps and is dropped)
  return ok;
}
// the gates on the gathered model entry, as ONE predicate computed from nt and vt without a branch -- every loaded value has an unconditional
// use, so no load can be moved under a condition -- each with the comparison sense of the reference: `x > t` rejects, a NaN passes
__device__ __forceinline__ bool icp_finish(const TrackArgs& a, float4 vg, float4 ng, float4 vt, float4 nt) {
  const bool has_n = !kf_is_zero4(nt);
  // `norm(p - q) > dist || norm(n_tgt x n_in) > sin` (CalPointToPlaneErrSolverParams.cu:52) on the squares: two square roots fewer per pixel
  const float3 dv = kf3(vt.x - vg.x, vt.y - vg.y, vt.z - vg.z), cr = kf_cross(kf3(nt.x, nt.y, nt.z), kf3(ng.x, ng.y, ng.z));
  const bool far = kf_dot(dv, dv) > a.th.dist_thres2, steep = kf_dot(cr, cr) > a.th.sin_thres2;
  return has_n & !far & !steep;
}
__device__ __forceinline__ void icp_row(float4 vg, float4 vt, float4 nt, float row[7]) {
  const float3 p = kf3(vt.x, vt.y, vt.z), q = kf3(vg.x, vg.y, vg.z), n = kf3(nt.x, nt.y, nt.z);
  row[0] = q.y * n.z - q.z * n.y; row[1] = q.z * n.x - q.x * n.z; row[2] = q.x * n.y - q.y * n.x;
  row[3] = n.x; row[4] = n.y; row[5] = n.z;
  row[6] = kf_dot(n, kf_sub(p, q));
}

// ICP_THREADS, ICP_PX, icp_level_geometry (pixels per lane and publishers of a level) and the fold's slot rule: shared with the host's test program
#include "icp_fold_slots.h"
// index of this lane's j-th pixel: pixels are dealt to the grid_l workgroups in 64-pixel chunks, round robin -- every workgroup sees
// the same mix of surface and background, so they all reach the exchange of partial sums at about the same time (contiguous blocks
// did not)
__device__ __forceinline__ int icp_dealt_pixel_of(int j, int grid_l, int wg) {
  return (((int)(threadIdx.x >> 6) * grid_l + wg) + j * ((ICP_THREADS / 64) * grid_l)) * 64 + (int)(threadIdx.x & 63);
}
__device__ __forceinline__ int icp_dealt_pixel(int j, int grid_l) { return icp_dealt_pixel_of(j, grid_l, (int)blockIdx.x); }
// The 27 sums of a lane, declared as `IcpSums sums; float* acc = sums.v;`.  The struct is the point: a plain local `float acc[27]` is turned into ONE
// <27 x float> value before anything is inlined or unrolled (the back end's promotion of private arrays to vectors), it then lives in a 32-register
// tuple, and every merge point of a branch copies or shifts the whole tuple -- 16-deep v_mov_b64 ladders, blocks of 27 re-zeroing moves, 163 moves in
// the pixel phase.  A struct member is left alone and splits into 27 scalars, which an exec-masked region updates in place.
struct IcpSums { float v[27]; };
// one Gauss-Newton step's pixel phase for this lane's NPX pixels: correspondences + the 27 products, fused accumulation; acc is written, not added to.
// Straight-line up to the products: NPX projections (the running transform is read from LDS once for all of them), then the 2 x NPX model-map
// gathers, all of them ahead of the first wait -- a pixel without a correspondence reads entry 0 and drops it --, then each pixel's gates as one
// boolean and its 27 fused multiply-adds under that one predicate, in place, pixels in the order j = 0, 1, 2.  What this form is written against (the
// listing showed each): a load whose only uses are conditional gets sunk under the condition, and with it a wait of its own -- the first pixel's
// normal, a wait, the zero test, then its vertex and a second wait: two dependent round trips per step; an early `continue` / `return false` around
// the sums multiplies the merge points.  (profiles/icp_pixel_gates.txt)
template <int NPX>
__device__ __forceinline__ void icp_accumulate_px(const TrackArgs& a, const float* s_cur, const float* s_linv, const float4 iv[ICP_PX], const float4 in_[ICP_PX],
                                                  const float4* __restrict__ model_v, const float4* __restrict__ model_n, float acc[27]) {
  float4 vg[NPX], ng[NPX], vt[NPX], nt[NPX]; int mi[NPX]; bool ok[NPX];
#pragma unroll
  for (int j = 0; j < NPX; ++j) ok[j] = icp_project(a, s_cur, s_linv, iv[j], in_[j], vg[j], ng[j], mi[j]);
#pragma unroll
  for (int j = 0; j < NPX; ++j) { nt[j] = model_n[mi[j]]; vt[j] = model_v[mi[j]]; }
#pragma unroll
  for (int j = 0; j < NPX; ++j) ok[j] = ok[j] & icp_finish(a, vg[j], ng[j], vt[j], nt[j]);
#pragma unroll
  for (int k = 0; k < 27; ++k) acc[k] = 0.f;
#pragma unroll
  for (int j = 0; j < NPX; ++j) {
    if (ok[j]) {                                                           // a rejected pixel leaves every sum untouched (exec mask): its data may hold NaN / Inf
      float row[7];
      icp_row(vg[j], vt[j], nt[j], row);
      int s = 0;
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = r; c < 7; ++c) { acc[s] = __builtin_fmaf(row[r], row[c], acc[s]); ++s; }   // :92-105 packing; fused multiply-add: half the instructions, the better rounding (the sums are tolerance-checked)
    }
  }
}
// px_n: how many of the lane's ICP_PX pixels the level deals (wave-uniform: icp_level_geometry; the others are zeros, which every gate rejects).  The coarse
// levels deal one: their steps run the one-pixel instantiation and neither project nor gather for the two empty slots.
__device__ __forceinline__ void icp_accumulate(const TrackArgs& a, const float* s_cur, const float* s_linv, const float4 iv[ICP_PX], const float4 in_[ICP_PX],
                                               const float4* __restrict__ model_v, const float4* __restrict__ model_n, float acc[27], int px_n) {
  if (px_n == 1) icp_accumulate_px<1>(a, s_cur, s_linv, iv, in_, model_v, model_n, acc);
  else icp_accumulate_px<ICP_PX>(a, s_cur, s_linv, iv, in_, model_v, model_n, acc);
}
// workgroup total of the 27 sums (512 lanes): 16-lane row totals by DPP, one LDS word per (sum, row), then 4 lanes per sum add 8 row
// totals each and two DPP shifts combine the four partial chains (fixed order).  Returns true on the one lane that ends up holding
// sum k in sw.  s_wave: 27 x 32 floats.
__device__ __forceinline__ bool icp_wg_reduce(float acc[27], float* s_wave, int& k, float& sw) {
  const int row = threadIdx.x >> 4;
#pragma unroll
  for (int i = 0; i < 27; ++i) acc[i] = kf_row_scan_sum(acc[i]);      // 27 independent DPP chains, free to interleave
  if ((threadIdx.x & 15) == 15) {
#pragma unroll
    for (int i = 0; i < 27; ++i) s_wave[i * (ICP_THREADS / 16) + row] = acc[i];
  }
  __syncthreads();
  k = threadIdx.x >> 2; sw = 0.f;
  if (threadIdx.x < 27 * 4) {
    const int part = threadIdx.x & 3;
    sw = s_wave[k * (ICP_THREADS / 16) + part * 8];
#pragma unroll
    for (int w = 1; w < 8; ++w) sw += s_wave[k * (ICP_THREADS / 16) + part * 8 + w];
    sw += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(sw), 0x111, 0xf, 0xf, true));   // row_shr:1
    sw += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(sw), 0x112, 0xf, 0xf, true));   // row_shr:2
    return part == 3;
  }
  return false;
}
__global__ void __launch_bounds__(ICP_THREADS) k_icp_step(TrackArgs a) {
  __shared__ float s_cur[16], s_linv[16];
  __shared__ float s_wave[27 * (ICP_THREADS / 16)], s_tot[(ICP_THREADS / 32) * 32];
  __shared__ int s_code;
  // the lane's own vertices / normals do not depend on the running transform: request them before the fold + solve
  const int npx = a.px_end > 0 ? a.px_end : a.cam.cols * a.cam.rows;
  float4 iv[ICP_PX], in_[ICP_PX];
#pragma unroll
  for (int j = 0; j < ICP_PX; ++j) {
    // px_l > 0: the persistent loop's dealing (same pixels in the same lanes -> same bits); else a contiguous range per workgroup
    const int i = a.px_l > 0 ? icp_dealt_pixel(j, a.deal_grid) : a.px_begin + (int)blockIdx.x * (ICP_THREADS * ICP_PX) + (int)threadIdx.x + j * ICP_THREADS;
    iv[j] = make_float4(0.f, 0.f, 0.f, 0.f); in_[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if ((a.px_l == 0 || j < a.px_l) && i < npx) { iv[j] = a.new_v[i]; in_[j] = a.new_n[i]; }
  }
  if (!step_prologue(a, s_cur, s_linv, s_tot, &s_code)) return;
  IcpSums sums; float* acc = sums.v;
  icp_accumulate(a, s_cur, s_linv, iv, in_, a.model_v, a.model_n, acc, a.px_l > 0 ? a.px_l : ICP_PX);
  int k; float sw;
  if (icp_wg_reduce(acc, s_wave, k, sw)) a.partials[(size_t)(a.step & 1) * KF_ICP_MAX_WG * 32 + blockIdx.x * 32 + k] = sw;
}

// ---- persistent ICP: the whole 19-step loop in ONE launch ---------------------------------------------------------------------
// One 512-lane workgroup per CU (no scratch at <= 256 VGPRs), 150 of them at VGA, all co-resident.  Between two Gauss-Newton
// steps nothing but the 27 partial sums of each workgroup has to cross CUs, so there is no grid barrier: a workgroup
// publishes its sums as tagged 64-bit words (one write-through store each) and every workgroup folds all of them, polling
// until the tags are current (fold_partials_tagged below; MI355X_MICROARCH.md "Valid forms": sc1 store -> sc1 load hand-off).
// A step then costs one store->load propagation (~1 us) instead of a dependent dispatch (~5 us measured here) plus a cold
// start of the 30 KB straight-line step code, which is what bounded the one-launch-per-step form at ~22 us per step; the
// two-level counter barrier this replaces cost three dependent atomic round trips (~4 us) per step.
// What every persistent tracking launch (k_icp_loop, k_icp_loop_batched, k_sdf_loop) needs to exchange its partial sums and to end (track_loop_end)
struct TrackLoopArgs {
  unsigned long long* slots;                     // KF_ICP_LOOP_STEPS x KF_ICP_LOOP_MAX_WG x 32 tagged partial sums, one array per step
  unsigned tag_base;                             // this launch's sequence number (host counter x 64); tag = tag_base + step
  KfTrackState* track;
  unsigned* stall_word;                          // pinned host word: set when the loop gives up waiting, polled by the next tracking call
  int n_loop;                                    // the loop's workgroups = the publishers of a step
  int play_dead;                                 // fault injection (kf_inject_track_stall): this workgroup exits at once, as if it had never become resident
  int exp_mode;                                  // diagnostics only (KF_ICP_EXP): 1 = skip the solve (timing), 7 = shader-clock stamps per phase
  // The fusion pass's brick cull as the TAIL of this launch (cull.h): it needs nothing but the committed pose, which every workgroup of the loop holds
  // once the last step is applied -- so k_integrate_cull and one kernel boundary leave the stream (k_icp_loop and k_sdf_loop; the host arms it when the
  // previous kf_integrate_volume left its parameters behind and the volume is small enough: kf_arm_tail_cull).
  int cull_on;
  IntegrateArgs cull;
};
struct IcpLoopArgs : TrackLoopArgs {
  const float4* new_v[KF_MAX_LEVELS]; const float4* new_n[KF_MAX_LEVELS];
  const float4* model_v[KF_MAX_LEVELS]; const float4* model_n[KF_MAX_LEVELS];
  KfCam cam[KF_MAX_LEVELS];
  int iters[KF_MAX_LEVELS]; int levels;
  TrackThresholds th;
  // Riders: workgroups [n_loop, gridDim.x) do not take part in the loop -- they carry the NEXT frame's u16 -> f32 + gate + bilateral filter
  // (kf_prefetch_frame, requested before kf_icp_track).  The loop keeps one workgroup on each of ~200 CUs busy for ~0.14 ms at two waves per
  // SIMD and leaves the other CUs idle; the riders are dispatched behind the loop's workgroups (they cannot displace them), wait for
  // nobody, and are long done when the loop ends.  gridDim.x == n_loop: none.
  int n_virtual;                                 // workgroups the pixel dealing is defined for (= the workgroups level 0 needs at ICP_PX pixels per lane, what the per-step form
                                                 // launches): n_loop in k_icp_loop; larger in k_icp_loop_batched, whose n_loop resident workgroups each play several of them
  KfBilateralArgs bil; int bil_gx, bil_tiles, bil_fast;
};

// A workgroup gives up waiting for the others' partial sums after ICP_WAIT_LIMIT ticks of the 100 MHz wall clock (s_memrealtime) = 20 ms -- a
// legitimate wait is tens of microseconds; the clock is read every 64th poll (~1-1.5 us each).  Giving up costs latency, not the frame: one
// workgroup then finishes the frame's Gauss-Newton loop alone (track_loop_end below), with the same bits.
#define ICP_WAIT_LIMIT 2000000ull
#ifndef KF_ICP_POLL_PIPE
#define KF_ICP_POLL_PIPE 2        // s_sleep between two polls (anything from 0 to 8 measures alike; -DKF_ICP_POLL_SINGLE selects the older one-poll loop)
#endif
#ifndef KF_ICP_POLL_DEPTH
#define KF_ICP_POLL_DEPTH 1       // polls (sets of a batch's words) a lane keeps in flight
#endif
#ifndef KF_ICP_POLL_DEPTH_SMALL
#define KF_ICP_POLL_DEPTH_SMALL KF_ICP_POLL_DEPTH      // the same where a set is at most 4 words (tuning: profiles/icp_fold_shapes.txt)
#endif
#ifdef KF_ICP_POLL_SINGLE
#undef ICP_FOLD_LADDER
#define ICP_FOLD_LADDER(X)        // the one-poll loop (and the experiments that live in it) always polls ICP_FOLD_BATCH slots
#endif
// Partial sums of the persistent loop travel as 64-bit (value, tag) words: the tag is the launch's sequence number plus the
// Gauss-Newton step, every step has its own slot array, and a word is published by ONE 8-byte write-through store -- so a
// reader needs no barrier and no flag: it polls the words it is about to add until their tags are current.  The adds run
// in a fixed order (workgroup-major within a part, then the parts): every workgroup of the loop arrives at the same bits.  The
// per-step launch form (k_icp_step) deals pixels to workgroups differently, so the two forms agree to tolerance, not bitwise.
//
// One batch of one lane: the words of the publishers w0, w0 + parts, ... (NS of them, icp_fold_batch_slots) of sum k are polled until all their tags are
// current, then added to s in ascending order.  What a poll costs is what it loads: every workgroup of the loop reads every publisher's 27 words, 43 KB per
// poll and CU at VGA level 0 and 8.6 MB over the chip, through the same fabric the publishers' stores have to cross.  Hence (profiles/icp_fold_shapes.txt,
// tracking stage at C2 in us):
//  * a batch polls no more slots than its level has publishers for -- the slots left out were + 0.f on a sum that starts at +0.f and cannot become -0.f,
//    the same bits (13 slots in every batch 120.1, {3, 10, 13} 114.9, {2, 4, 7, 10, 13} 116.4);
//  * ONE poll in flight, and none once the set is current.  A second one does not find a publication sooner, it delays it: 114.9 with one, 142.3 with
//    two really in flight (level 0: everyone folded 4.3 instead of 2.8 us after the first publish), 116.7 with two for the sets of 3 words alone;
//    a sweep that is still on its way when the fold is through costs 6 more.
//    (The loop this one replaces asked for two and, behind a per-lane exit, got one and a half: the compiler waited for the younger set before it
//    re-issued the older one, and moved both between registers every turn -- 128.9.)
//
// PAIRS (icp_fold_slots.h).  The sums 2m and 2m + 1 of a publisher are one aligned 16-byte unit {value, tag, value, tag} of its slot row, and a lane of the
// ICP loops' fold polls such a unit with ONE 16-byte sc1 load (8-byte sc1 loads move their bytes at 0.54-0.70 x the rate of 16-byte ones), checks both tags
// and adds two chains: 14 lanes per part instead of 27, half the load instructions per poll.  Each half stays a granule of its own -- its tag sits next to
// its value, written by one 8-byte store, and a reader trusts a half by that tag alone -- so nothing rests on the 16 bytes being read as one: a half that is
// stale, or left from an earlier launch, fails its tag and is polled again.  Word 27, the second half of pair 13, is padding: nobody writes it and its
// tag is not looked at.  The loads are raw buffer loads with aux 16 (sc1) on a descriptor over one step's slot array.
// Measured (profiles/icp_pair_exchange.txt, tracking stage at C2 in us): single words 114.4, 16-byte polls 109.8, 16-byte polls AND one 16-byte store per
// pair 111.2, the 16-byte store alone 114.6 -- the publishers keep their 8-byte stores (-DKF_ICP_STORE16: the pair store; -DKF_ICP_POLL8: single-word polls).
// The SDF loop keeps single words on both sides: the pair poll costs it 16 more bytes of scratch at 256 VGPRs and 3.5 us of its stage.
typedef unsigned kf_v4u __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t icp_slot_rsrc(const unsigned long long* step_slots) {      // (step_slots: wave-uniform)
  return __builtin_amdgcn_make_buffer_rsrc((void*)step_slots, 0, KF_ICP_LOOP_MAX_WG * 32 * (int)sizeof(unsigned long long), 0x00020000);
}
// Publisher w's 27 sums after icp_wg_reduce / sdf_wg_reduce -- lane 4 k + 3 holds sum k in `sw`, the lanes from 108 on 0.f -- go out as tagged words, one
// write-through store each.  Every lane calls.
__device__ __forceinline__ void icp_publish_tagged(unsigned long long* step_slots, int w, unsigned tag, float sw) {
#ifdef KF_ICP_STORE16
  // variant: the holder of a pair's second sum fetches the first from four lanes below (same DPP row, same wave) and stores both, the padding half as {0, tag}
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, __float_as_int(sw), 0x114, 0xf, 0xf, true);     // row_shr:4
  const int m = icp_pair_stored_by((int)threadIdx.x);
  if (m >= 0) {
    const kf_v4u q = {lo, tag, __float_as_uint(sw), tag};
    __builtin_amdgcn_raw_buffer_store_b128(q, icp_slot_rsrc(step_slots), (int)icp_pair_byte_offset(w, m), 0, 16);
  }
#else
  if (threadIdx.x < ICP_SUMS * 4 && (threadIdx.x & 3) == 3)
    __hip_atomic_store(step_slots + w * 32 + (threadIdx.x >> 2), ((unsigned long long)tag << 32) | (unsigned long long)__float_as_uint(sw), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}
// One batch of one lane of the pair fold: the 16-byte units of pair m of the publishers w0, w0 + parts, ... (NS of them) are polled until both tags of every
// unit are current, then added to the two chains s0 (sum 2m) and s1 (sum 2m + 1) in ascending order -- the operands and the order of fold_batch_tagged's
// chains for k = 2m and 2m + 1.  One poll in flight, one exit at the foot taken by the wave as a whole, the give-up test uniform: as below.
// (Two sub-lanes sharing a lane's units, the running sums handed from one to the other: built and measured slower, 113.0 against 110.7 -- not kept.)
template <int NS>
__device__ __forceinline__ void fold_batch_pairs(__amdgpu_buffer_rsrc_t rsrc, int n_wg, int w0, int parts, int m, unsigned tag, float& s0, float& s1, int* s_abort,
                                                 const unsigned* rescue_tag, unsigned tag_base, unsigned long long& t_wait0) {
  unsigned spins = 0;
  kf_v4u u[NS];
  int off[NS];
  // (a unit without a publisher -- the ragged last row: the lane's own first unit once more, the value dropped below; no branch around a load)
#pragma unroll
  for (int j = 0; j < NS; ++j) { const int w = w0 + j * parts; off[j] = (int)icp_pair_byte_offset(w < n_wg ? w : w0, m); }
#pragma unroll
  for (int j = 0; j < NS; ++j) u[j] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off[j], 0, 16);
#ifdef KF_ICP_STORE16
  const unsigned pad = ~0u;
#else
  const unsigned pad = icp_pair_half_is_sum(m, 1) ? ~0u : 0u;                   // the padding word is never written: its tag is not looked at
#endif
  float v0[NS], v1[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) { v0[j] = 0.f; v1[j] = 0.f; }
  bool done = false;                                                            // the same in every lane of the wave
  do {
    if (++spins == 64u) {                                                       // never spin forever
      spins = 0u;
      // (somebody else of this launch already gave up and one workgroup is finishing the frame alone: nothing more will be published)
      bool give_up = rescue_tag && (unsigned)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(rescue_tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == tag_base;
      if (!give_up) {
        const unsigned long long now = __builtin_amdgcn_s_memrealtime();
        const unsigned long long t0 = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(t_wait0 >> 32)) << 32) |
                                      (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)t_wait0);
        if (t0 == 0ull) t_wait0 = now; else give_up = now - t0 > ICP_WAIT_LIMIT;
      }
      if (give_up) { *s_abort = 1; done = true; }                               // (the fold is void: its caller looks at s_abort first)
    }
    unsigned stale = 0u;
#pragma unroll
    for (int j = 0; j < NS; ++j) stale |= (u[j].y ^ tag) | ((u[j].w ^ tag) & pad);
    if (!done && __ballot(stale != 0u) == 0ull) {                               // current: its values are the ones added
#pragma unroll
      for (int j = 0; j < NS; ++j) { v0[j] = __uint_as_float(u[j].x); v1[j] = __uint_as_float(u[j].z); }
      done = true;
    }
    if (!done) {
      __builtin_amdgcn_s_sleep(KF_ICP_POLL_PIPE);
      asm volatile("" ::: "memory");                                            // a poll is a new look at memory, every turn
#pragma unroll
      for (int j = 0; j < NS; ++j) u[j] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off[j], 0, 16);
    }
  } while (!done);
#pragma unroll
  for (int j = 0; j < NS; ++j) { const bool real = w0 + j * parts < n_wg; s0 += real ? v0[j] : 0.f; s1 += real ? v1[j] : 0.f; }
}
template <int NS>
__device__ __forceinline__ float fold_batch_tagged(const unsigned long long* slots, int n_wg, int w0, int parts, int k, unsigned tag, float s, int* s_abort,
                                                   int exp_mode, const unsigned* rescue_tag, unsigned tag_base, unsigned long long& t_wait0) {
  unsigned spins = 0;
#ifndef KF_ICP_POLL_SINGLE
  // D sets of the batch's words in flight (D = 1 unless a tuning build asks for more): the oldest is looked at while the younger ones are on their way; the
  // sets take turns in place -- the loop is unrolled by the depth, and no set is ever copied into another's registers.
  constexpr int D = NS <= 4 ? KF_ICP_POLL_DEPTH_SMALL : KF_ICP_POLL_DEPTH;
  // the batch's addresses are fixed before the loop and a lane without a publisher for slot j polls its own FIRST word once more
  // (not one shared word: the slots of a ragged last row would all hammer one publisher's line; the value is dropped below): no branch around a load, no
  // exec-mask juggling per slot -- the poll iteration was 265 instructions, i.e. the loop noticed a publication up to 0.4 us late
  unsigned long long u[D][NS];
  const unsigned long long* src[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) { const int w = w0 + j * parts; src[j] = slots + (size_t)((w < n_wg ? w : w0) * 32 + k); }
#pragma unroll
  for (int d = 0; d < D; ++d) {
    if (d) __builtin_amdgcn_s_sleep(KF_ICP_POLL_PIPE);
#pragma unroll
    for (int j = 0; j < NS; ++j) u[d][j] = __hip_atomic_load(src[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // The wave leaves as one, when a set is current in all its lanes: a word that is current stays so (a slot is written once per launch and step), and a
  // lane that is through would wait for its neighbours anyway.  The loop has ONE exit, at its foot, and the set that is found current is copied out where
  // it is found.  With more than one set in flight nothing in the loop issues a poll under a condition either, and the turn is played to its end (its
  // last polls land in registers nobody reads): behind a per-lane exit, an exit per set or a poll under a condition the compiler cannot tell how many
  // loads are in flight where a set is looked at -- it waits for all of them and moves whole sets between registers.
  float v[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) v[j] = 0.f;
  bool done = false;                                                            // the same in every lane of the wave
  do {
    // never spin forever: looked at once per turn of the sets, i.e. every 64 polls as before
    if (++spins == 64u / D) {
      spins = 0u;
      // (somebody else of this launch already gave up and one workgroup is finishing the frame alone: nothing more will be published)
      bool give_up = rescue_tag && (unsigned)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(rescue_tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == tag_base;
      if (!give_up) {
        const unsigned long long now = __builtin_amdgcn_s_memrealtime();
        const unsigned long long t0 = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(t_wait0 >> 32)) << 32) |
                                      (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)t_wait0);
        if (t0 == 0ull) t_wait0 = now; else give_up = now - t0 > ICP_WAIT_LIMIT;
      }
      if (give_up) { *s_abort = 1; done = true; }                               // (the fold is void: its caller looks at s_abort first)
    }
#pragma unroll
    for (int d = 0; d < D; ++d) {                                               // set d is the oldest in flight
      unsigned stale = 0u;
#pragma unroll
      for (int j = 0; j < NS; ++j) stale |= (unsigned)(u[d][j] >> 32) ^ tag;
      if (!done && __ballot(stale != 0u) == 0ull) {                             // current: its values are the ones added
#pragma unroll
        for (int j = 0; j < NS; ++j) v[j] = __uint_as_float((unsigned)u[d][j]);
        done = true;
      }
      if (D > 1 || !done) {
        if (!done) __builtin_amdgcn_s_sleep(KF_ICP_POLL_PIPE);
#pragma unroll
        for (int j = 0; j < NS; ++j) u[d][j] = __hip_atomic_load(src[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  } while (!done);
#pragma unroll
  for (int j = 0; j < NS; ++j) s += (w0 + j * parts < n_wg) ? v[j] : 0.f;
  return s;
#else
  float v[NS];
  for (;;) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      const int w = w0 + j * parts;
      v[j] = 0.f;
      if (w < n_wg && !(exp_mode == 3 && w >= 16 && k != 0)) {     // (experiment 3: wait for every workgroup, move 1/27 of the words)
        const unsigned long long u = __hip_atomic_load(&slots[w * 32 + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v[j] = __uint_as_float((unsigned)u);
        ok = ok && (unsigned)(u >> 32) == tag;
      }
    }
    if (ok) break;
    __builtin_amdgcn_s_sleep(2);
    if ((++spins & 63u) == 0u) {                                             // never spin forever
      const unsigned long long now = __builtin_amdgcn_s_memrealtime();
      if (t_wait0 == 0ull) t_wait0 = now; else if (now - t_wait0 > ICP_WAIT_LIMIT) { *s_abort = 1; break; }
    }
  }
#pragma unroll
  for (int j = 0; j < NS; ++j) s += v[j];
  return s;
#endif
}
// PAIRS: the fold's lanes poll 16-byte units (fold_batch_pairs: 14 lanes per part, in the workgroup's first parts / 4 waves; the other waves go straight to
// the barrier) -- or single words (fold_batch_tagged: 27 lanes per part, every wave).  The same adds in the same order either way.
#ifdef KF_ICP_POLL8
#define ICP_FOLD_PAIRS_DEFAULT false
#else
#define ICP_FOLD_PAIRS_DEFAULT true
#endif
template <bool PAIRS = ICP_FOLD_PAIRS_DEFAULT>
__device__ __forceinline__ void fold_partials_tagged(const unsigned long long* slots, int n_wg, unsigned tag, float* s_tot, int* s_abort, int exp_mode = 0,
                                                     const unsigned* rescue_tag = nullptr, unsigned tag_base = 0u) {
  const int parts = blockDim.x >> 5;
  unsigned long long t_wait0 = 0ull;
  if constexpr (PAIRS) {
    int part, m;
    if (icp_fold_pair_lane((int)threadIdx.x, parts, part, m)) {
      const __amdgpu_buffer_rsrc_t rsrc = icp_slot_rsrc(slots);
      float s0 = 0.f, s1 = 0.f;
      int base = 0;                                                             // the batch's first publisher: the same in every lane
      for (int w0 = part; w0 < n_wg; w0 += ICP_FOLD_BATCH * parts, base += ICP_FOLD_BATCH * parts) {
        const int ns = icp_fold_batch_slots(n_wg, base, parts);                 // the poll's form: a uniform branch outside the poll loop
#define ICP_FOLD_FORM(n) if (ns == (n)) fold_batch_pairs<n>(rsrc, n_wg, w0, parts, m, tag, s0, s1, s_abort, rescue_tag, tag_base, t_wait0); else
        ICP_FOLD_LADDER(ICP_FOLD_FORM)
#undef ICP_FOLD_FORM
        fold_batch_pairs<ICP_FOLD_BATCH>(rsrc, n_wg, w0, parts, m, tag, s0, s1, s_abort, rescue_tag, tag_base, t_wait0);
      }
      s_tot[part * 32 + 2 * m] = s0;
      if (icp_pair_half_is_sum(m, 1)) s_tot[part * 32 + 2 * m + 1] = s1;     // (the padding half's chain goes nowhere)
    }
    fold_combine_parts(s_tot, parts);     // the parts' sums, in the order the per-step fold uses too
    return;
  }
  const int k = threadIdx.x & 31, part = threadIdx.x >> 5;
  float s = 0.f;
  if (k < 27) {
    int base = 0;                                                               // the batch's first publisher: the same in every lane
    for (int w0 = part; w0 < n_wg; w0 += ICP_FOLD_BATCH * parts, base += ICP_FOLD_BATCH * parts) {
      // the poll's form is chosen here, by a uniform branch outside the poll loop
      const int ns = icp_fold_batch_slots(n_wg, base, parts);
#define ICP_FOLD_FORM(n) if (ns == (n)) s = fold_batch_tagged<n>(slots, n_wg, w0, parts, k, tag, s, s_abort, exp_mode, rescue_tag, tag_base, t_wait0); else
      ICP_FOLD_LADDER(ICP_FOLD_FORM)
#undef ICP_FOLD_FORM
      s = fold_batch_tagged<ICP_FOLD_BATCH>(slots, n_wg, w0, parts, k, tag, s, s_abort, exp_mode, rescue_tag, tag_base, t_wait0);
    }
  }
  s_tot[part * 32 + k] = s;
  fold_combine_parts(s_tot, parts);       // the parts' sums, in the order the per-step fold uses too
}


// ---- the end of a persistent tracking launch -------------------------------------------------------------------------------------------------
// How a persistent loop left its Gauss-Newton steps: at fold `fold` (of `n_pub` publishers) with its update's `code` -- STEP_PENDING: that fold is still
// to be done and applied -- or timed out waiting in that fold.  `applied`: the updates applied so far.
enum { STEP_PENDING = -1 };
struct LoopOutcome { int code, fold, n_pub, applied; bool timed_out; };
enum { LOOP_DONE = 0, LOOP_SOLO = 1 };

// the whole verdict of a tracking call (a persistent launch may have run without k_track_begin's reset).  One lane calls.
__device__ __forceinline__ void track_verdict(KfTrackState* st, int status, int iterations, int converged, int rescued) {
  st->status = status; st->tracked = status == KF_TRACK_OK ? 1 : 0; st->iterations = iterations; st->converged = converged; st->rescued = rescued;
}
// Who ends a persistent tracking launch?  One compare-and-swap on KfTrackState::commit_word decides for every workgroup: (tag_base | 1) the launch's own
// workgroups, (tag_base | 2) ONE workgroup that finishes it alone after a time-out.  `want`: 1 or 2; `seen0`: the word as this workgroup read it when it
// started (an older launch's value, normally).  Returns the winner (1 or 2); *mine: this call's compare-and-swap set the word.  One lane calls.
__device__ __forceinline__ unsigned track_commit_decide(KfTrackState* st, unsigned tag_base, unsigned want, unsigned seen0, bool* mine) {
  unsigned expect = seen0;
  *mine = false;
  for (;;) {
    if ((expect & ~63u) == tag_base) return expect & 63u;                 // this launch's word is set: somebody decided
    const unsigned seen = atomicCAS(&st->commit_word, expect, tag_base | want);
    if (seen == expect) { *mine = true; return want; }
    expect = seen;                                                          // (an older word replaced by this launch's)
  }
}
// The loop's workgroups wait for each other, so they must all be resident; when some are not (a foreign process holds CUs -- the cross-process
// registry of ctx.hip only sees processes of this library) a fold times out.  The frame is NOT given up.  Every workgroup of a persistent launch
// (k_icp_loop, k_icp_loop_batched, k_sdf_loop) ends here, with its loop's outcome:
//  * the loop went through: track_commit_decide settles the party.  The launch's own workgroups: workgroup 0 commits (SDF.cpp:103, ICP.cpp:84; a
//    lost frame keeps the old pose) and every workgroup runs its own share of the tail.  A workgroup that claimed the launch: this one leaves.
//  * a fold timed out: the first workgroup to claim the launch raises rescue_tag (whoever still polls leaves) and the stall word, and gets LOOP_SOLO:
//    the caller runs the frame's whole loop again by itself, playing every publisher of the launch in turn -- the same pixel dealing, pixel phase,
//    reduction, tagged slots and fold, hence the SAME BITS as the loop (tests/test_gpu_track_forms.py injects the fault) -- and comes back with
//    `solo`: it commits and runs every share of the tail.  It costs milliseconds, not the frame; the host backs off to per-step launches afterwards.
//    Somebody else's claim: leave.  The launch's own workgroups ended it after all: the fold that timed out is then the launch's last executed one
//    (a workgroup that passed it proves every partial sum of it published), so it is folded again and applied to the transform this workgroup holds
//    -- the step the others took -- and the workgroup ends with them: the verdict if it is workgroup 0, its own share of the tail.
// `apply`: the tracker's update from s_tot (STEP_*, behind a workgroup barrier), leaving the running transform in *s_cur; s_tinv: 16 floats of LDS the loop
// no longer needs (the committed pose's inverse goes there).  Every lane calls.
template <bool PAIRS = ICP_FOLD_PAIRS_DEFAULT, class Apply>
__device__ __forceinline__ int track_loop_end(const TrackLoopArgs& L, unsigned commit_seen0, bool solo, LoopOutcome o, float* s_tot, int* s_abort,
                                              float* const& s_cur, Apply& apply, float* s_tinv) {
  KfTrackState* st = L.track;
  __shared__ unsigned s_who;                                                   // 1 the launch's own workgroups end it, 2 a claimant, 3 this workgroup claimed it
  __shared__ unsigned s_cull[17];
  for (;;) {
    if (o.code == STEP_PENDING) {
      fold_partials_tagged<PAIRS>(L.slots + (size_t)o.fold * KF_ICP_LOOP_MAX_WG * 32, o.n_pub, L.tag_base + (unsigned)o.fold, s_tot, s_abort, 0,
                           solo ? nullptr : &st->rescue_tag, L.tag_base);
      o.timed_out = *s_abort != 0;
    }
    // a lane of an idle wave settles it, while wave 0 solves a pending step; s_who is read behind the next workgroup barrier
    if (!solo && threadIdx.x == 128) {
      bool mine;
      unsigned who = track_commit_decide(st, L.tag_base, o.timed_out ? 2u : 1u, commit_seen0, &mine);
      if (o.timed_out && who == 2u && mine) {
        __hip_atomic_store(&st->rescue_tag, L.tag_base, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(L.stall_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        who = 3u;
      }
      s_who = who;
    }
    if (!o.timed_out) break;
    __syncthreads();
    if (solo) {                                                                // (a solo fold waits for nobody: unreachable)
      if (threadIdx.x == 0) track_verdict(st, KF_TRACK_STALLED, o.applied, 0, 1);
      return LOOP_DONE;
    }
    if (s_who != 1u) return s_who == 3u ? LOOP_SOLO : LOOP_DONE;
    __syncthreads();
    if (threadIdx.x == 0) *s_abort = 0;                                        // every sum of the fold is published: it cannot wait again
    o.code = STEP_PENDING; o.timed_out = false;
  }
  if (o.code == STEP_PENDING) { o.code = apply(); if (o.code == STEP_APPLIED) ++o.applied; }
  else __syncthreads();
  if (!solo && s_who == 2u) return LOOP_DONE;                                  // a workgroup claimed the launch: it commits and runs every share of the tail
  const bool good = o.code == STEP_APPLIED || o.code == STEP_CONVERGED;        // (uniform over the launch: every workgroup arrives at the same verdict)
  const bool writer = solo || blockIdx.x == 0, tail = L.cull_on && good;
  if (writer) {
    if (threadIdx.x < 27 && KF_EXP_MODE(L) != 7) st->reduced[threadIdx.x] = s_tot[threadIdx.x];
    if (good && threadIdx.x < 16) st->pose[threadIdx.x] = s_cur[threadIdx.x];
    if (threadIdx.x == 0) track_verdict(st, good ? KF_TRACK_OK : o.code, o.applied, o.code == STEP_CONVERGED ? 1 : 0, solo ? 1 : 0);
  }
  if (!good || (!writer && !tail)) return LOOP_DONE;
  if (threadIdx.x == 64) kf_mat44_inverse(s_cur, s_tinv);                      // a lane of another wave: world -> camera (integrateVolume.cu:84), for the fusion pass and the tail
  __syncthreads();
  if (writer && threadIdx.x < 16) st->pose_inv[threadIdx.x] = s_tinv[threadIdx.x];
  if (tail) {                                                                  // every workgroup holds the same pose bits, hence the same inverse
    if (solo) { for (int w = 0; w < L.n_loop; ++w) cull_tail(L.cull, s_tinv, w, L.n_loop, s_cull); }
    else cull_tail(L.cull, s_tinv, (int)blockIdx.x, L.n_loop, s_cull);
  }
  return LOOP_DONE;
}

// a rider workgroup of a tracking launch: two 64x4 tiles of the NEXT frame's gate + bilateral filter (IcpLoopArgs::bil)
__device__ __forceinline__ void icp_rider(const IcpLoopArgs& L) {
  __shared__ float s_bil[2 * (BIL_TX + 8) * (BIL_TY + 8)];
  const int half = (int)(threadIdx.x >> 8), t = ((int)blockIdx.x - L.n_loop) * 2 + half;
  const int tt = t < L.bil_tiles ? t : L.bil_tiles;                          // past the last tile: a row below the image, nothing is touched
  float* tile = s_bil + half * ((BIL_TX + 8) * (BIL_TY + 8));
  if (L.bil_fast) kf_bilateral_tile<4, true>(L.bil, tt % L.bil_gx, tt / L.bil_gx, (int)(threadIdx.x & 255), tile);
  else kf_bilateral_tile<4, false>(L.bil, tt % L.bil_gx, tt / L.bil_gx, (int)(threadIdx.x & 255), tile);
}

// this lane's pixels of workgroup w of a level's dealing (zeros where w holds no pixels, beyond px_l and beyond the image)
__device__ __forceinline__ void icp_load_pixels(const float4* __restrict__ new_v, const float4* __restrict__ new_n, int w, int grid_l, int px_l, int npx,
                                                float4 iv[ICP_PX], float4 in_[ICP_PX]) {
#pragma unroll
  for (int j = 0; j < ICP_PX; ++j) {
    const int i = icp_dealt_pixel_of(j, grid_l, w);
    iv[j] = make_float4(0.f, 0.f, 0.f, 0.f); in_[j] = iv[j];
    if (w < grid_l && j < px_l && i < npx) { iv[j] = new_v[i]; in_[j] = new_n[i]; }
  }
}
// One publisher's share of a Gauss-Newton step of level l: publisher g plays the workgroups g, g + n_loop, ... of the dealing in turn -- each turn exactly a
// workgroup's pixel phase and reduction in the per-step form's dealing -- adds their sums up HERE, in that order, and publishes them as ONE set of 27 tagged
// words: a step's fold then walks n_loop x 27 words (205 at 1280x960), not grid_l x 27 (800).  The per-step form folds its partials in the same groups
// (fold_partials, TrackArgs::fold_group): the same bits.  ivn / inn: the first turn's pixels, requested by the caller; every later turn's are requested one
// turn ahead (a turn's own loads, ~1 us from L2 / the Infinity Cache, would otherwise be exposed three or four times per step).
__device__ __forceinline__ void icp_publish(const IcpLoopArgs& L, const TrackArgs& a, int l, int step, int g, int grid_l, int px_l,
                                            const float* s_cur, const float* s_linv, float* s_wave, float4 ivn[ICP_PX], float4 inn[ICP_PX]) {
  const int npx = a.cam.cols * a.cam.rows;
  float gsum = 0.f;
  for (int w = g; w < grid_l; w += L.n_loop) {
    float4 iv[ICP_PX], in_[ICP_PX];
#pragma unroll
    for (int j = 0; j < ICP_PX; ++j) { iv[j] = ivn[j]; in_[j] = inn[j]; }
    if (w + L.n_loop < grid_l) icp_load_pixels(L.new_v[l], L.new_n[l], w + L.n_loop, grid_l, px_l, npx, ivn, inn);
    IcpSums sums; float* acc = sums.v;
    icp_accumulate(a, s_cur, s_linv, iv, in_, L.model_v[l], L.model_n[l], acc, px_l);
    int k; float sw;
    const bool holder = icp_wg_reduce(acc, s_wave, k, sw);
    if (holder) gsum = (w == g) ? sw : gsum + sw;
    __syncthreads();                                                           // s_wave is reused by the next turn
    if (w + L.n_loop >= grid_l)                                                // the last turn: publish (gsum: 0.f in every lane that holds no sum)
      icp_publish_tagged(L.slots + (size_t)step * KF_ICP_LOOP_MAX_WG * 32, g, L.tag_base + (unsigned)step, gsum);
  }
}

// The Gauss-Newton steps of a persistent ICP launch, coarse -> fine (ICP.cpp:65), up to the last step's fold -- or an earlier verdict, or a fold that timed out.
// BATCHED (k_icp_loop_batched, the solo finish): every step plays this workgroup's publisher (icp_publish) -- or every publisher in turn, `solo`.  A lane's
// pixels cannot stay in registers across steps (several turns share them): they are re-read every step, from L2 / the Infinity Cache (78 MB per step at
// 1280x960 fit the 256 MiB cache).  Otherwise (k_icp_loop) every workgroup is one workgroup of the dealing, and its pixels stay in registers for all the
// iterations of a level.  `apply` (track_loop_end) flips the running transform s_pose[cur_buf] between the two buffers.
template <bool BATCHED, class Apply>
__device__ __forceinline__ LoopOutcome icp_loop_steps(const IcpLoopArgs& L, TrackArgs& a, bool solo, Apply& apply, float (*s_pose)[16], int& cur_buf,
                                                      float*& s_cur, const float* s_linv, float* s_wave, float* s_tot, int* s_abort) {
  KfTrackState* st = L.track;
  LoopOutcome o = {STEP_APPLIED, 0, 0, 0, false};
  int step = 0;
  // diagnostic build path (KF_ICP_EXP=7): workgroup 0 accumulates shader-clock ticks per segment into track->reduced
  const bool stamp = !BATCHED && KF_EXP_MODE(L) == 7 && blockIdx.x == 0 && threadIdx.x == 0;
  unsigned long long t_last = 0; float seg[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#define KF_STAMP(i) do { if (stamp) { unsigned long long t_now = __builtin_amdgcn_s_memtime(); seg[i] += (float)(t_now - t_last); t_last = t_now; } } while (0)
  if (stamp) t_last = __builtin_amdgcn_s_memtime();
  for (int l = L.levels - 1; l >= 0; --l) {
    a.cam = L.cam[l];
    const int npx = a.cam.cols * a.cam.rows;
    int px_l, grid_l;
    icp_level_geometry(npx, L.n_virtual, l, px_l, grid_l);
    const int g0 = solo ? 0 : (int)blockIdx.x;                                 // this workgroup's (first) publisher
    float4 iv[ICP_PX], in_[ICP_PX];
    // this lane's own vertices / normals depend neither on the running transform nor on the iteration: they are loaded once per pyramid level and stay in
    // registers for all of its iterations (the reference re-reads them 4 / 5 / 10 times).  (A conditional load on purpose: the branch-free form that helps
    // the per-step gathers in icp_accumulate costs 21 us per frame here -- measured, profiles/r03_icp_step.txt -- and these loads happen once per level.)
    if constexpr (!BATCHED) icp_load_pixels(L.new_v[l], L.new_n[l], g0, grid_l, px_l, npx, iv, in_);
    for (int it = 0; it < L.iters[l]; ++it, ++step) {
      KF_STAMP(0);
      // batched: this step's first turn's pixels are requested before the previous step's sums are waited for (they depend on the level only)
      if constexpr (BATCHED) icp_load_pixels(L.new_v[l], L.new_n[l], g0, grid_l, px_l, npx, iv, in_);
      if (step > 0) {
        o.fold = step - 1;
#ifdef KF_EXPERIMENTS
        if (!BATCHED && KF_EXP_MODE(L) == 14) {
          // experiment (VERDICT r3 #3b, "leader fold"): workgroup 0 alone folds and solves; everybody else polls ONE line -- the new transform as 16
          // tagged words (+ the verdict) -- instead of folding the 200 x 27 partial sums itself.  Same bits; timing: profiles/r04_icp_exchange.txt
          unsigned long long* bc = L.slots + (size_t)28 * KF_ICP_LOOP_MAX_WG * 32 + (size_t)(step - 1) * 32;
          const unsigned tag = L.tag_base + (unsigned)(step - 1);
          __shared__ int s_bc_code;
          if (blockIdx.x == 0) {
            fold_partials_tagged(L.slots + (size_t)(step - 1) * KF_ICP_LOOP_MAX_WG * 32, o.n_pub, tag, s_tot, s_abort);
            o.code = apply();
            if (threadIdx.x < 17) {
              const unsigned bits = threadIdx.x < 16 ? __float_as_uint(s_cur[threadIdx.x]) : (unsigned)o.code;
              __hip_atomic_store(bc + threadIdx.x, ((unsigned long long)tag << 32) | bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
          } else {
            if (threadIdx.x < 17) {
              unsigned long long u;
              do { u = __hip_atomic_load(bc + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); if ((unsigned)(u >> 32) != tag) __builtin_amdgcn_s_sleep(1); } while ((unsigned)(u >> 32) != tag);
              if (threadIdx.x < 16) s_pose[cur_buf ^ 1][threadIdx.x] = __uint_as_float((unsigned)u); else s_bc_code = (int)(unsigned)u;
            }
            __syncthreads();
            o.code = s_bc_code;
            if (o.code == STEP_APPLIED) { cur_buf ^= 1; s_cur = s_pose[cur_buf]; }
          }
          __syncthreads();
        } else
#endif
        {
          fold_partials_tagged(L.slots + (size_t)(step - 1) * KF_ICP_LOOP_MAX_WG * 32, (KF_EXP_MODE(L) == 2 && o.n_pub > 16) ? 16 : o.n_pub, L.tag_base + (unsigned)(step - 1),
                               s_tot, s_abort, KF_EXP_MODE(L), solo ? nullptr : &st->rescue_tag, L.tag_base);
          if (*s_abort) { o.timed_out = true; return o; }
          KF_STAMP(1);
#ifdef KF_EXPERIMENTS
          if (KF_EXP_MODE(L) == 9 && blockIdx.x == 5 && (threadIdx.x & 63) == 0)     // per-wave: fold of the previous step done
            L.slots[(size_t)25 * KF_ICP_LOOP_MAX_WG * 32 + (size_t)step * 32 + 16 + (threadIdx.x >> 6)] = __builtin_amdgcn_s_memrealtime();
          if (KF_EXP_MODE(L) == 8 && threadIdx.x == 0) L.slots[(size_t)24 * KF_ICP_LOOP_MAX_WG * 32 + (size_t)(step - 1) * 1024 + blockIdx.x * 2 + 1] = __builtin_amdgcn_s_memrealtime();
#endif
          if (KF_EXP_MODE(L) == 1) { o.code = STEP_APPLIED; __syncthreads(); }    // timing only: skip the 6x6 solve
          else o.code = apply();
        }
        if (o.code != STEP_APPLIED) return o;                                  // same verdict in every workgroup
        ++o.applied;
      }
      KF_STAMP(2);
      if constexpr (BATCHED) {
        const int g1 = solo ? (grid_l < L.n_loop ? grid_l : L.n_loop) : g0 + 1;
        for (int g = g0; g < g1; ++g) {
          if (g > g0) icp_load_pixels(L.new_v[l], L.new_n[l], g, grid_l, px_l, npx, iv, in_);
          icp_publish(L, a, l, step, g, grid_l, px_l, s_cur, s_linv, s_wave, iv, in_);
        }
        o.n_pub = grid_l < L.n_loop ? grid_l : L.n_loop;
      } else {
        if ((int)blockIdx.x < grid_l) {
          IcpSums sums; float* acc = sums.v;
          icp_accumulate(a, s_cur, s_linv, iv, in_, L.model_v[l], L.model_n[l], acc, px_l);
          KF_STAMP(3);
#ifdef KF_EXPERIMENTS
          if (KF_EXP_MODE(L) == 9 && blockIdx.x == 5 && (threadIdx.x & 63) == 0)     // per-wave: pixel phase done (workgroup 5)
            L.slots[(size_t)25 * KF_ICP_LOOP_MAX_WG * 32 + (size_t)step * 32 + (threadIdx.x >> 6)] = __builtin_amdgcn_s_memrealtime();
#endif
          // workgroup partial, stored write-through (sc1) for the other CUs
          int k; float sw;
          icp_wg_reduce(acc, s_wave, k, sw);
          icp_publish_tagged(L.slots + (size_t)step * KF_ICP_LOOP_MAX_WG * 32, (int)blockIdx.x, L.tag_base + (unsigned)step, sw);
        }
        KF_STAMP(4);
        KF_STAMP(5);
#ifdef KF_EXPERIMENTS
        if (KF_EXP_MODE(L) == 9 && blockIdx.x == 5 && (threadIdx.x & 63) == 0)       // per-wave: partial published / wave idle again
          L.slots[(size_t)25 * KF_ICP_LOOP_MAX_WG * 32 + (size_t)step * 32 + 8 + (threadIdx.x >> 6)] = __builtin_amdgcn_s_memrealtime();
        if (KF_EXP_MODE(L) == 8 && threadIdx.x == 0) L.slots[(size_t)24 * KF_ICP_LOOP_MAX_WG * 32 + (size_t)step * 1024 + blockIdx.x * 2] = __builtin_amdgcn_s_memrealtime();
#endif
        o.n_pub = grid_l;
      }
    }
  }
#undef KF_STAMP
  if (stamp) { for (int i = 0; i < 6; ++i) st->reduced[20 + i] = seg[i]; }
  o.code = STEP_PENDING; o.fold = step - 1;                                   // the last step's system: folded and applied by track_loop_end
  return o;
}

// Both persistent ICP kernels: the loop, then track_loop_end -- and after a time-out that this workgroup claimed, the frame's whole loop again by itself,
// from the committed pose (which nobody else can have changed since the kernel started: the claim excludes every other committer).
template <bool BATCHED>
__device__ __forceinline__ void icp_loop(const IcpLoopArgs& L) {
  if ((int)blockIdx.x >= L.n_loop) { icp_rider(L); return; }                   // a rider: two 64x4 filter tiles (bilateral_tile.h), then done
  __shared__ float s_pose[2][16], s_linv[16];                                  // the running transform lives in one of two buffers: a step writes the other one
  __shared__ float s_wave[27 * (ICP_THREADS / 16)], s_tot[(ICP_THREADS / 32) * 32];
  __shared__ int s_abort;
  int cur_buf = 0;
  float* s_cur = s_pose[0];
  KfTrackState* st = L.track;
  // a workgroup that only becomes resident after the launch has been given up has nothing to do; `play_dead`: fault injection (kf_inject_track_stall) --
  // the last workgroup behaves as if it never became resident.  (The pose and the two words are requested together: one round trip.)
  const float pose_e = st->pose[threadIdx.x & 15];                             // ICP.cpp:62 cur_transform = _pose
  const unsigned commit_seen0 = __hip_atomic_load(&st->commit_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (__hip_atomic_load(&st->rescue_tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == L.tag_base) return;
  if (L.play_dead && (int)blockIdx.x == L.n_loop - 1) return;
  TrackArgs a;
  a.th = L.th; a.sdf = 0;
#ifdef KF_EXPERIMENTS
  a.dbg = (!BATCHED && KF_EXP_MODE(L) == 11 && blockIdx.x == 0) ? L.slots + (size_t)26 * KF_ICP_LOOP_MAX_WG * 32 : nullptr;
  a.exp_nodet = !BATCHED && KF_EXP_MODE(L) == 12;
#endif
  auto start = [&](bool solo) {                                               // the running transform and last_transform_inv (ICP.cpp:62-63)
    cur_buf = 0; s_cur = s_pose[0];
    if (threadIdx.x < 16) s_cur[threadIdx.x] = solo ? st->pose[threadIdx.x] : pose_e;
    if (threadIdx.x == 0) s_abort = 0;
    __syncthreads();
    if (threadIdx.x == 0) kf_mat44_inverse(s_cur, s_linv);
    __syncthreads();
  };
  auto apply = [&]() {
    const int code = apply_step(a, s_tot, s_cur, nullptr, s_pose[cur_buf ^ 1]);
    if (code == STEP_APPLIED) { cur_buf ^= 1; s_cur = s_pose[cur_buf]; }
    return code;
  };
  start(false);
  LoopOutcome o = icp_loop_steps<BATCHED>(L, a, false, apply, s_pose, cur_buf, s_cur, s_linv, s_wave, s_tot, &s_abort);
  if (track_loop_end(L, commit_seen0, false, o, s_tot, &s_abort, s_cur, apply, s_linv) != LOOP_SOLO) return;
#ifdef KF_ICP_NO_SOLO          // A/B variant only (tools/build_variant.sh): what the solo path costs the hot loop in registers / code placement
  if (threadIdx.x == 0) track_verdict(st, KF_TRACK_STALLED, 0, 0, 0);
#else
#ifdef KF_EXPERIMENTS
  a.dbg = nullptr; a.exp_nodet = false;
#endif
  start(true);
  o = icp_loop_steps<true>(L, a, true, apply, s_pose, cur_buf, s_cur, s_linv, s_wave, s_tot, &s_abort);
  track_loop_end(L, commit_seen0, true, o, s_tot, &s_abort, s_cur, apply, s_linv);
#endif
}
__global__ void __launch_bounds__(ICP_THREADS) k_icp_loop(IcpLoopArgs L) { icp_loop<false>(L); }
// ---- the same loop for images whose level 0 needs more workgroups than the chip holds at once (1280x960: 800) ------------------------------------------
// The per-step form pays a kernel boundary per Gauss-Newton step and folds 800 x 27 partials from a cold start each time (24 us per step at 1280x960:
// 0.46 ms of BASELINE config C5's frame).  Here n_loop resident workgroups play the n_virtual workgroups of the dealing in turn (icp_publish), so the
// tagged slots hold the same partial sums and the same fold arrives at the SAME BITS as k_icp_step (tests/test_gpu_track_forms.py).
__global__ void __launch_bounds__(ICP_THREADS) k_icp_loop_batched(IcpLoopArgs L) { icp_loop<true>(L); }

// ---- SDF tracker ------------------------------------------------------------------------------------------------------
// the six perturbed transforms delta * cur for +w1, -w1, +w2, -w2, +w3, -w3 (CalSDFErrSolverParams.cu:118-133) into s_m[1..6]; s_m[0] = cur.  96 lanes.
__device__ __forceinline__ void sdf_perturbed_transforms(float (*s_m)[16], float w_h) {
  if (threadIdx.x < 96) {
    const int mi = threadIdx.x >> 4, e = threadIdx.x & 15, r = e >> 2, cidx = e & 3;
    const int axis = mi >> 1; const float sg = (mi & 1) ? -1.f : 1.f;     // second matrix of a pair flips the sign
    float d[4] = {0.f, 0.f, 0.f, 0.f}; d[r] = 1.f;
    if (axis == 0) { if (r == 1) d[2] = -sg * w_h; if (r == 2) d[1] = sg * w_h; }          // m23 = -w, m32 = +w
    else if (axis == 1) { if (r == 0) d[2] = sg * w_h; if (r == 2) d[0] = -sg * w_h; }     // m13 = +w, m31 = -w
    else { if (r == 0) d[1] = -sg * w_h; if (r == 1) d[0] = sg * w_h; }                    // m12 = -w, m21 = +w
    s_m[1 + mi][e] = d[0] * s_m[0][cidx] + d[1] * s_m[0][4 + cidx] + d[2] * s_m[0][8 + cidx] + d[3] * s_m[0][12 + cidx];
  }
}
// one pixel into the 27 running sums (computeSDFSolverbufKernel, CalSDFErrSolverParams.cu:68-108: row[i] * row[j], i <= j); d = 0: no depth, no row
template <typename AD>
__device__ __forceinline__ void sdf_accumulate_pixel(const KfVolume& vol, const AD& S, const float (*s_m)[16], const KfCam& cam, int i, float d, float w_h, float v_h,
                                                     const KfRecip& rS, float rcell, bool slab, float acc[27]) {
  const float3 p = kf_depth_to_skeleton((unsigned)(i % cam.cols), (unsigned)(i / cam.cols), d, cam);
  float row[7];
  const bool ok = sdf_pixel_row<AD>(vol, S, s_m, p, w_h, v_h, rS, rcell, slab, row) && d != 0.f;
  if (!ok) {
#pragma unroll
    for (int k = 0; k < 7; ++k) row[k] = 0.f;                            // (a rejected pixel adds +0.0 twenty-seven times: the sums keep their bits)
  }
  int s = 0;
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = r; c < 7; ++c) { acc[s] = __builtin_fmaf(row[r], row[c], acc[s]); ++s; }
}
template <typename AD>
__global__ void __launch_bounds__(TRK_THREADS) k_sdf_step(TrackArgs a) {
  __shared__ float s_m[7][16];                 // cur, then delta*cur for +w1,-w1,+w2,-w2,+w3,-w3 (CalSDFErrSolverParams.cu:118-133)
  __shared__ float s_linv[16];
  __shared__ float s_wave[27 * (TRK_THREADS / 16)], s_tot[32 * 32];
  __shared__ int s_code;
  if (!step_prologue(a, s_m[0], s_linv, s_tot, &s_code)) return;
  const float w_h = 0.001f;                                               // :119 `float w_h = 0.001;`
  const float v_h = a.vol.size / (float)a.vol.res;                        // :120
  sdf_perturbed_transforms(s_m, w_h);
  __syncthreads();
  float acc[27];
#pragma unroll
  for (int k = 0; k < 27; ++k) acc[k] = 0.f;
  const KfRecip rS = kf_recip(a.vol.size);
  const float rcell = 1.0f / a.vol.cell;
  const AD S(a.vol);
  // a wave takes 8x8 pixel tiles (see k_sdf_loop: a compact footprint in the volume = few cache lines per gather instruction), grid-stride over the tiles
  const int tiles_x = (a.cam.cols + 7) >> 3, n_tiles = tiles_x * ((a.cam.rows + 7) >> 3);
  for (int tile = (int)blockIdx.x * (TRK_THREADS / 64) + (int)(threadIdx.x >> 6); tile < n_tiles; tile += (int)gridDim.x * (TRK_THREADS / 64)) {
    const int x = (tile % tiles_x) * 8 + (int)(threadIdx.x & 7), y = (tile / tiles_x) * 8 + (int)((threadIdx.x >> 3) & 7);
    const bool in = x < a.cam.cols && y < a.cam.rows;
    const int i = in ? y * a.cam.cols + x : 0;
    const float d = in ? a.depth[i] : 0.f;
    if (__ballot(d != 0.f) == 0ull) continue;                             // a wave without a single depth value: nothing to look up
    // z-slabs: a pixel belongs to the slab that owns the voxel of its world point; every rank sums its own pixels and the
    // 27-float systems are all-reduced.  The 13 lookups reach at most the halo (kf_sdf_partition_step checks it).
    sdf_accumulate_pixel<AD>(a.vol, S, s_m, a.cam, i, d, w_h, v_h, rS, rcell, a.slab_pixels != 0, acc);
  }
  store_partial(acc, a.partials + (size_t)(a.step & 1) * KF_ICP_MAX_WG * 32, s_wave);
}
// volumes whose stored voxels fill less than 4 GB are addressed through a raw buffer descriptor (sdf_rows.h)
static inline bool sdf_buffer_addressing(const KfVolume& v) {
  return (unsigned long long)(v.bz1 - v.bz0) * v.nb * v.nb * KF_BRICK_VOX * sizeof(float2) < 0xFFFFFFFFull && v.nb <= 1024;
}
static inline void launch_sdf_step(kf_ctx* c, int grid, const TrackArgs& a) {
  if (sdf_buffer_addressing(a.vol)) hipLaunchKernelGGL(k_sdf_step<SdfBufAddr>, dim3(grid), dim3(TRK_THREADS), 0, c->stream, a);
  else hipLaunchKernelGGL(k_sdf_step<SdfFlatAddr>, dim3(grid), dim3(TRK_THREADS), 0, c->stream, a);
}

// ---- SDF tracker, persistent: the whole Gauss-Newton loop of CameraPoseFinderSDF::estimateCameraPose (SDF.cpp:57-103) in ONE launch ---------------
// Round 4 launched one k_sdf_step per iteration (+ begin + finish): at VGA 300 workgroups of 4 waves -- about one wave per SIMD -- each walking 4 pixels x 13
// dependent lookups, 60 us per executed iteration (profiles/r05_c3_before_kernel_stats.csv), three of them per frame on Scene S.  Here the iterations share a
// launch the way the ICP loop's do: n_loop co-resident 512-lane workgroups, pixels dealt in 64-pixel chunks round robin (icp_dealt_pixel_of: every workgroup
// sees the same mix of surface and background), the 27 sums per workgroup by DPP + LDS, published as tagged 64-bit words and folded by everybody in one fixed
// order (fold_partials_tagged), the 6x6 system solved by a wave (llt_solve6_wave), the shake / convergence tests and the fp64 exponential map on that wave,
// and the loop leaves as soon as the increment's norm drops below 1e-3 (SDF.cpp:87-90) -- no launches that find `converged` and return.
// It ends as the ICP loop does (track_loop_end); a workgroup that finishes the launch alone runs the same loop again playing every workgroup of the
// dealing in turn (`first` / `stride`).
#ifndef SDF_THREADS
#define SDF_THREADS ICP_THREADS
#endif
struct SdfLoopArgs : TrackLoopArgs {
  KfVolume vol; const float* depth; KfCam cam;
  int max_iter;
  TrackThresholds th;
  int px_l;                                      // pixels per lane = 8x8 tiles per wave: ceil(tiles / (waves per workgroup * n_loop))
  int slab_pixels;
};
// direct_exponential_map (eigen_utils.cpp:84-127) + SDF.cpp:92-100 with the three even series in t = theta^2 instead of sqrt / sin / cos / five fp64 divisions
// on the one-lane chain of every iteration: sinc = sum (-t)^k / (2k+1)!, mcosc = sum (-t)^k / (2k+2)!, msinc = sum (-t)^k / (2k+3)!, cos = 1 - t mcosc.
// Nine terms: below 1e-19 for theta <= 0.5 (the shake test admits 0.3 rad with the stock parameters); larger increments take the library routines.  The
// reference's small-angle constants (sinc = 1 below 1e-8, mcosc = 1/2 and msinc = 1/6 below 2.5e-4) are kept.  Tolerance side (pose within 1e-4).
__device__ __forceinline__ void sdf_apply_increment_series(const float x[6], const float* cur, float ncur[16]) {
  const double u0 = (double)x[0], u1 = (double)x[1], u2 = (double)x[2];
  const double t = u0 * u0 + u1 * u1 + u2 * u2;
  if (!(t <= 0.25)) { sdf_apply_increment(x, cur, ncur); return; }
  // three independent Horner chains in -t (they interleave on the one lane that runs them)
  double a = 1.0 / 355687428096000.0, b = 1.0 / 6402373705728000.0, c = 1.0 / 121645100408832000.0;                    // 1/17!, 1/18!, 1/19!
  a = 1.0 / 1307674368000.0 - t * a;  b = 1.0 / 20922789888000.0 - t * b;  c = 1.0 / 355687428096000.0 - t * c;        // 1/15!, 1/16!, 1/17!
  a = 1.0 / 6227020800.0 - t * a;     b = 1.0 / 87178291200.0 - t * b;     c = 1.0 / 1307674368000.0 - t * c;          // 1/13!, 1/14!, 1/15!
  a = 1.0 / 39916800.0 - t * a;       b = 1.0 / 479001600.0 - t * b;       c = 1.0 / 6227020800.0 - t * c;             // 1/11!, 1/12!, 1/13!
  a = 1.0 / 362880.0 - t * a;         b = 1.0 / 3628800.0 - t * b;         c = 1.0 / 39916800.0 - t * c;               // 1/9!, 1/10!, 1/11!
  a = 1.0 / 5040.0 - t * a;           b = 1.0 / 40320.0 - t * b;           c = 1.0 / 362880.0 - t * c;                 // 1/7!, 1/8!, 1/9!
  a = 1.0 / 120.0 - t * a;            b = 1.0 / 720.0 - t * b;             c = 1.0 / 5040.0 - t * c;                   // 1/5!, 1/6!, 1/7!
  a = 1.0 / 6.0 - t * a;              b = 1.0 / 24.0 - t * b;              c = 1.0 / 120.0 - t * c;                    // 1/3!, 1/4!, 1/5!
  a = 1.0 - t * a;                    b = 0.5 - t * b;                     c = 1.0 / 6.0 - t * c;
  const double co = 1.0 - t * b;                                          // cos(theta), from the un-thresholded series
  const double sinc = t < 1.0e-16 ? 1.0 : a;                                           // fabs(theta) < 1e-8
  const double mcosc = t < 6.25e-8 ? 0.5 : b;                                          // fabs(theta) < 2.5e-4
  const double msinc = t < 6.25e-8 ? (1. / 6.0) : c;
  const double t3 = (double)x[3], t4 = (double)x[4], t5 = (double)x[5];
  double R[9];
  R[0] = co + mcosc * u0 * u0;         R[1] = -sinc * u2 + mcosc * u0 * u1; R[2] = sinc * u1 + mcosc * u0 * u2;
  R[3] = sinc * u2 + mcosc * u1 * u0;  R[4] = co + mcosc * u1 * u1;         R[5] = -sinc * u0 + mcosc * u1 * u2;
  R[6] = -sinc * u1 + mcosc * u2 * u0; R[7] = sinc * u0 + mcosc * u2 * u1;  R[8] = co + mcosc * u2 * u2;
  double dt[3];
  dt[0] = t3 * (sinc + u0 * u0 * msinc) + t4 * (u0 * u1 * msinc - u2 * mcosc) + t5 * (u0 * u2 * msinc + u1 * mcosc);
  dt[1] = t3 * (u0 * u1 * msinc + u2 * mcosc) + t4 * (sinc + u1 * u1 * msinc) + t5 * (u1 * u2 * msinc - u0 * mcosc);
  dt[2] = t3 * (u0 * u2 * msinc - u1 * mcosc) + t4 * (u1 * u2 * msinc + u0 * mcosc) + t5 * (sinc + u2 * u2 * msinc);
  float Rt[9], tf[3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) Rt[r * 3 + cc] = (float)R[cc * 3 + r];
#pragma unroll
  for (int k = 0; k < 3; ++k) tf[k] = (float)dt[k];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) ncur[r * 4 + cc] = Rt[r * 3] * cur[cc] + Rt[r * 3 + 1] * cur[4 + cc] + Rt[r * 3 + 2] * cur[8 + cc];
    ncur[r * 4 + 3] = cur[r * 4 + 3] - (Rt[r * 3] * tf[0] + Rt[r * 3 + 1] * tf[1] + Rt[r * 3 + 2] * tf[2]);
  }
  ncur[12] = 0.f; ncur[13] = 0.f; ncur[14] = 0.f; ncur[15] = 1.f;
}
// One iteration's update (SDF.cpp:79-100) by wave 0 from the folded sums: solve, shake test, convergence test, exponential map.  Every workgroup runs it on
// identical inputs -> identical transforms.  On STEP_APPLIED s_cur holds the new transform when the function returns (all lanes, after its barrier).
__device__ __forceinline__ int sdf_apply_step_wave(const float* s_tot, float* s_cur, float dist_shake2, float cos_shake, int* s_code) {
  if (threadIdx.x < 64) {
    float x[6]; bool singular; float det;
    llt_solve6_wave(s_tot, x, singular, det);                                // (A.llt().solve(b): no pivot test in the reference -- a non-positive pivot yields NaN there and here)
    const float ang = threadIdx.x == 0 ? x[0] : (threadIdx.x == 1 ? x[1] : x[2]);
    float sn, cs; kf_sincos_small(ang, &sn, &cs);
    const int sni = __float_as_int(sn), csi = __float_as_int(cs);
    const float c0 = __int_as_float(__builtin_amdgcn_readlane(csi, 0)), s0 = __int_as_float(__builtin_amdgcn_readlane(sni, 0));
    const float c1 = __int_as_float(__builtin_amdgcn_readlane(csi, 1)), s1 = __int_as_float(__builtin_amdgcn_readlane(sni, 1));
    const float c2 = __int_as_float(__builtin_amdgcn_readlane(csi, 2)), s2 = __int_as_float(__builtin_amdgcn_readlane(sni, 2));
    float T[16];
    const bool still = transform_from_sincos(x, c0, s0, c1, s1, c2, s2, dist_shake2, cos_shake, T);      // SDF.cpp:25-43 (only its verdict is used, :81-85)
    int code = STEP_APPLIED;
    if (!still) code = STEP_LOST_SHAKE;
    else {
      const float nx = sqrtf(x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3] + x[4] * x[4] + x[5] * x[5]);
      if (nx < 0.001f) code = STEP_CONVERGED;                                // SDF.cpp:87-90: stop before applying x
    }
    if (threadIdx.x == 0) {
      if (code == STEP_APPLIED) {
        float ncur[16];
        sdf_apply_increment_series(x, s_cur, ncur);
#pragma unroll
        for (int i = 0; i < 16; ++i) s_cur[i] = ncur[i];
      }
      *s_code = code;
    }
  }
  __syncthreads();
  return *s_code;
}
// icp_wg_reduce for any workgroup size T (a multiple of 64): 16-lane row totals by DPP, one LDS word per (sum, row), then 4 lanes per sum add a quarter of the
// T / 16 row totals each and two DPP shifts combine them (fixed order).  s_wave: 27 x (T / 16) floats.
template <int T>
__device__ __forceinline__ bool sdf_wg_reduce(float acc[27], float* s_wave, int& k, float& sw) {
  constexpr int ROWS = T / 16, PER = ROWS / 4;
  const int row = threadIdx.x >> 4;
#pragma unroll
  for (int i = 0; i < 27; ++i) acc[i] = kf_row_scan_sum(acc[i]);
  if ((threadIdx.x & 15) == 15) {
#pragma unroll
    for (int i = 0; i < 27; ++i) s_wave[i * ROWS + row] = acc[i];
  }
  __syncthreads();
  k = threadIdx.x >> 2; sw = 0.f;
  if (threadIdx.x < 27 * 4) {
    const int part = threadIdx.x & 3;
    sw = s_wave[k * ROWS + part * PER];
#pragma unroll
    for (int w = 1; w < PER; ++w) sw += s_wave[k * ROWS + part * PER + w];
    sw += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(sw), 0x111, 0xf, 0xf, true));   // row_shr:1
    sw += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(sw), 0x112, 0xf, 0xf, true));   // row_shr:2
    return part == 3;
  }
  return false;
}
#ifndef SDF_FOLD_PAIRS
#define SDF_FOLD_PAIRS false
#endif
template <typename AD>
__global__ void __launch_bounds__(SDF_THREADS) k_sdf_loop(SdfLoopArgs L) {
  __shared__ float s_m[7][16];
  __shared__ float s_wave[27 * (SDF_THREADS / 16)], s_tot[(SDF_THREADS / 32) * 32];
  __shared__ int s_abort, s_code;
  KfTrackState* st = L.track;
  // (the claim word and the commit word are requested together with the pose: one round trip)
  const unsigned commit_seen0 = __hip_atomic_load(&st->commit_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (__hip_atomic_load(&st->rescue_tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == L.tag_base) return;     // the launch was given to one workgroup before this one arrived
  if (L.play_dead && (int)blockIdx.x == L.n_loop - 1) return;
  const float w_h = 0.001f;                                               // CalSDFErrSolverParams.cu:119
  const float v_h = L.vol.size / (float)L.vol.res;                        // :120
  const int grid_l = L.n_loop;
  const int tiles_x = (L.cam.cols + 7) >> 3, tiles_y = (L.cam.rows + 7) >> 3;
  const KfRecip rS = kf_recip(L.vol.size);
  const float rcell = 1.0f / L.vol.cell;
  const AD S(L.vol);
  float* const s_cur = s_m[0];
  auto apply = [&]() { return sdf_apply_step_wave(s_tot, s_cur, L.th.dist_shake2, L.th.cos_shake, &s_code); };     // SDF.cpp:79-100
  int first = (int)blockIdx.x, stride = L.n_loop;                         // the workgroups of the dealing this one plays: its own -- or all of them, once it finishes alone
  bool solo = false;
  for (;;) {
    // SDF.cpp:56 cur_transform = _pose -- for the solo finish, too: the claim excludes every other committer, so st->pose is still the pose at kernel entry
    if (threadIdx.x < 16) s_cur[threadIdx.x] = st->pose[threadIdx.x];
    if (threadIdx.x == 0) s_abort = 0;
    __syncthreads();
    LoopOutcome o = {STEP_APPLIED, 0, grid_l, 0, false};
    for (int it = 0; it < L.max_iter; ++it) {                             // SDF.cpp:57
      sdf_perturbed_transforms(s_m, w_h);
      __syncthreads();
#pragma unroll 1
      for (int w = first; w < grid_l; w += stride) {
        float acc[27];
#pragma unroll
        for (int k = 0; k < 27; ++k) acc[k] = 0.f;
#pragma unroll 1
        for (int j = 0; j < L.px_l; ++j) {
          // a wave takes an 8x8 pixel TILE, not 64 pixels of a row: its 64 world points then fall into a few bricks' worth of cache lines (a scanline
          // of 64 pixels crosses ~30 voxel columns and, on a slanted surface, as many layers: ~22 lines per gather instruction, which is what
          // bounded the pixel phase -- profiles/r05_c3_*); tiles are dealt to the waves round robin like the ICP loop's 64-pixel chunks
          const int tile = ((int)(threadIdx.x >> 6) * grid_l + w) + j * ((SDF_THREADS / 64) * grid_l);
          const int tx = tile % tiles_x, ty = tile / tiles_x;
          const int x = tx * 8 + (int)(threadIdx.x & 7), y = ty * 8 + (int)((threadIdx.x >> 3) & 7);
          const bool in = ty < tiles_y && x < L.cam.cols && y < L.cam.rows;
          const int i = in ? y * L.cam.cols + x : 0;
          const float d = in ? L.depth[i] : 0.f;
          if (__ballot(d != 0.f) == 0ull) continue;                       // a wave without a single depth value
          sdf_accumulate_pixel<AD>(L.vol, S, s_m, L.cam, i, d, w_h, v_h, rS, rcell, L.slab_pixels != 0, acc);
        }
        int k; float sw;
        sdf_wg_reduce<SDF_THREADS>(acc, s_wave, k, sw);
        icp_publish_tagged(L.slots + (size_t)it * KF_ICP_LOOP_MAX_WG * 32, w, L.tag_base + (unsigned)it, sw);
        __syncthreads();                                                   // s_wave is reused by the next turn
      }
      fold_partials_tagged<SDF_FOLD_PAIRS>(L.slots + (size_t)it * KF_ICP_LOOP_MAX_WG * 32, grid_l, L.tag_base + (unsigned)it, s_tot, &s_abort, 0, solo ? nullptr : &st->rescue_tag, L.tag_base);
      o.fold = it;
      if (s_abort) { o.timed_out = true; break; }
      o.code = apply();
      if (o.code != STEP_APPLIED) break;
      ++o.applied;
    }
    if (track_loop_end<SDF_FOLD_PAIRS>(L, commit_seen0, solo, o, s_tot, &s_abort, s_cur, apply, s_m[1]) != LOOP_SOLO) return;
    solo = true; first = 0; stride = 1;
  }
}

// ---- loop control ---------------------------------------------------------------------------------------------------
// mode 0: frame 0 (no tracking, "tracked"); mode 1: start of a Gauss-Newton loop
__global__ void k_track_begin(KfTrackState* st, int mode) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  st->status = KF_TRACK_OK; st->iterations = 0; st->converged = 0; st->rescued = 0;
  if (mode == 0) { st->tracked = 1; return; }
  st->tracked = 0;
  for (int i = 0; i < 16; ++i) st->cur[0][i] = st->pose[i];                 // ICP.cpp:62
  kf_mat44_inverse(st->pose, st->last_inv);                                // ICP.cpp:63 last_transform_inv = _pose.getInverse()
}

// Last launch of a loop: fold + apply the final step (a.step = number of steps launched), then commit _pose (ICP.cpp:84,
// SDF.cpp:103).  With use_state == 0 it only leaves the 27 sums in track->reduced (per-call wrappers).
__global__ void __launch_bounds__(ICP_THREADS) k_track_finish(TrackArgs a) {
  __shared__ float s_cur[16], s_linv[16], s_tot[32 * 32];
  __shared__ int s_code;
  KfTrackState* st = a.track;
  if (!a.use_state || a.fold_out) {                                       // fold only: per-call wrappers, pixel-partitioned ICP
    fold_partials(a.partials + (size_t)((a.step + 1) & 1) * KF_ICP_MAX_WG * 32, a.n_prev_wg, s_tot);
    if (threadIdx.x < 32) {
      if (a.fold_out) a.fold_out[threadIdx.x] = threadIdx.x < 27 ? s_tot[threadIdx.x] : 0.f;
      else if (threadIdx.x < 27) st->reduced[threadIdx.x] = s_tot[threadIdx.x];
    }
    return;
  }
  if (!step_prologue(a, s_cur, s_linv, s_tot, &s_code)) return;            // lost or converged: already recorded
  if (threadIdx.x < 16) st->pose[threadIdx.x] = s_cur[threadIdx.x];
  if (threadIdx.x == 64) kf_mat44_inverse(s_cur, st->pose_inv);
  if (threadIdx.x == 0) st->tracked = 1;
}

// acos(ca) <= angle  <=>  ca >= cos(angle) for angle in [0, pi]; beyond pi every rotation passes, below 0 none does (NaN stays NaN: none)
static inline float shake_cos(float angle) { return angle >= 3.14159274f ? -2.f : (angle < 0.f ? 2.f : cosf(angle)); }
// norm > t  <=>  norm^2 > t^2 only for t >= 0; for a negative threshold the reference's comparison holds for every norm (every pixel
// is rejected, every increment counts as shaking): -1 keeps that, since a squared norm is never below zero
static inline float gate_square(float t) { return t < 0.f ? -1.f : t * t; }
// the thresholds of one tracking call, in every form the kernels use
static inline TrackThresholds track_thresholds(float dist_thres, float sin_thres, float dist_shake, float angle_shake) {
  TrackThresholds t;
  t.dist_thres = dist_thres; t.sin_thres = sin_thres; t.dist_shake = dist_shake; t.angle_shake = angle_shake;
  t.cos_shake = shake_cos(angle_shake); t.dist_shake2 = gate_square(dist_shake);
  t.dist_thres2 = gate_square(dist_thres); t.sin_thres2 = gate_square(sin_thres);
  return t;
}
// the camera of pyramid level l (ICP.cpp:36-48: every level halves the one above)
static inline KfCam level_cam(const kf_camera_params* cam0, int l) {
  kf_camera_params p = *cam0;
  for (int k = 0; k < l; ++k) { p.cols /= 2; p.rows /= 2; p.cx /= 2; p.cy /= 2; p.fx /= 2; p.fy /= 2; }
  return kf_to_cam(&p);
}
static int icp_iters(int levels, int iters[KF_MAX_LEVELS]) {                // ICP.cpp:14-35
  iters[0] = iters[1] = iters[2] = 0;
  if (levels == 1) iters[0] = 3; else if (levels == 2) { iters[0] = 10; iters[1] = 5; } else if (levels == 3) { iters[0] = 10; iters[1] = 5; iters[2] = 4; } else return 0;
  return iters[0] + iters[1] + iters[2];
}
static inline int track_grid(int npx) {           // SDF tracker: 256 lanes, grid-stride
  int g = kf_div_up(npx, TRK_THREADS * TRK_PX);
  return g < 1 ? 1 : (g > KF_ICP_MAX_WG ? KF_ICP_MAX_WG : g);
}
static inline int icp_grid(int npx) { return kf_div_up(npx, ICP_THREADS * ICP_PX); }   // ICP: every pixel exactly once

extern "C" int kf_set_pose(kf_ctx* c, const kf_mat44* pose) {
  if (!c || !pose) return KF_ERR_ARG;
  { const int ds = kf_tail_cull_discard(c); if (ds) return ds; }   // (a cull that ran for the tracked pose does not describe this one)
  memcpy(c->host_pinned, pose->m, 64);
  const int one = 1;
  memcpy((char*)c->host_pinned + 64, &one, sizeof(one));
  kf_mat44_inverse(pose->m, (float*)((char*)c->host_pinned + 128));          // same arithmetic as the device's commits
  KF_CHECK(hipMemcpyAsync(c->track->pose, c->host_pinned, 64, hipMemcpyHostToDevice, c->stream));
  KF_CHECK(hipMemcpyAsync(c->track->pose_inv, (char*)c->host_pinned + 128, 64, hipMemcpyHostToDevice, c->stream));
  // a pose supplied by the caller counts as a successful localisation: the device-predicated integrate (transform == NULL) fuses with it
  KF_CHECK(hipMemcpyAsync(&c->track->tracked, (char*)c->host_pinned + 64, sizeof(one), hipMemcpyHostToDevice, c->stream));
  KF_CHECK(hipStreamSynchronize(c->stream));     // the pinned staging words are reused
  return 0;
}

extern "C" int kf_cal_point_to_plane_solver_params(kf_ctx* c, uint32_t level, const kf_mat44* cur, const kf_mat44* last_inv,
                                                   const kf_camera_params* cam, float dist_thres, float sin_thres) {
  if (!c || !cur || !last_inv || !cam || level >= (uint32_t)c->levels) return KF_ERR_ARG;
  if ((int)cam->cols != c->lvl_cols[level] || (int)cam->rows != c->lvl_rows[level]) return KF_ERR_ARG;
  TrackArgs a; memset(&a, 0, sizeof(a));
  a.new_v = c->new_v[level]; a.new_n = c->new_n[level]; a.model_v = c->model_v[level]; a.model_n = c->model_n[level];
  a.cam = kf_to_cam(cam);
  for (int i = 0; i < 16; ++i) { a.cur_val.m[i] = cur->m[i]; a.linv_val.m[i] = last_inv->m[i]; }
  a.th = track_thresholds(dist_thres, sin_thres, 0.f, 0.f);
  a.partials = c->icp_partials; a.track = c->track;
  const int grid = icp_grid(a.cam.cols * a.cam.rows);
  if (grid > KF_ICP_MAX_WG) return KF_ERR_ARG;
  hipLaunchKernelGGL(k_icp_step, dim3(grid), dim3(ICP_THREADS), 0, c->stream, a);
  a.step = 1; a.n_prev_wg = grid;
  hipLaunchKernelGGL(k_track_finish, dim3(1), dim3(ICP_THREADS), 0, c->stream, a);
  return (int)hipGetLastError();
}

extern "C" int kf_cal_sdf_solver_params(kf_ctx* c, const kf_camera_params* cam, const kf_mat44* cur) {
  if (!c || !cam || !cur) return KF_ERR_ARG;
  if ((int)cam->cols != c->cols || (int)cam->rows != c->rows) return KF_ERR_ARG;
  TrackArgs a; memset(&a, 0, sizeof(a));
  a.cam = kf_to_cam(cam); a.vol = c->vol; a.depth = c->trunced_depth; a.sdf = 1;
  for (int i = 0; i < 16; ++i) a.cur_val.m[i] = cur->m[i];
  a.partials = c->icp_partials; a.track = c->track;
  const int grid = track_grid(c->cols * c->rows);
  launch_sdf_step(c, grid, a);
  a.step = 1; a.n_prev_wg = grid;
  hipLaunchKernelGGL(k_track_finish, dim3(1), dim3(ICP_THREADS), 0, c->stream, a);
  return (int)hipGetLastError();
}

extern "C" int kf_read_solver_params(kf_ctx* c, float out27[27]) {
  if (!c || !out27) return KF_ERR_ARG;
  KF_CHECK(hipMemcpyAsync(c->host_pinned, c->track->reduced, 27 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  KF_CHECK(hipStreamSynchronize(c->stream));
  memcpy(out27, c->host_pinned, 27 * sizeof(float));
  return 0;
}

// a persistent loop timed out and was finished by one workgroup alone (track_loop_end: the frame is kept, milliseconds late): back off to
// per-step launches for a while (64 frames, doubling up to 4096 on repeats; 1024 clean loop frames in a row forget the history).  One episode
// is noted once: launches of the loop that were already enqueued when the word was seen raise it again while the back-off is running.
static void kf_note_loop_stall(kf_ctx* c) {
  if (c->persistent_backoff > 0) return;
  c->persistent_backoff_len = c->persistent_backoff_len ? (c->persistent_backoff_len >= 2048 ? 4096 : c->persistent_backoff_len * 2) : 64;
  c->persistent_backoff = c->persistent_backoff_len;
  c->loop_clean_frames = 0;
}
// May this tracking call run a persistent loop (k_icp_loop, k_icp_loop_batched, k_sdf_loop)?  `fits`: the caller's own conditions.  A loop of an EARLIER frame
// that gave up waiting (its workgroups were not co-resident: a foreign process on the GPU) has set the pinned stall word by now -- no read-back of the verdict
// needed: the next frames take one launch per step (same bits for ICP, see k_icp_step); after `persistent_backoff_len` of them the loop is tried again, and
// every further stall doubles that wait.  The loop also needs this context alone on a device nobody else uses.  Admitted: this launch's tags and fault
// injection go into L.
static bool kf_loop_admit(kf_ctx* c, bool fits, TrackLoopArgs& L) {
  unsigned* stall_word = (unsigned*)((char*)c->host_pinned + KF_PINNED_STALL_WORD);
  if (__atomic_load_n(stall_word, __ATOMIC_RELAXED)) { __atomic_store_n(stall_word, 0u, __ATOMIC_RELAXED); kf_note_loop_stall(c); }
  else if (c->persistent_backoff == 0 && c->persistent_backoff_len && ++c->loop_clean_frames >= 1024) { c->persistent_backoff_len = 0; c->loop_clean_frames = 0; }
  if (!fits || c->loop_refused || kf_live_contexts(c->cfg.device) != 1 || kf_device_shared(c->cfg.device)) return false;
  if (c->persistent_backoff > 0) { --c->persistent_backoff; return false; }
  c->icp_loop_seq += 64u;                                    // tags of one launch never collide with an earlier launch's slots
  L.slots = c->icp_loop_slots; L.tag_base = c->icp_loop_seq; L.track = c->track; L.stall_word = stall_word;
  if (c->inject_stall > 0) { L.play_dead = 1; --c->inject_stall; }
  return true;
}

// The fusion pass's cull as the tail of a persistent tracking launch (k_icp_loop, k_sdf_loop): the previous kf_integrate_volume(transform == NULL) left its
// parameters behind, the tile tables describe THIS frame's depth map, no deferred-weight words (their cull retires bricks: side effects nobody could undo) and
// few enough macro cells for the launch's workgroups.  kf_integrate_volume consumes it, or undoes it when it is asked for something else.
static bool kf_arm_tail_cull(kf_ctx* c, const kf_camera_params* cam0, int n_wg, int waves, IntegrateArgs& out) {
  if (!(kf_switch(KF_SW_CULL_IN_TRACK) && c->cull_hint.valid && !kf_defer_enabled(c) &&
        c->tile_serial != 0 && c->tile_serial == c->trunc_serial && c->tile_built_dist == c->cull_hint.max_dist &&
        memcmp(&c->cull_hint.dcam, cam0, sizeof(*cam0)) == 0 && kf_cull_tail_fits(c, n_wg, waves))) return false;
  kf_fill_cull_args(c, out, &c->cull_hint.dcam, c->cull_hint.sdf_trunc, c->cull_hint.max_dist);
  c->tail_cull.armed = 1; c->tail_cull.parity = out.parity; c->tail_cull.bz0 = c->vol.bz0; c->tail_cull.bz1 = c->vol.bz1;
  c->tail_cull.sdf_trunc = c->cull_hint.sdf_trunc; c->tail_cull.max_dist = c->cull_hint.max_dist; c->tail_cull.dcam = c->cull_hint.dcam;
  c->tail_cull.trunc_serial = c->trunc_serial;
  return true;
}

extern "C" int kf_icp_track(kf_ctx* c, uint32_t frame_id, const kf_icp_params* icp, const kf_camera_params* cam0) {
  if (!c || !icp || !cam0) return KF_ERR_ARG;
  if ((int)icp->pyramid_levels != c->levels || (int)cam0->cols != c->cols || (int)cam0->rows != c->rows) return KF_ERR_ARG;
  c->last_track_form = 0;
  { const int ds = kf_tail_cull_discard(c); if (ds) return ds; }   // (a tail cull of the previous frame that no kf_integrate_volume consumed)
  if (frame_id == 0) {                                       // ICP.cpp:52-55
    hipLaunchKernelGGL(k_track_begin, dim3(1), dim3(64), 0, c->stream, c->track, 0);
    return (int)hipGetLastError();
  }
  int iters[KF_MAX_LEVELS];
  const int n_steps = icp_iters(c->levels, iters);
  int st;
  kf_evt_begin(c, KF_STAGE_TRACK);
  const int grid0 = icp_grid(c->cols * c->rows);
  const int persistent_env = kf_switch(KF_SW_ICP_PERSISTENT), coop_env = kf_switch(KF_SW_ICP_COOPERATIVE);
  if (c->loop_occupancy == 0) {                              // (asked once, whatever form this call takes: the per-step form folds in the batched loop's groups)
    // every workgroup must be resident at once (they wait for each other's tagged partial sums): ask the runtime how many 512-lane
    // workgroups of THESE kernels a CU holds (registers, LDS) instead of assuming one
    int per_cu = 0, per_cu_b = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_icp_loop, ICP_THREADS, 0) != hipSuccess || per_cu < 1) per_cu = -1;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_b, k_icp_loop_batched, ICP_THREADS, 0) != hipSuccess || per_cu_b < 1) per_cu_b = -1;
    c->loop_occupancy = per_cu; c->loop_occupancy_batched = per_cu_b;
  }
  // Images whose level 0 needs more workgroups than the chip holds at once (1280x960: 800): the batched loop -- as many resident workgroups as the
  // VGA loop uses (the CU count less a share for the riders), each playing several workgroups of the dealing in turn.  KF_ICP_BATCHED=0: per step.
  const bool beyond = c->loop_occupancy < 1 || (long long)grid0 > (long long)c->loop_occupancy * c->num_cus;
  const int room_env = kf_switch(KF_SW_ICP_BATCHED_ROOM);    // KF_ICP_BATCHED_ROOM=n: resident workgroups of the batched loop (A/B; every launch form folds in groups of n, so the forms stay bitwise equal)
  const int room = c->loop_occupancy_batched >= 1 ? ((room_env >= 16 && room_env <= c->num_cus * c->loop_occupancy_batched) ? room_env : c->num_cus - c->num_cus / 5) : 0;      // 256 CUs: 205 resident workgroups, 51 CUs left to the riders
  const bool batched = beyond && kf_switch(KF_SW_ICP_BATCHED) && !coop_env && room >= 16 && grid0 <= KF_ICP_LOOP_MAX_WG;
  // fold_group: the publishers of a batched launch.  Every launch form of such an image adds the partial sums of the workgroups g, g + fold_group, ... first
  // (the batched loop's resident workgroup g plays exactly those): the forms stay bitwise equal
  const int fold_group = batched ? room : 0;
  IcpLoopArgs L; memset(&L, 0, sizeof(L));
  const bool use_loop = kf_loop_admit(c, persistent_env && grid0 <= KF_ICP_LOOP_MAX_WG && n_steps <= KF_ICP_LOOP_STEPS && (!beyond || batched), L);
  // ICP.cpp:57-63: the four pyramids + the loop's set-up, one launch -- unless every pyramid describes its level 0 already (the raycast launch
  // left the model maps' behind, its riders the prefetched frame's: raycast.hip) AND the persistent loop runs, which reads nothing of that
  // set-up but the committed pose and writes its whole verdict itself: the steady-state frame then has no pyramid launch at all
  const bool pyramids_done = c->levels == 3 && c->new_pyr_ok && c->model_pyr_ok;
  if (!(use_loop && !coop_env && pyramids_done) && (st = kf_launch_pyramids_and_begin(c, 1))) return st;
  if (use_loop) {
    for (int l = 0; l < c->levels; ++l) {
      L.new_v[l] = c->new_v[l]; L.new_n[l] = c->new_n[l]; L.model_v[l] = c->model_v[l]; L.model_n[l] = c->model_n[l];
      L.cam[l] = level_cam(cam0, l); L.iters[l] = iters[l];
    }
    L.levels = c->levels;
    L.th = track_thresholds(icp->dist_thres, icp->norm_sin_thres, icp->dist_shake, icp->angle_shake);
    L.exp_mode = KF_EXP_ENV(ICP_EXP);
    L.n_loop = batched ? room : grid0; L.n_virtual = grid0;
    // a pending kf_prefetch_frame: the next frame's filter rides in this launch (see IcpLoopArgs) and leaves the gated + filtered image in
    // the alternate buffers; the raycast launch that follows carries its tile tables (the fusion pass in between clears them) and its
    // vertices / normals.  Not under a cooperative launch, whose whole grid would have to be resident.
    unsigned n_riders = 0;
    if (kf_switch(KF_SW_PREFETCH_IN_TRACK) && !coop_env && c->fp_pending && c->alt_raw && !c->fp_filtered) {
      bool fast;
      kf_bilateral_args(c, c->fp_src, nullptr, c->alt_raw, c->alt_trunced, c->alt_filtered, c->fp_params[0], c->fp_params[1], c->fp_params[2], c->fp_params[3],
                        false, &L.bil, &fast);
      L.bil_fast = fast ? 1 : 0;
      L.bil_gx = kf_div_up(c->cols, BIL_TX); L.bil_tiles = L.bil_gx * kf_div_up(c->rows, BIL_TY);
      n_riders = (unsigned)((L.bil_tiles + 1) / 2);
      c->fp_filtered = 1;
    }
    if (!batched && !coop_env && L.exp_mode == 0 && kf_arm_tail_cull(c, cam0, grid0, ICP_THREADS / 64, L.cull)) L.cull_on = 1;
    if (coop_env) {
      // a cooperative launch: the runtime itself checks that the whole grid can be resident and refuses otherwise
      void* params[] = {(void*)&L};
      const hipError_t e = hipLaunchCooperativeKernel((const void*)k_icp_loop, dim3(grid0), dim3(ICP_THREADS), params, 0, c->stream);
      if (e == hipSuccess) { c->last_track_form = 1; kf_evt_end(c, KF_STAGE_TRACK); return 0; }
      (void)hipGetLastError();                               // refused: this device / configuration cannot hold the loop -- per-step from now on
      c->loop_refused = 1;
    } else {
      if (batched) hipLaunchKernelGGL(k_icp_loop_batched, dim3((unsigned)L.n_loop + n_riders), dim3(ICP_THREADS), 0, c->stream, L);
      else hipLaunchKernelGGL(k_icp_loop, dim3((unsigned)grid0 + n_riders), dim3(ICP_THREADS), 0, c->stream, L);
      c->last_track_form = 1;
      kf_evt_end(c, KF_STAGE_TRACK);
      return (int)hipGetLastError();
    }
  }
  // one launch per Gauss-Newton step: the same pixel dealing, the same reduction and fold orders as the loop -> the same pose bits
  TrackArgs a; memset(&a, 0, sizeof(a));
  a.use_state = 1;
  a.th = track_thresholds(icp->dist_thres, icp->norm_sin_thres, icp->dist_shake, icp->angle_shake);
  a.partials = c->icp_partials; a.track = c->track;
  a.fold_group = fold_group;
  int step = 0, prev_grid = 0;
  for (int l = c->levels - 1; l >= 0; --l)                   // coarse -> fine, ICP.cpp:65
    for (int it = 0; it < iters[l]; ++it) {
      a.new_v = c->new_v[l]; a.new_n = c->new_n[l]; a.model_v = c->model_v[l]; a.model_n = c->model_n[l];
      a.cam = level_cam(cam0, l);
      a.step = step; a.consume = step > 0; a.n_prev_wg = prev_grid;
      icp_level_geometry(a.cam.cols * a.cam.rows, grid0, l, a.px_l, a.deal_grid);
      const int grid = a.deal_grid;
      if (grid > KF_ICP_MAX_WG) return KF_ERR_ARG;
      hipLaunchKernelGGL(k_icp_step, dim3(grid), dim3(ICP_THREADS), 0, c->stream, a);
      prev_grid = grid; ++step;
    }
  a.step = step; a.consume = 1; a.n_prev_wg = prev_grid;
  hipLaunchKernelGGL(k_track_finish, dim3(1), dim3(ICP_THREADS), 0, c->stream, a);
  c->last_track_form = 2;
  kf_evt_end(c, KF_STAGE_TRACK);
  return (int)hipGetLastError();
}

// ---- pixel-partitioned ICP for z-slab / multi-GPU runs (all-reduce of the 27-float system) -------------
// The caller owns a 32-float device buffer `dev_sums`.  Per Gauss-Newton step: kf_icp_partition_step sums this rank's pixel
// range and leaves the 27 sums in dev_sums; the caller all-reduces dev_sums (SUM) over the ranks; the next step (or
// kf_icp_partition_finish) consumes it.  Every rank applies the identical all-reduced system, so the poses agree bitwise.
extern "C" int kf_icp_partition_begin(kf_ctx* c, uint32_t frame_id) {
  if (!c) return KF_ERR_ARG;
  { const int ds = kf_tail_cull_discard(c); if (ds) return ds; }
  if (frame_id != 0) kf_evt_begin(c, KF_STAGE_TRACK);       // (the stage timer runs from here to kf_icp_partition_finish: it includes the caller's all-reduces)
  return kf_launch_pyramids_and_begin(c, frame_id == 0 ? 0 : 1);
}
extern "C" int kf_icp_partition_steps(kf_ctx* c) { int it[KF_MAX_LEVELS]; return c ? icp_iters(c->levels, it) : 0; }
extern "C" int kf_icp_partition_step(kf_ctx* c, uint32_t step, const kf_icp_params* icp, const kf_camera_params* cam0,
                                     uint32_t part, uint32_t parts, float* dev_sums) {
  if (!c || !icp || !cam0 || !dev_sums || parts == 0 || part >= parts) return KF_ERR_ARG;
  int iters[KF_MAX_LEVELS];
  const int total = icp_iters(c->levels, iters);
  if ((int)step >= total) return KF_ERR_ARG;
  int l = c->levels - 1, s = (int)step;                                     // coarse -> fine
  while (s >= iters[l]) { s -= iters[l]; --l; }
  TrackArgs a; memset(&a, 0, sizeof(a));
  a.use_state = 1;
  a.new_v = c->new_v[l]; a.new_n = c->new_n[l]; a.model_v = c->model_v[l]; a.model_n = c->model_n[l];
  a.cam = level_cam(cam0, l);
  a.th = track_thresholds(icp->dist_thres, icp->norm_sin_thres, icp->dist_shake, icp->angle_shake);
  a.partials = c->icp_partials; a.track = c->track;
  a.step = (int)step; a.consume = step > 0; a.ext_prev = step > 0 ? dev_sums : nullptr;
  const int rows_per = kf_div_up(a.cam.rows, (int)parts);                    // whole image rows per rank
  const int y0 = (int)part * rows_per, y1 = (y0 + rows_per < a.cam.rows) ? y0 + rows_per : a.cam.rows;
  a.px_begin = y0 * a.cam.cols; a.px_end = (y1 > y0 ? y1 : y0) * a.cam.cols;
  const int grid = (a.px_end > a.px_begin) ? icp_grid(a.px_end - a.px_begin) : 1;
  if (grid > KF_ICP_MAX_WG) return KF_ERR_ARG;
  if (a.px_end <= a.px_begin) { a.px_begin = 1; a.px_end = 1; }              // empty range: the kernel's bound check skips every pixel
  hipLaunchKernelGGL(k_icp_step, dim3(grid), dim3(ICP_THREADS), 0, c->stream, a);
  TrackArgs f = a; f.step = (int)step + 1; f.n_prev_wg = grid; f.fold_out = dev_sums; f.ext_prev = nullptr;
  hipLaunchKernelGGL(k_track_finish, dim3(1), dim3(ICP_THREADS), 0, c->stream, f);
  return (int)hipGetLastError();
}
extern "C" int kf_icp_partition_finish(kf_ctx* c, const kf_icp_params* icp, const float* dev_sums) {
  if (!c || !icp || !dev_sums) return KF_ERR_ARG;
  int iters[KF_MAX_LEVELS];
  TrackArgs a; memset(&a, 0, sizeof(a));
  a.use_state = 1; a.consume = 1; a.step = icp_iters(c->levels, iters); a.ext_prev = dev_sums;
  a.th = track_thresholds(icp->dist_thres, icp->norm_sin_thres, icp->dist_shake, icp->angle_shake); a.partials = c->icp_partials; a.track = c->track;
  hipLaunchKernelGGL(k_track_finish, dim3(1), dim3(ICP_THREADS), 0, c->stream, a);
  kf_evt_end(c, KF_STAGE_TRACK);
  return (int)hipGetLastError();
}

#ifdef KF_EXPERIMENTS
extern "C" int kf_exp_read_icp_slots(kf_ctx* c, unsigned long long* dst, size_t first, size_t n) {
  KF_CHECK(hipMemcpyAsync(dst, c->icp_loop_slots + first, n * 8, hipMemcpyDeviceToHost, c->stream));
  KF_CHECK(hipStreamSynchronize(c->stream));
  return 0;
}
#endif

extern "C" int kf_sdf_track(kf_ctx* c, uint32_t frame_id, const kf_sdf_tracker_params* sp, const kf_camera_params* cam) {
  if (!c || !sp || !cam) return KF_ERR_ARG;
  if ((int)cam->cols != c->cols || (int)cam->rows != c->rows) return KF_ERR_ARG;
  c->last_track_form = 0;
  { const int ds = kf_tail_cull_discard(c); if (ds) return ds; }
  if (frame_id == 0) {                                       // SDF.cpp:46-49
    hipLaunchKernelGGL(k_track_begin, dim3(1), dim3(64), 0, c->stream, c->track, 0);
    return (int)hipGetLastError();
  }
  kf_evt_begin(c, KF_STAGE_TRACK);
  // The whole loop in one launch (k_sdf_loop) under the conditions of the persistent ICP loop: this context alone on the device, no back-off after a
  // time-out, every workgroup resident.  KF_SDF_PERSISTENT=0 (or KF_ICP_PERSISTENT=0): one launch per iteration, as the z-slab partition runs it.
  {
    const bool buf = sdf_buffer_addressing(c->vol);
    const bool fits = kf_switch(KF_SW_SDF_PERSISTENT) && kf_switch(KF_SW_ICP_PERSISTENT) && sp->max_iter_nums >= 1 && sp->max_iter_nums <= KF_ICP_LOOP_STEPS;
    if (fits && c->sdf_loop_occupancy == 0) {
      int per_cu = 0;
      const hipError_t e = buf ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_sdf_loop<SdfBufAddr>, SDF_THREADS, 0)
                               : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_sdf_loop<SdfFlatAddr>, SDF_THREADS, 0);
      c->sdf_loop_occupancy = (e == hipSuccess && per_cu >= 1) ? per_cu : -1;
    }
    SdfLoopArgs L; memset(&L, 0, sizeof(L));
    if (kf_loop_admit(c, fits && c->sdf_loop_occupancy >= 1, L)) {
      const int npx = c->cols * c->rows;
      int n_loop = kf_switch(KF_SW_SDF_LOOP_WG) > 0 ? kf_switch(KF_SW_SDF_LOOP_WG) : c->num_cus;                           // one workgroup per CU
      n_loop = n_loop > c->num_cus * c->sdf_loop_occupancy ? c->num_cus * c->sdf_loop_occupancy : n_loop;
      n_loop = n_loop > KF_ICP_LOOP_MAX_WG ? KF_ICP_LOOP_MAX_WG : n_loop;
      const int need = kf_div_up(kf_div_up(c->cols, 8) * kf_div_up(c->rows, 8), SDF_THREADS / 64);
      if (n_loop > need) n_loop = need;
      L.vol = c->vol; L.depth = c->trunced_depth; L.cam = kf_to_cam(cam); L.max_iter = (int)sp->max_iter_nums;
      L.th = track_thresholds(0.f, 0.f, sp->dist_shake, sp->angle_shake);
      const int n_tiles = kf_div_up(c->cols, 8) * kf_div_up(c->rows, 8);      // 8x8 pixel tiles, one per wave and round
      L.n_loop = n_loop; L.px_l = kf_div_up(n_tiles, (SDF_THREADS / 64) * n_loop);
      if (kf_arm_tail_cull(c, cam, n_loop, SDF_THREADS / 64, L.cull)) L.cull_on = 1;
      if (buf) hipLaunchKernelGGL(k_sdf_loop<SdfBufAddr>, dim3((unsigned)n_loop), dim3(SDF_THREADS), 0, c->stream, L);
      else hipLaunchKernelGGL(k_sdf_loop<SdfFlatAddr>, dim3((unsigned)n_loop), dim3(SDF_THREADS), 0, c->stream, L);
      c->last_track_form = 1;
      kf_evt_end(c, KF_STAGE_TRACK);
      return (int)hipGetLastError();
    }
  }
  hipLaunchKernelGGL(k_track_begin, dim3(1), dim3(64), 0, c->stream, c->track, 1);
  TrackArgs a; memset(&a, 0, sizeof(a));
  a.use_state = 1; a.sdf = 1;
  a.cam = kf_to_cam(cam); a.vol = c->vol; a.depth = c->trunced_depth;
  a.th = track_thresholds(0.f, 0.f, sp->dist_shake, sp->angle_shake);
  a.partials = c->icp_partials; a.track = c->track;
  const int grid = track_grid(c->cols * c->rows);
  int step = 0;
  for (uint32_t it = 0; it < sp->max_iter_nums; ++it) {
    a.step = step; a.consume = step > 0; a.n_prev_wg = grid;
    launch_sdf_step(c, grid, a);
    ++step;
  }
  a.step = step; a.consume = step > 0; a.n_prev_wg = grid;
  hipLaunchKernelGGL(k_track_finish, dim3(1), dim3(ICP_THREADS), 0, c->stream, a);
  c->last_track_form = 2;
  kf_evt_end(c, KF_STAGE_TRACK);
  return (int)hipGetLastError();
}

// ---- SDF tracker on z-slabs (pixel -> owning slab by pworld0.z, all-reduce of the 27-float system) -----------
// Same protocol as the pixel-partitioned ICP above: the caller owns a 32-float device buffer `dev_sums`; per Gauss-Newton iteration
// kf_sdf_partition_step sums the pixels whose world point falls into the layers this context owns and leaves the 27 sums there, the
// caller all-reduces it (SUM) over the ranks, the next step (or kf_sdf_partition_finish) applies the reduced system.  Every rank
// applies identical numbers -> identical poses.  All `max_iter_nums` steps are always issued (launches after convergence return at
// once), so every rank makes the same collective calls.
extern "C" int kf_sdf_partition_begin(kf_ctx* c, uint32_t frame_id) {
  if (!c) return KF_ERR_ARG;
  { const int ds = kf_tail_cull_discard(c); if (ds) return ds; }
  c->last_track_form = 0;
  if (frame_id != 0) kf_evt_begin(c, KF_STAGE_TRACK);       // (ends in kf_sdf_partition_finish: the caller's all-reduces are inside)
  hipLaunchKernelGGL(k_track_begin, dim3(1), dim3(64), 0, c->stream, c->track, frame_id == 0 ? 0 : 1);
  return (int)hipGetLastError();
}
static int sdf_partition_args(kf_ctx* c, const kf_sdf_tracker_params* sp, const kf_camera_params* cam, TrackArgs& a) {
  if ((int)cam->cols != c->cols || (int)cam->rows != c->rows) return KF_ERR_ARG;
  // the perturbed lookups (rotations by 0.001 rad about the origin of a volume-sized lever, +- one cell) and their trilinear taps must
  // stay inside the stored layers: refuse a halo thinner than that, as kf_raycast_volume_slab does for its own reach
  const int need = (int)ceilf(0.001f * 1.7320508f * c->vol.size / c->vol.cell) + 3;
  const int lo = c->vol.own_z0 - c->vol.bz0 * KF_BRICK, hi = c->vol.bz1 * KF_BRICK - c->vol.own_z1;
  if ((c->vol.own_z0 > 0 && lo < need) || (c->vol.own_z1 < c->vol.res && hi < need)) return KF_ERR_ARG;
  memset(&a, 0, sizeof(a));
  a.use_state = 1; a.sdf = 1; a.slab_pixels = 1;
  a.cam = kf_to_cam(cam); a.vol = c->vol; a.depth = c->trunced_depth;
  a.th = track_thresholds(0.f, 0.f, sp->dist_shake, sp->angle_shake);
  a.partials = c->icp_partials; a.track = c->track;
  return 0;
}
extern "C" int kf_sdf_partition_step(kf_ctx* c, uint32_t step, const kf_sdf_tracker_params* sp, const kf_camera_params* cam, float* dev_sums) {
  if (!c || !sp || !cam || !dev_sums || step >= sp->max_iter_nums) return KF_ERR_ARG;
  TrackArgs a;
  int st = sdf_partition_args(c, sp, cam, a);
  if (st) return st;
  const int grid = track_grid(c->cols * c->rows);
  a.step = (int)step; a.consume = step > 0; a.n_prev_wg = grid; a.ext_prev = step > 0 ? dev_sums : nullptr;
  launch_sdf_step(c, grid, a);
  TrackArgs f = a; f.step = (int)step + 1; f.n_prev_wg = grid; f.fold_out = dev_sums; f.ext_prev = nullptr;
  hipLaunchKernelGGL(k_track_finish, dim3(1), dim3(ICP_THREADS), 0, c->stream, f);
  return (int)hipGetLastError();
}
extern "C" int kf_sdf_partition_finish(kf_ctx* c, const kf_sdf_tracker_params* sp, const kf_camera_params* cam, const float* dev_sums) {
  if (!c || !sp || !cam || !dev_sums) return KF_ERR_ARG;
  TrackArgs a;
  int st = sdf_partition_args(c, sp, cam, a);
  if (st) return st;
  a.consume = sp->max_iter_nums > 0; a.step = (int)sp->max_iter_nums; a.ext_prev = dev_sums;
  hipLaunchKernelGGL(k_track_finish, dim3(1), dim3(ICP_THREADS), 0, c->stream, a);
  kf_evt_end(c, KF_STAGE_TRACK);
  return (int)hipGetLastError();
}

// The blocking read-back split in two, so that a caller can put more work behind the tracker before it waits for the verdict:
// kf_request_track_result enqueues the copy of the tracking state (into pinned memory) right where the stream stands and marks
// the spot with an event; kf_wait_track_result blocks on THAT event only -- whatever was enqueued after the request keeps running.
extern "C" int kf_request_track_result(kf_ctx* c) {
  if (!c) return KF_ERR_ARG;
  if (!c->ev_track) KF_CHECK(hipEventCreateWithFlags(&c->ev_track, hipEventDisableTiming));
  KF_CHECK(hipMemcpyAsync((char*)c->host_pinned + 1024, c->track, sizeof(KfTrackState), hipMemcpyDeviceToHost, c->stream));
  KF_CHECK(hipEventRecord(c->ev_track, c->stream));
  c->track_requested = 1;
  return 0;
}
extern "C" int kf_wait_track_result(kf_ctx* c, kf_track_result* out) {
  if (!c || !out) return KF_ERR_ARG;
  if (!c->track_requested) return KF_ERR_STATE;
  KF_CHECK(hipEventSynchronize(c->ev_track));
  c->track_requested = 0;
  const KfTrackState* h = (const KfTrackState*)((const char*)c->host_pinned + 1024);
  memcpy(out->pose.m, h->pose, 64);
  out->tracked = h->tracked; out->status = h->status; out->iterations = h->iterations; out->launch_form = (h->rescued && c->last_track_form == 1) ? 3 : c->last_track_form;
  if (h->rescued && c->last_track_form == 1) kf_note_loop_stall(c);
  return 0;
}

extern "C" int kf_read_track_result(kf_ctx* c, kf_track_result* out) {
  if (!c || !out) return KF_ERR_ARG;
  KfTrackState* h = (KfTrackState*)c->host_pinned;
  KF_CHECK(hipMemcpyAsync(h, c->track, sizeof(KfTrackState), hipMemcpyDeviceToHost, c->stream));
  KF_CHECK(hipStreamSynchronize(c->stream));
  memcpy(out->pose.m, h->pose, 64);
  // launch_form 3: the persistent loop timed out waiting for a partial sum -- some of its workgroups were not resident (another process on
  // the GPU?) -- and one workgroup finished the frame alone (same bits, milliseconds late).  The next frames track with one launch per
  // step, then the loop is tried again.
  out->tracked = h->tracked; out->status = h->status; out->iterations = h->iterations; out->launch_form = (h->rescued && c->last_track_form == 1) ? 3 : c->last_track_form;
  if (h->rescued && c->last_track_form == 1) kf_note_loop_stall(c);
  return 0;
}

// Fault injection for tests and rehearsals: in each of the next `launches` launches of the persistent ICP loop one workgroup exits at once, as
// if a foreign process had kept it off the chip -- the others time out (20 ms) and one of them finishes the frame alone.  Results are unchanged.
extern "C" int kf_inject_track_stall(kf_ctx* c, int launches) {
  if (!c || launches < 0) return KF_ERR_ARG;
  c->inject_stall = launches;
  return 0;
}
