// reloc_search.hpp -- the host side of relocalising a frame in the map (HybKinectfu::relocalise above kf_map_score_poses / kf_map_refine_poses; no reference
// counterpart): which points of a vertex map are scored, which candidate poses make up the lattice around a guess, and how scores are ranked.  Plain host
// C++, fp64, no device: the library (host_capi.cpp: hkf_reloc_points, hkf_reloc_lattice, hkf_reloc_rank) and the stand-alone test program
// (tests/map_reloc_main.cpp) both include it.  The search is a lattice around a guess: its reach is the lattice's extent and nothing more.
#pragma once
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "../../include/hybkf.h"
#include "../csrc/align_step.h"

#define HKF_RELOC_MAX_CANDIDATES (1u << 20)

// what HybKinectfu::relocalise takes.  A value of 0 for trans_step, rot_step, top, max_points, a negative level: the default (see hybkf_host.hpp).
struct RelocParams {
  int32_t has_guess;            // guess holds the centre pose (camera -> WORLD metres, row-major 4x4); otherwise the current pose is the centre
  float guess[16];
  float trans_step, rot_step;   // metres, radians
  int32_t n[6];                 // the lattice's half widths: three translation axes, three rotation axes (a negative one: the default, 2)
  uint32_t top, max_points;
  int32_t level;                // pyramid level of the vertex map
  uint32_t min_obs;             // a pose is eligible with at least this many observed points
  float band, gate;             // kf_map_score_poses' band, kf_map_refine_poses' gate
  float accept_inliers;         // accepted with n_in >= accept_inliers * points
  uint32_t max_iter, min_pairs;
  double eps_rot, eps_trans;
};
struct RelocReport {
  uint32_t candidates, points;
  uint32_t best_index, verdict, iterations;
  int32_t accepted;
  kf_pose_score best_score, refined_score;
  double best_pose[12], refined_pose[12];   // [R | t], camera -> world voxels
  float median_depth, trans_step, rot_step; // metres, metres, radians: the steps used
};
static inline RelocParams hkf_reloc_defaults() {
  RelocParams p = {};
  for (int k = 0; k < 6; ++k) p.n[k] = 2;
  p.top = 16; p.max_points = 4096; p.level = -1; p.min_obs = 64; p.band = 0.5f; p.gate = 1.f; p.accept_inliers = 0.5f;
  p.max_iter = 25; p.min_pairs = 64; p.eps_rot = 2.5e-4; p.eps_trans = 1e-3;
  return p;
}

// The points of a vertex map (n_pix float4 in metres, as kf_download_map(KF_MAP_NEW_VERTICES, L) gives it): a vertex with z == 0 is no measurement; the valid
// ones in row-major order; with more than max_points of them, those with the indices floor(i * count / max_points), i = 0 .. max_points - 1; each coordinate
// written as (float)((double)x / (double)cell).  Returns the number written (0 for a NULL pointer, cell not > 0 or max_points 0); *median_depth_m (may be
// NULL): element count / 2 of the valid z values in ascending order, metres (0 without a valid vertex).
static inline uint32_t reloc_points(const float* verts, uint32_t n_pix, float cell, uint32_t max_points, float* out, float* median_depth_m) {
  if (median_depth_m) *median_depth_m = 0.f;
  if (!verts || !out || !(cell > 0.f) || max_points == 0u) return 0u;
  std::vector<uint32_t> valid;
  std::vector<float> z;
  for (uint32_t i = 0; i < n_pix; ++i)
    if (verts[4 * (size_t)i + 2] != 0.f) { valid.push_back(i); z.push_back(verts[4 * (size_t)i + 2]); }
  const uint64_t count = valid.size();
  if (count == 0) return 0u;
  std::sort(z.begin(), z.end());
  if (median_depth_m) *median_depth_m = z[count / 2];
  const uint64_t take = count > max_points ? max_points : count;
  for (uint64_t i = 0; i < take; ++i) {
    const uint32_t src = valid[count > max_points ? (size_t)(i * count / max_points) : (size_t)i];
    for (int k = 0; k < 3; ++k) out[3 * i + k] = (float)((double)verts[4 * (size_t)src + k] / (double)cell);
  }
  return (uint32_t)take;
}

// the number of candidates of a lattice with half widths n[6]: prod (2 n + 1); -1 for a negative n or more than 2^20
static inline int64_t reloc_lattice_count(const int32_t n[6]) {
  int64_t k = 1;
  for (int a = 0; a < 6; ++a) {
    if (n[a] < 0 || n[a] > 1024) return -1;
    k *= 2 * (int64_t)n[a] + 1;
    if (k > (int64_t)HKF_RELOC_MAX_CANDIDATES) return -1;
  }
  return k;
}

// The candidate poses around a centre pose [Rc | tc] (row-major 3x4, camera -> world voxels): R = Rc * exp(omega^), omega = (ja, jb, jc) * rot_step -- the
// camera turns about its own centre --, t = tc + (ia, ib, ic) * trans_step along the world's axes; every index over [-n, n] of its axis, the zero offset
// included.  Order: translation outermost -- ia slowest, then ib, ic, ja, jb, and jc fastest.  Writes the first `cap` poses (12 doubles each; out may be NULL
// with cap 0) and returns their number K = prod (2 n + 1), or -1: a NULL centre or n, a negative n, K above 2^20.
static inline int64_t reloc_lattice(const double* centre, const int32_t n[6], double trans_step, double rot_step, double* out, int64_t cap) {
  if (!centre || !n) return -1;
  const int64_t K = reloc_lattice_count(n);
  if (K < 0) return -1;
  if (!out || cap <= 0) return K;
  int64_t k = 0;
  for (int ia = -n[0]; ia <= n[0]; ++ia)
    for (int ib = -n[1]; ib <= n[1]; ++ib)
      for (int ic = -n[2]; ic <= n[2]; ++ic)
        for (int ja = -n[3]; ja <= n[3]; ++ja)
          for (int jb = -n[4]; jb <= n[4]; ++jb)
            for (int jc = -n[5]; jc <= n[5]; ++jc, ++k) {
              if (k >= cap) return K;
              const double xi[6] = {ja * rot_step, jb * rot_step, jc * rot_step, 0.0, 0.0, 0.0};
              double E[9], u[3];
              kf_align_exp(xi, E, u);
              double* P = out + 12 * k;
              for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) P[4 * i + j] = centre[4 * i] * E[j] + centre[4 * i + 1] * E[3 + j] + centre[4 * i + 2] * E[6 + j];
              P[3] = centre[3] + ia * trans_step; P[7] = centre[7] + ib * trans_step; P[11] = centre[11] + ic * trans_step;
            }
  return K;
}

// Ranking: a pose is eligible with n_obs >= min_obs; the key is the signed integer 2 * n_in - n_obs -- inliers minus contradictions --, larger first; ties go
// to the smaller sum_q, then to the smaller index.  Writes the best min(M, eligible) indices to best (may be NULL with M 0) and returns how many were eligible.
static inline uint32_t reloc_rank(const kf_pose_score* scores, uint32_t n, uint32_t min_obs, uint32_t M, uint32_t* best) {
  if (!scores) return 0u;
  std::vector<uint32_t> idx;
  for (uint32_t i = 0; i < n; ++i) if (scores[i].n_obs >= min_obs) idx.push_back(i);
  const uint32_t eligible = (uint32_t)idx.size();
  if (!best || M == 0u) return eligible;
  const uint32_t take = eligible < M ? eligible : M;
  std::partial_sort(idx.begin(), idx.begin() + take, idx.end(), [&](uint32_t a, uint32_t b) {
    const int64_t ka = 2 * (int64_t)scores[a].n_in - (int64_t)scores[a].n_obs, kb = 2 * (int64_t)scores[b].n_in - (int64_t)scores[b].n_obs;
    if (ka != kb) return ka > kb;
    if (scores[a].sum_q != scores[b].sum_q) return scores[a].sum_q < scores[b].sum_q;
    return a < b;
  });
  for (uint32_t i = 0; i < take; ++i) best[i] = idx[i];
  return eligible;
}
