// relocal.hip -- relocalising a depth frame in the map: the two kernels that make a search over camera poses affordable.  kf_map_score_poses scores many
// candidate poses of one point set against the map in integers (how many points are observed, lie in the band, behind a surface, in free space);
// kf_map_pose_sums forms the Gauss-Newton sums of a few poses in one launch, and kf_map_refine_poses drives kf_align_brick_store's loop over them, per pose.
// No reference counterpart (the reference blocks on a key press when the camera is lost).  The map is map_lookup.h's, the sample map_sample.h's
// (kf_map_sample's bits), a row's way into the sums and the workgroup's fold align_rows.h's, the step and the loop's turn align_step.h's.  The contract is
// written out above kf_map_score_poses in include/hybkf.h, the argument in DESIGN.md 4e-10.
#include "kf_internal.h"
#include "brick_key.h"
#include "brick_find.h"
#include "resample_shared.h"
#include "map_lookup.h"
#include "map_sample.h"
#include "align_rows.h"
#include <string.h>
#include <new>
#include <vector>

#define KF_SCORE_MAX_POINTS (1u << 24)
#define KF_SCORE_MAX_POSES (1u << 20)
#define KF_SCORE_TARGET_GROUPS 2048u   // 256 compute units x 8 workgroups: what a small pose count is spread over
#define KF_SUMS_MAX_POSES 4096u
#define KF_SUMS_MAX_GROUPS 64u         // G = min(ceil(n_points / 256), this): a fixed function of the point count, so the fold order is too

// the position of camera point (x, y, z) under pose P = [R | t], per axis ((R0 x + R1 y) + R2 z) + t in fp64, one rounding per operation
__device__ __forceinline__ void pose_point(const double* __restrict__ P, float x, float y, float z, double& w0, double& w1, double& w2) {
  const double dx = (double)x, dy = (double)y, dz = (double)z;
  w0 = ((P[0] * dx + P[1] * dy) + P[2] * dz) + P[3];
  w1 = ((P[4] * dx + P[5] * dy) + P[6] * dz) + P[7];
  w2 = ((P[8] * dx + P[9] * dy) + P[10] * dz) + P[11];
}

// One workgroup: one pose, the points chunk * 256 + lane, + n_chunks * 256, ...: lanes next to each other take points next to each other (neighbouring
// pixels: their corners fall into the same few bricks), and every lane keeps its brick across its points.  The pose is the same for the whole workgroup: its
// 12 doubles are scalar loads.  Five integer counts per lane, folded by integer shuffles in the wave, through LDS across the four waves, and added to the
// pose's score by one integer atomic per field: integer addition commutes, so the bytes do not depend on the grid, the chunking or who arrives first.
__global__ void __launch_bounds__(256) k_score_poses(MapRef m, unsigned n_points, const float* __restrict__ pts, unsigned n_chunks, const double* __restrict__ poses,
                                                     float band, kf_pose_score* __restrict__ scores) {
  __shared__ unsigned s_cnt[4][4];
  __shared__ unsigned long long s_q[4];
  const unsigned pose = blockIdx.x / n_chunks, chunk = blockIdx.x - pose * n_chunks;
  const double* __restrict__ P = poses + (size_t)pose * 12u;
  MapBrick b = map_brick_none();
  unsigned n_obs = 0u, n_in = 0u, n_behind = 0u, n_free = 0u;
  unsigned long long sum_q = 0ull;
  for (size_t i = (size_t)chunk * 256u + threadIdx.x; i < n_points; i += (size_t)n_chunks * 256u) {
    double w0, w1, w2;
    pose_point(P, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], w0, w1, w2);
    QuerySample s;
    if (!query_sample<false, false>(m, w0, w1, w2, b, s)) continue;
    const float a = fabsf(s.tsdf);
    const bool in = a < band, behind = !in && s.tsdf < 0.f;
    n_obs += 1u;
    n_in += in ? 1u : 0u;
    n_behind += behind ? 1u : 0u;
    n_free += (!in && !behind) ? 1u : 0u;
    sum_q += (unsigned long long)(unsigned)(fminf(a, 1.f) * 65536.f);      // (the product is exact, the conversion truncates: at most 65536)
  }
  unsigned q_lo = (unsigned)sum_q, q_hi = (unsigned)(sum_q >> 32);
#pragma unroll
  for (int k = 32; k >= 1; k >>= 1) {
    n_obs += (unsigned)__shfl_xor((int)n_obs, k);
    n_in += (unsigned)__shfl_xor((int)n_in, k);
    n_behind += (unsigned)__shfl_xor((int)n_behind, k);
    n_free += (unsigned)__shfl_xor((int)n_free, k);
    const unsigned long long o = ((unsigned long long)(unsigned)__shfl_xor((int)q_hi, k) << 32) | (unsigned)__shfl_xor((int)q_lo, k);
    sum_q += o;
    q_lo = (unsigned)sum_q; q_hi = (unsigned)(sum_q >> 32);
  }
  const unsigned wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0u) {
    s_cnt[wave][0] = n_obs; s_cnt[wave][1] = n_in; s_cnt[wave][2] = n_behind; s_cnt[wave][3] = n_free;
    s_q[wave] = sum_q;
  }
  __syncthreads();
  kf_pose_score* out = scores + pose;
  if (threadIdx.x < 4u) {
    const unsigned v = (s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x]) + (s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x]);
    if (v) atomicAdd(&out->n_obs + threadIdx.x, v);                        // (n_obs, n_in, n_behind, n_free: four words in a row)
  } else if (threadIdx.x == 4u) {
    const unsigned long long v = (s_q[0] + s_q[1]) + (s_q[2] + s_q[3]);
    if (v) atomicAdd(reinterpret_cast<unsigned long long*>(&out->sum_q), v);
  }
}

// The sums of one evaluation, for several poses at once.  Workgroup (g, k) = blockIdx.x = k * G + g takes pose k and the points i with (i / 256) % G == g, lane
// i % 256, each lane its points in ascending order.  Row of a point: phi and the gradient g by kf_map_sample's lines at w; it takes part when observed and
// fabsf(phi) < gate; x = (float)(w - centre), the difference in fp64; J = (x cross g, g) in fp32, e = -phi; the
// row enters the lane's sums and the workgroup folds them as in k_store_align_sums (align_rows.h); a lane sees at most 2^24 points.
__global__ void __launch_bounds__(256) k_pose_sums(MapRef m, unsigned n_points, const float* __restrict__ pts, unsigned groups, const KfAlignXf* __restrict__ pc,
                                                   float gate, double* __restrict__ rows) {
  const unsigned pose = blockIdx.x / groups, grp = blockIdx.x - pose * groups;
  const KfAlignXf* __restrict__ P = pc + pose;
  MapBrick b = map_brick_none();
  double acc[28];
#pragma unroll
  for (int k = 0; k < 28; ++k) acc[k] = 0.0;
  unsigned n = 0u;
  for (size_t i = (size_t)grp * 256u + threadIdx.x; i < n_points; i += (size_t)groups * 256u) {
    double w0, w1, w2;
    pose_point(P->m, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], w0, w1, w2);
    QuerySample s;
    if (!query_sample<true, false>(m, w0, w1, w2, b, s) || !(fabsf(s.tsdf) < gate)) continue;
    const float x0 = (float)(w0 - P->c[0]), x1 = (float)(w1 - P->c[1]), x2 = (float)(w2 - P->c[2]);
    const double J[6] = {(double)(x1 * s.gz - x2 * s.gy), (double)(x2 * s.gx - x0 * s.gz), (double)(x0 * s.gy - x1 * s.gx), (double)s.gx, (double)s.gy, (double)s.gz};
    const double e = (double)(-s.tsdf);
    align_row_add(J, e, acc, n);
  }
  align_rows_fold(acc, n, rows + (size_t)blockIdx.x * KF_ALIGN_SUMS);
}

// the finishing launch: a pose's `groups` rows added in ascending order, one lane per entry
__global__ void __launch_bounds__(256) k_pose_sums_fold(unsigned n_poses, unsigned groups, const double* __restrict__ rows, double* __restrict__ sums) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n_poses * KF_ALIGN_SUMS) return;
  const unsigned pose = i / KF_ALIGN_SUMS, k = i - pose * KF_ALIGN_SUMS;
  const double* __restrict__ r = rows + (size_t)pose * groups * KF_ALIGN_SUMS + k;
  double v = 0.0;
  for (unsigned g = 0; g < groups; ++g) v += r[(size_t)g * KF_ALIGN_SUMS];
  sums[i] = v;
}

static inline bool score_args_ok(uint32_t n_points, uint32_t n_poses, uint32_t max_poses, float band) {
  return n_points >= 1u && n_points <= KF_SCORE_MAX_POINTS && n_poses >= 1u && n_poses <= max_poses && isfinite(band) && band > 0.f && band <= 1.f;
}

extern "C" int kf_map_score_poses_device(kf_ctx* c, uint32_t n_points, const float* dev_points, uint32_t n_poses, const double* dev_poses, float band,
                                         kf_pose_score* dev_scores) {
  if (!c || !dev_points || !dev_poses || !dev_scores || !score_args_ok(n_points, n_poses, KF_SCORE_MAX_POSES, band)) return KF_ERR_ARG;
  if (!kf_whole_volume(c)) return KF_ERR_STATE;
  KF_CHECK(hipSetDevice(c->cfg.device));
  // the chunking: a small pose count is spread over the chip, a large one gets one workgroup per pose that walks all the points
  const unsigned most = (n_points + 255u) / 256u, want = (KF_SCORE_TARGET_GROUPS + n_poses - 1u) / n_poses;
  const unsigned n_chunks = want < most ? want : most;
  KF_CHECK(hipMemsetAsync(dev_scores, 0, (size_t)n_poses * sizeof(kf_pose_score), c->stream));
  hipLaunchKernelGGL(k_score_poses, dim3(n_poses * n_chunks), dim3(256), 0, c->stream, query_map(c), n_points, dev_points, n_chunks, dev_poses, band, dev_scores);
  return (int)hipGetLastError();
}

extern "C" int kf_map_score_poses(kf_ctx* c, uint32_t n_points, const float* points, uint32_t n_poses, const double* poses, float band, kf_pose_score* scores) {
  if (!c || !points || !poses || !scores || !score_args_ok(n_points, n_poses, KF_SCORE_MAX_POSES, band)) return KF_ERR_ARG;
  if (!kf_whole_volume(c)) return KF_ERR_STATE;
  KF_CHECK(hipSetDevice(c->cfg.device));
  const size_t b_pts = 12 * (size_t)n_points, b_pose = 96 * (size_t)n_poses, b_sc = sizeof(kf_pose_score) * (size_t)n_poses;
  KfCarveTemp tmp;
  if (!tmp.get(KfCarveTemp::pad(b_pts) + KfCarveTemp::pad(b_pose) + KfCarveTemp::pad(b_sc))) return KF_ERR_ALLOC;
  const double* d_pose = tmp.up(c, poses, b_pose);
  const float* d_pts = tmp.up(c, points, b_pts);
  kf_pose_score* d_sc = tmp.down(scores, b_sc);
  return tmp.finish(c, tmp.st ? tmp.st : kf_map_score_poses_device(c, n_points, d_pts, n_poses, d_pose, band, d_sc));
}

// the device side of kf_map_pose_sums and kf_map_refine_poses: the points once, then per evaluation the poses in, the folded sums out
struct PoseSumsRun {
  KfCarveTemp tmp;
  float* d_pts = nullptr; KfAlignXf* d_pc = nullptr; double* d_rows = nullptr; double* d_sums = nullptr;
  unsigned n_points = 0, groups = 0;
  // false: the temporary does not fit
  bool get(uint32_t points, uint32_t poses) {
    n_points = points;
    groups = (points + 255u) / 256u;
    if (groups > KF_SUMS_MAX_GROUPS) groups = KF_SUMS_MAX_GROUPS;
    const size_t b_pts = 12 * (size_t)points, b_pc = sizeof(KfAlignXf) * (size_t)poses, b_sums = 8 * (size_t)KF_ALIGN_SUMS * poses, b_rows = b_sums * groups;
    if (!tmp.get(KfCarveTemp::pad(b_pts) + KfCarveTemp::pad(b_pc) + KfCarveTemp::pad(b_sums) + KfCarveTemp::pad(b_rows))) return false;
    d_pc = (KfAlignXf*)tmp.take(b_pc); d_rows = (double*)tmp.take(b_rows); d_sums = (double*)tmp.take(b_sums); d_pts = (float*)tmp.take(b_pts);
    return true;
  }
  // the sums of pc[0 .. n) into sums (29 n doubles); blocks
  int eval(kf_ctx* c, unsigned n, const KfAlignXf* pc, float gate, double* sums) {
    int st = (int)hipMemcpyAsync(d_pc, pc, sizeof(KfAlignXf) * (size_t)n, hipMemcpyHostToDevice, c->stream);
    if (!st) {
      hipLaunchKernelGGL(k_pose_sums, dim3(n * groups), dim3(256), 0, c->stream, query_map(c), n_points, d_pts, groups, d_pc, gate, d_rows);
      hipLaunchKernelGGL(k_pose_sums_fold, dim3((n * KF_ALIGN_SUMS + 255u) / 256u), dim3(256), 0, c->stream, n, groups, d_rows, d_sums);
      st = (int)hipGetLastError();
    }
    if (!st) st = (int)hipMemcpyAsync(sums, d_sums, 8 * (size_t)KF_ALIGN_SUMS * n, hipMemcpyDeviceToHost, c->stream);
    const int ss = (int)hipStreamSynchronize(c->stream);
    return st ? st : ss;
  }
};

static bool all_finite(const double* v, size_t n) {
  for (size_t i = 0; i < n; ++i) if (!isfinite(v[i])) return false;
  return true;
}

extern "C" int kf_map_pose_sums(kf_ctx* c, uint32_t n_points, const float* points, uint32_t n_poses, const double* poses, const double* centres, float gate,
                                double* sums) {
  if (!c || !points || !poses || !centres || !sums || !score_args_ok(n_points, n_poses, KF_SUMS_MAX_POSES, gate)) return KF_ERR_ARG;
  if (!all_finite(poses, 12 * (size_t)n_poses) || !all_finite(centres, 3 * (size_t)n_poses)) return KF_ERR_ARG;
  if (!kf_whole_volume(c)) return KF_ERR_STATE;
  std::vector<KfAlignXf> pc;
  std::vector<double> out;
  try { pc.resize(n_poses); out.resize((size_t)KF_ALIGN_SUMS * n_poses); } catch (const std::bad_alloc&) { return KF_ERR_ALLOC; }   // (no exception crosses the C boundary)
  for (uint32_t k = 0; k < n_poses; ++k) { memcpy(pc[k].m, poses + 12 * (size_t)k, sizeof(pc[k].m)); memcpy(pc[k].c, centres + 3 * (size_t)k, sizeof(pc[k].c)); }
  KF_CHECK(hipSetDevice(c->cfg.device));
  PoseSumsRun run;
  if (!run.get(n_points, n_poses)) return KF_ERR_ALLOC;
  int st = (int)hipMemcpyAsync(run.d_pts, points, 12 * (size_t)n_points, hipMemcpyHostToDevice, c->stream);
  if (st) { (void)hipStreamSynchronize(c->stream); return st; }
  st = run.eval(c, n_poses, pc.data(), gate, out.data());
  if (st) return st;
  memcpy(sums, out.data(), out.size() * sizeof(double));             // (only a call that succeeded writes)
  return 0;
}

extern "C" int kf_map_refine_poses(kf_ctx* c, uint32_t n_points, const float* points, uint32_t n_poses, double* poses, const double* centres,
                                   const kf_refine_params* params, kf_align_report* reports) {
  if (!c || !points || !poses || !centres || !params || !reports || !score_args_ok(n_points, n_poses, KF_SUMS_MAX_POSES, params->gate)) return KF_ERR_ARG;
  if (!all_finite(poses, 12 * (size_t)n_poses) || !kf_align_stop_valid(params->eps_rot, params->eps_trans, centres, n_poses)) return KF_ERR_ARG;
  if (!kf_whole_volume(c)) return KF_ERR_STATE;
  std::vector<KfAlignLoop> st;
  std::vector<uint32_t> live;                                        // the poses still running, ascending
  std::vector<KfAlignXf> pc;
  std::vector<double> sums;
  try { st.resize(n_poses); live.resize(n_poses); pc.resize(n_poses); sums.resize((size_t)KF_ALIGN_SUMS * n_poses); } catch (const std::bad_alloc&) { return KF_ERR_ALLOC; }
  for (uint32_t k = 0; k < n_poses; ++k) { kf_align_loop_begin(st[k], poses + 12 * (size_t)k); live[k] = k; }
  KF_CHECK(hipSetDevice(c->cfg.device));
  PoseSumsRun run;
  if (!run.get(n_points, n_poses)) return KF_ERR_ALLOC;
  {
    const int e = (int)hipMemcpyAsync(run.d_pts, points, 12 * (size_t)n_points, hipMemcpyHostToDevice, c->stream);
    if (e) { (void)hipStreamSynchronize(c->stream); return e; }
  }
  while (!live.empty()) {
    // one launch and one read-back for all the poses still running
    for (size_t a = 0; a < live.size(); ++a) { memcpy(pc[a].m, st[live[a]].cur, sizeof(pc[a].m)); memcpy(pc[a].c, centres + 3 * (size_t)live[a], sizeof(pc[a].c)); }
    const int e = run.eval(c, (unsigned)live.size(), pc.data(), params->gate, sums.data());
    if (e) return e;                                                 // (nothing written)
    size_t kept = 0;
    for (size_t a = 0; a < live.size(); ++a)                          // (the stepped pose is not checked for being rigid: the poses that go in are not either)
      if (kf_align_loop_turn(st[live[a]], sums.data() + (size_t)KF_ALIGN_SUMS * a, centres + 3 * (size_t)live[a], params->max_iter, params->min_pairs,
                             params->eps_rot, params->eps_trans, false))
        live[kept++] = live[a];
    live.resize(kept);
  }
  for (uint32_t k = 0; k < n_poses; ++k) { memcpy(poses + 12 * (size_t)k, st[k].good, sizeof(st[k].good)); reports[k] = st[k].rep; }
  return 0;
}
