// align.hip -- aligning two maps: the rigid transform a map merge needs, found by Gauss-Newton on the SDF-to-SDF error between the brick store and an
// incoming map.  No reference counterpart.  The rule is written out above kf_align_brick_store in include/hybkf.h; one evaluation of the 29 sums is the
// kernel below -- how a row enters them and how a workgroup folds them is align_rows.h, shared with relocal.hip --, the step from the sums to the next
// transform and the turn of the loop that gives the verdicts are align_step.h (host, fp64), the source keys' check and table and a brick's base corner are
// rigid_keys.h, the source's upload, its 27 bricks around a held one and a corner's fetch are the rigid merge's (resample_shared.h).
#include "kf_internal.h"
#include "brick_key.h"
#include "brick_find.h"
#include "rigid_keys.h"
#include "resample_shared.h"
#include "align_rows.h"
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <new>
#include <vector>

#define KF_ALIGN_MAX_GROUPS 1024u      // the grid is min(held, this): a fixed function of the held count, so the fold order is too

// One held voxel in the band: td its tsdf, (ux, uy, uz) its source position relative to the brick's base corner (ibx, iby, ibz), (xx, xy, xz) its position
// relative to the centre.  All eight corners floor(u) + {0, 1}^3 are read; one that the source does not hold, whose weight is not > 0 or whose |tsdf| is
// not < 1 leaves the voxel out.  s_src, (b0x, b0y, b0z): source_bricks27's.  Adds the voxel's row to acc and n (align_row_add).
__device__ __forceinline__ void align_voxel(const KfResampleSource& src, const unsigned* s_src, float td, float ux, float uy, float uz, int ibx, int iby, int ibz,
                                            int b0x, int b0y, int b0z, float xx, float xy, float xz, float r00, float r01, float r02, float r10, float r11,
                                            float r12, float r20, float r21, float r22, double (&acc)[28], unsigned& n) {
  float fx, fy, fz;
  const int ix = source_split(ux, ibx, fx), iy = source_split(uy, iby, fy), iz = source_split(uz, ibz, fz);
  float v[8];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const KfSourceCorner c = source_corner(src, s_src, ix + (k & 1), iy + ((k >> 1) & 1), iz + (k >> 2), b0x, b0y, b0z, ok);
    v[k] = c.t;
    ok = ok && c.w > 0.f && fabsf(c.t) < 1.f;
  }
  if (!ok) return;
  // the value: x, then y, then z; the gradient in source voxels from the same eight values
  const float a0 = lerp1(v[0], v[1], fx), a1 = lerp1(v[2], v[3], fx), a2 = lerp1(v[4], v[5], fx), a3 = lerp1(v[6], v[7], fx);
  const float b0 = lerp1(a0, a1, fy), b1 = lerp1(a2, a3, fy);
  const float phi = lerp1(b0, b1, fz);
  const float d0 = v[1] - v[0], d1 = v[3] - v[2], d2 = v[5] - v[4], d3 = v[7] - v[6];
  const float gx = lerp1(lerp1(d0, d1, fy), lerp1(d2, d3, fy), fz);
  const float gy = lerp1(a1 - a0, a3 - a2, fz);
  const float gz = b1 - b0;
  // the row: the gradient in the destination's axes, J = (x cross gd, gd), e = phi - td
  const float gdx = (r00 * gx + r01 * gy) + r02 * gz, gdy = (r10 * gx + r11 * gy) + r12 * gz, gdz = (r20 * gx + r21 * gy) + r22 * gz;
  const double J[6] = {(double)(xy * gdz - xz * gdy), (double)(xz * gdx - xx * gdz), (double)(xx * gdy - xy * gdx), (double)gdx, (double)gdy, (double)gdz};
  const double e = (double)(phi - td);
  align_row_add(J, e, acc, n);
}

// The sums of one evaluation for kf_align_brick_store.  One workgroup iteration per held slot, 256 lanes x 2 x-adjacent voxels (the slot's float4); the
// slots are read only.  order: the held slots by ascending key, so which workgroup adds which brick, and when, depends on the keys held and not on the slots
// they happened to claim.  Per slot: its key, the base corner ib / fb by kf_rigid_brick_base's formula in fp64 (the same operations in the same order, no
// contraction: the host function's bits; a corner that does not fit 31 bits leaves the slot out), the 27 source slots by source_bricks27.
// One barrier per iteration: the lanes OR two bits into a flags word -- the source holds one of the 27; a held voxel lies in the band -- and the workgroup
// goes on only with both.  The word is one of three in rotation (the one used two iterations later is cleared after this iteration's barrier, which every
// lane has passed before it can write to it), the 27 slots one of two sets (a lane can write the other set while a slower one still reads this one, and
// reaches this one again only past the next barrier).
// Every lane keeps 28 fp64 sums and an integer count across its iterations (at most 2^20 iterations of 512 voxels); at the end the workgroup folds them in a
// fixed order and writes its row of 29 doubles (align_rows_fold): no atomic on a float anywhere, the same bits on every run.
__global__ void __launch_bounds__(256) k_store_align_sums(KfBrickStore st, KfBrickStore stab, KfResampleSource src, unsigned held, KfAlignXf xf,
                                                          const unsigned* __restrict__ order, double* __restrict__ rows) {
  __shared__ unsigned s_src[2][27];
  __shared__ unsigned s_flag[3];
  const float r00 = (float)xf.m[0], r01 = (float)xf.m[1], r02 = (float)xf.m[2], r10 = (float)xf.m[4], r11 = (float)xf.m[5], r12 = (float)xf.m[6];
  const float r20 = (float)xf.m[8], r21 = (float)xf.m[9], r22 = (float)xf.m[10];
  const float lx = (float)((threadIdx.x & 3u) << 1), ly = (float)((threadIdx.x >> 2) & 7u), lz = (float)(threadIdx.x >> 5);
  double acc[28];
#pragma unroll
  for (int k = 0; k < 28; ++k) acc[k] = 0.0;
  unsigned n = 0u;
  if (threadIdx.x < 3u) s_flag[threadIdx.x] = 0u;
  __syncthreads();
  unsigned par = 0u, tri = 0u;
  for (unsigned e = blockIdx.x; e < held; e += gridDim.x, par ^= 1u, tri = tri == 2u ? 0u : tri + 1u) {
    const unsigned slot = order[e];
    int32_t K[3];
    kf_brick_key_unpack(st.key[slot], K);
    // kf_rigid_brick_base, and the bracket of x_j = (float)(8 K_j + 0.5 - centre_j) + l_j
    const double q0 = 8.0 * K[0] + 0.5, q1 = 8.0 * K[1] + 0.5, q2 = 8.0 * K[2] + 0.5;
    const double a0 = q0 - xf.m[3], a1 = q1 - xf.m[7], a2 = q2 - xf.m[11];
    int ib[3];
    float fb[3];
    bool fit = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double c = ((xf.m[j] * a0 + xf.m[4 + j] * a1) + xf.m[8 + j] * a2) - 0.5;
      const double fl = floor(c);
      fit = fit && fl >= -1073741824.0 && fl < 1073741824.0;
      ib[j] = fit ? (int)fl : 0;
      fb[j] = (float)(c - fl);
      if (fb[j] == 1.0f) { ib[j] += 1; fb[j] = 0.f; }
    }
    const float xbx = (float)(q0 - xf.c[0]), xby = (float)(q1 - xf.c[1]), xbz = (float)(q2 - xf.c[2]);
    const float4 h = reinterpret_cast<const float4*>(st.tw + (size_t)slot * KF_BRICK_VOX)[threadIdx.x];
    const bool in0 = h.y > 0.f && fabsf(h.x) < 1.f, in1 = h.w > 0.f && fabsf(h.z) < 1.f;
    int b0x, b0y, b0z;
    const bool any = source_bricks27(stab, fit, ib[0], ib[1], ib[2], fb[0], fb[1], fb[2], r00, r01, r02, r10, r11, r12, r20, r21, r22, b0x, b0y, b0z, s_src[par]);
    const unsigned bits = (__ballot(any) ? 1u : 0u) | (__ballot(fit && (in0 || in1)) ? 2u : 0u);   // (wave-uniform)
    if ((threadIdx.x & 63u) == 0u && bits) atomicOr(&s_flag[tri], bits);
    __syncthreads();
    const unsigned both = s_flag[tri];
    if (threadIdx.x == 0u) s_flag[tri == 0u ? 2u : tri - 1u] = 0u;            // the word of the iteration after the next
    if (both != 3u) continue;                                                 // (workgroup-uniform) nothing of the source near this brick, or nothing held in the band
    // u_j = ((r0j lx + r1j ly) + r2j lz) + fb_j, for the lane's voxel and its +x neighbour
#pragma unroll 1
    for (int i = 0; i < 2; ++i) {
      if (!(i ? in1 : in0)) continue;
      const float vx = i ? lx + 1.f : lx;
      const float ux = ((r00 * vx + r10 * ly) + r20 * lz) + fb[0], uy = ((r01 * vx + r11 * ly) + r21 * lz) + fb[1], uz = ((r02 * vx + r12 * ly) + r22 * lz) + fb[2];
      align_voxel(src, s_src[par], i ? h.z : h.x, ux, uy, uz, ib[0], ib[1], ib[2], b0x, b0y, b0z, xbx + vx, xby + ly, xbz + lz, r00, r01, r02, r10, r11, r12,
                  r20, r21, r22, acc, n);
    }
  }
  align_rows_fold(acc, n, rows + (size_t)blockIdx.x * KF_ALIGN_SUMS);
}

extern "C" int kf_align_step(const double sums[29], const double centre[3], double xf[12], double step[6]) {
  return kf_align_step_host(sums, centre, xf, step);
}

extern "C" int kf_align_brick_store(kf_ctx* c, uint32_t count, const int32_t* keys, const float* tsdf, const float* weight, double xf[12],
                                    const kf_align_params* params, kf_align_report* report) {
  if (!c || !xf || !params || !report) return KF_ERR_ARG;
  if (!kf_whole_volume(c)) return KF_ERR_ARG;                // a z-slab context has no store
  if (!c->bstore.max_bricks) return KF_ERR_STATE;
  if ((count && (!keys || !tsdf || !weight)) || !kf_rigid_valid(xf) || !kf_align_stop_valid(params->eps_rot, params->eps_trans, params->centre, 1)) return KF_ERR_ARG;
  if (count > (1u << 30)) return KF_ERR_ALLOC;               // (as kf_merge_brick_store_rigid: the source table's probe counts entries in 32 bits)
  std::vector<unsigned long long> tkey;
  std::vector<unsigned> tslot;
  std::vector<double> rows;
  std::vector<unsigned long long> hkeys;
  std::vector<unsigned> order;
  uint32_t mask = 0, held = 0;
  try {                                                      // (no exception crosses the C boundary)
    if (!kf_source_keys_table(count, keys, tkey, tslot, mask)) return KF_ERR_ARG;
    rows.resize((size_t)KF_ALIGN_MAX_GROUPS * KF_ALIGN_SUMS);
  } catch (const std::bad_alloc&) { return KF_ERR_ALLOC; }
  KF_CHECK(hipSetDevice(c->cfg.device));
  { const int cs = kf_brick_store_count(c, &held, nullptr, nullptr); if (cs) return cs; }
  const unsigned groups = held > KF_ALIGN_MAX_GROUPS ? KF_ALIGN_MAX_GROUPS : held;
  // the held slots by ascending key (keys are unique): the order of every sum is then a function of the keys held alone
  try { hkeys.resize(held); order.resize(held); } catch (const std::bad_alloc&) { return KF_ERR_ALLOC; }
  if (held) {
    KF_CHECK(hipMemcpyAsync(hkeys.data(), c->bstore.key, (size_t)held * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    KF_CHECK(hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < held; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](unsigned a, unsigned b) { return hkeys[a] < hkeys[b]; });
  }
  KfResampleTemp tmp;
  double* drows = nullptr;
  unsigned* dorder = nullptr;
  KfBrickStore stab;
  KfResampleSource src;
  hipError_t e;
  if (!tmp.get((void**)&drows, (size_t)KF_ALIGN_MAX_GROUPS * KF_ALIGN_SUMS * sizeof(double)) || !tmp.get((void**)&dorder, (size_t)held * sizeof(unsigned)) ||
      !kf_source_map_upload(c, tmp, count, tsdf, weight, nullptr, tkey, tslot, mask, stab, src, e))   // the source goes up once, without its colour
    return KF_ERR_ALLOC;                                     // nothing touched
  if (e == hipSuccess && held) e = hipMemcpyAsync(dorder, order.data(), (size_t)held * sizeof(unsigned), hipMemcpyHostToDevice, c->stream);
  {
    const hipError_t se = hipStreamSynchronize(c->stream);   // on success and on failure alike: nothing still reads the caller's arrays
    if (e != hipSuccess || se != hipSuccess) return (int)(e != hipSuccess ? e : se);
  }
  KfAlignLoop loop;
  kf_align_loop_begin(loop, xf);
  double sums[KF_ALIGN_SUMS];
  do {
    // the sums at loop.cur: one row per workgroup, folded here in index order
    memset(sums, 0, sizeof(sums));
    if (groups) {
      KfAlignXf kx;                                          // by value: every index is a constant, the 15 doubles stay in scalar registers
      memcpy(kx.m, loop.cur, sizeof(kx.m)); memcpy(kx.c, params->centre, sizeof(kx.c));
      hipLaunchKernelGGL(k_store_align_sums, dim3(groups), dim3(256), 0, c->stream, c->bstore, stab, src, (unsigned)held, kx, dorder, drows);
      e = hipGetLastError();
      if (e == hipSuccess) e = hipMemcpyAsync(rows.data(), drows, (size_t)groups * KF_ALIGN_SUMS * sizeof(double), hipMemcpyDeviceToHost, c->stream);
      const hipError_t se = hipStreamSynchronize(c->stream);
      if (e != hipSuccess || se != hipSuccess) return (int)(e != hipSuccess ? e : se);
      for (unsigned g = 0; g < groups; ++g)
        for (int k = 0; k < KF_ALIGN_SUMS; ++k) sums[k] += rows[(size_t)g * KF_ALIGN_SUMS + k];
    }
  } while (kf_align_loop_turn(loop, sums, params->centre, params->max_iter, params->min_pairs, params->eps_rot, params->eps_trans, true));
  memcpy(xf, loop.good, sizeof(loop.good));
  *report = loop.rep;
  return 0;
}
