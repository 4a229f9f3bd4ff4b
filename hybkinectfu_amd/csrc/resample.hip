// resample.hip -- merging a map under a rigid transform: the incoming map is resampled at the destination's voxel centres, trilinearly, through a hash
// table of its own (resample_shared.h: the upload, source_bricks27, source_corner), and the resampled bricks meet the held ones under kf_merge_brick_store's
// rule (store_merge.h: store_merge_pair).  No reference counterpart.  The rule is written out above kf_merge_brick_store_rigid in include/hybkf.h; the host
// side (is it a transform, the candidate bricks, a candidate's base corner in fp64, the source keys and their table) is rigid_keys.h.
#include "kf_internal.h"
#include "brick_key.h"
#include "brick_find.h"
#include "store_merge.h"
#include "rigid_keys.h"
#include "resample_shared.h"
#include <stdint.h>
#include <new>
#include <vector>

// eight corner values (index: dx | dy << 1 | dz << 2) along x, then y, then z; an axis whose fraction is 0 passes its value on untouched.  (A corner that is
// not used holds 0 and meets only lerps that are not applied.)
__device__ __forceinline__ float lerp3(const float (&v)[8], float fx, float fy, float fz) {
  float a[4], b[2];
#pragma unroll
  for (int k = 0; k < 4; ++k) a[k] = fx > 0.f ? lerp1(v[2 * k], v[2 * k + 1], fx) : v[2 * k];
#pragma unroll
  for (int k = 0; k < 2; ++k) b[k] = fy > 0.f ? lerp1(a[2 * k], a[2 * k + 1], fy) : a[2 * k];
  return fz > 0.f ? lerp1(b[0], b[1], fz) : b[0];
}

// One destination voxel: (ux, uy, uz) its source position relative to the brick's base corner (ibx, iby, ibz).  The eight corners floor(u) + {0, 1}^3, of
// which the +1 ones are used on an axis only where the fraction is > 0; a used corner whose brick the source does not hold, or whose weight is not > 0,
// leaves the voxel unobserved: (0, 0, 0).  s_src, (b0x, b0y, b0z): source_bricks27's.
template <bool COLOR>
__device__ __forceinline__ KfIncoming resample_voxel(const KfResampleSource& src, const unsigned* s_src, float ux, float uy, float uz, int ibx, int iby, int ibz,
                                                      int b0x, int b0y, int b0z) {
  float fx, fy, fz;
  const int ix = source_split(ux, ibx, fx), iy = source_split(uy, iby, fy), iz = source_split(uz, ibz, fz);
  float t[8];
  unsigned cc[8];                                            // the corners' colours, packed; a channel becomes a float where it is lerped
  float wmin = 3.0e38f;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int dx = k & 1, dy = (k >> 1) & 1, dz = k >> 2;
    const bool used = ok && (!dx || fx > 0.f) && (!dy || fy > 0.f) && (!dz || fz > 0.f);
    const KfSourceCorner c = source_corner(src, s_src, ix + dx, iy + dy, iz + dz, b0x, b0y, b0z, used);
    t[k] = c.t; cc[k] = 0u;
    if (COLOR && src.color && c.held) cc[k] = (unsigned)src.color[3 * c.o] | ((unsigned)src.color[3 * c.o + 1] << 8) | ((unsigned)src.color[3 * c.o + 2] << 16);
    if (used) { ok = c.w > 0.f; wmin = fminf(wmin, c.w); }
  }
  KfIncoming r = {0.f, 0.f, 0u};
  if (!ok) return r;
  r.t = lerp3(t, fx, fy, fz); r.w = wmin;
  if (COLOR && src.color) {
#pragma unroll
    for (int s = 0; s < 24; s += 8) {
      float v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = (float)((cc[k] >> s) & 255u);
      r.c |= (unsigned)(unsigned char)fminf(255.f, lerp3(v, fx, fy, fz) + 0.5f) << s;
    }
  }
  return r;
}

// Resample and merge for kf_merge_brick_store_rigid.  One workgroup iteration per candidate destination brick, 256 lanes x 2 x-adjacent voxels (the slot's
// float4).  ckeys / cib / cfb: per candidate its key, and the source position of its voxel (0, 0, 0) as an integer and a fraction (rigid_keys.h).  r<i><j>:
// (float)R[i][j], nine scalars (a by-value array indexed at run time would go to scratch: see KfBrickBoxes, brickstore.hip).
// The 27 source slots the brick can draw on are looked up once into LDS (source_bricks27: its bound on the source range of one brick); when the source holds
// none of them the brick is done.  What the lanes resample meets the store under store_merge_pair.  Candidate keys are unique: no two workgroups meet in a slot.
template <bool COLOR>
__global__ void __launch_bounds__(256) k_store_resample_merge(KfBrickStore st, KfBrickStore stab, KfResampleSource src, unsigned count,
                                                              const int32_t* __restrict__ ckeys, const int32_t* __restrict__ cib, const float* __restrict__ cfb,
                                                              float r00, float r01, float r02, float r10, float r11, float r12, float r20, float r21, float r22,
                                                              float max_weight) {
  __shared__ unsigned s_src[27];
  __shared__ KfMergeShared sh;
  const float lx = (float)((threadIdx.x & 3u) << 1), ly = (float)((threadIdx.x >> 2) & 7u), lz = (float)(threadIdx.x >> 5);
  for (unsigned e = blockIdx.x; e < count; e += gridDim.x) {
    const int ibx = cib[3 * e], iby = cib[3 * e + 1], ibz = cib[3 * e + 2];
    const float fbx = cfb[3 * e], fby = cfb[3 * e + 1], fbz = cfb[3 * e + 2];
    int b0x, b0y, b0z;                                                        // everybody has read the last iteration's slots: the barriers below
    const bool any = source_bricks27(stab, true, ibx, iby, ibz, fbx, fby, fbz, r00, r01, r02, r10, r11, r12, r20, r21, r22, b0x, b0y, b0z, s_src);
    if (!__syncthreads_or(any)) continue;                                     // (workgroup-uniform) nothing of the source near this brick
    // u_j = ((r0j lx + r1j ly) + r2j lz) + fb_j, for the lane's voxel and its +x neighbour
    const float u0x = ((r00 * lx + r10 * ly) + r20 * lz) + fbx, u0y = ((r01 * lx + r11 * ly) + r21 * lz) + fby, u0z = ((r02 * lx + r12 * ly) + r22 * lz) + fbz;
    const float lx1 = lx + 1.f;
    const float u1x = ((r00 * lx1 + r10 * ly) + r20 * lz) + fbx, u1y = ((r01 * lx1 + r11 * ly) + r21 * lz) + fby, u1z = ((r02 * lx1 + r12 * ly) + r22 * lz) + fbz;
    const KfIncoming v0 = resample_voxel<COLOR>(src, s_src, u0x, u0y, u0z, ibx, iby, ibz, b0x, b0y, b0z);
    const KfIncoming v1 = resample_voxel<COLOR>(src, s_src, u1x, u1y, u1z, ibx, iby, ibz, b0x, b0y, b0z);
    store_merge_pair<COLOR>(st, kf_brick_key_pack(ckeys[3 * e], ckeys[3 * e + 1], ckeys[3 * e + 2]), v0, v1, src.color != nullptr, max_weight, sh);
  }
}

extern "C" int64_t kf_rigid_brick_keys(uint32_t count, const int32_t* keys, const double xf[12], int32_t* out_keys, int64_t cap) {
  try { return kf_rigid_keys(count, keys, xf, out_keys, cap); } catch (const std::bad_alloc&) { return -1; }   // (no exception crosses the C boundary)
}

extern "C" int kf_merge_brick_store_rigid(kf_ctx* c, uint32_t count, const int32_t* keys, const float* tsdf, const float* weight, const uint8_t* color,
                                          const double xf[12]) {
  if (!c) return KF_ERR_ARG;
  if (!c->bstore.max_bricks) return KF_ERR_STATE;
  if (color && !c->bstore.color) return KF_ERR_STATE;
  if (count == 0) return 0;                                  // nothing to merge: the arrays are not looked at
  if (!keys || !tsdf || !weight || !kf_rigid_valid(xf)) return KF_ERR_ARG;
  if (count > (1u << 30)) return KF_ERR_ALLOC;               // (the source table's probe counts entries in 32 bits, as the store's does; 2^30 bricks would be 4 TiB)
  std::vector<uint64_t> words;
  std::vector<unsigned long long> tkey;
  std::vector<unsigned> tslot;
  std::vector<int32_t> ckeys, cib;
  std::vector<float> cfb;
  uint32_t mask = 0;
  try {                                                      // (no exception crosses the C boundary)
    if (!kf_source_keys_table(count, keys, tkey, tslot, mask)) return KF_ERR_ARG;
    if (kf_rigid_candidates(count, keys, xf, words) < 0) return KF_ERR_ARG;   // a destination brick outside the key range
    ckeys.reserve(words.size() * 3); cib.reserve(words.size() * 3); cfb.reserve(words.size() * 3);
    for (const uint64_t w : words) {
      int32_t k3[3], ib[3];
      float fb[3];
      kf_rigid_word_key(w, k3);
      if (!kf_rigid_brick_base(xf, k3, ib, fb)) continue;    // (not reached for source keys in range: nowhere near the source)
      for (int k = 0; k < 3; ++k) { ckeys.push_back(k3[k]); cib.push_back(ib[k]); cfb.push_back(fb[k]); }
    }
  } catch (const std::bad_alloc&) { return KF_ERR_ALLOC; }
  const size_t ncand = ckeys.size() / 3;
  if (ncand == 0) return 0;
  if (ncand > 0xFFFFFFFFull) return KF_ERR_ALLOC;
  KF_CHECK(hipSetDevice(c->cfg.device));
  KfResampleTemp tmp;
  float* dfb = nullptr;
  int32_t *dck = nullptr, *dib = nullptr;
  KfBrickStore stab;
  KfResampleSource src;
  hipError_t e;
  if (!tmp.get((void**)&dck, ncand * 3 * sizeof(int32_t)) || !tmp.get((void**)&dib, ncand * 3 * sizeof(int32_t)) || !tmp.get((void**)&dfb, ncand * 3 * sizeof(float)) ||
      !kf_source_map_upload(c, tmp, count, tsdf, weight, color, tkey, tslot, mask, stab, src, e))
    return KF_ERR_ALLOC;                                     // nothing touched  (a colour without a colour plane was refused above)
  if (e == hipSuccess) e = hipMemcpyAsync(dck, ckeys.data(), ncand * 3 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dib, cib.data(), ncand * 3 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dfb, cfb.data(), ncand * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    const dim3 grid(ncand > 4096u ? 4096u : (unsigned)ncand), block(256);   // store_pass's cap
    const float r[9] = {(float)xf[0], (float)xf[1], (float)xf[2], (float)xf[4], (float)xf[5], (float)xf[6], (float)xf[8], (float)xf[9], (float)xf[10]};
    if (c->bstore.color) hipLaunchKernelGGL(k_store_resample_merge<true>, grid, block, 0, c->stream, c->bstore, stab, src, (unsigned)ncand, dck, dib, dfb,
                                            r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], c->vol.max_weight);
    else hipLaunchKernelGGL(k_store_resample_merge<false>, grid, block, 0, c->stream, c->bstore, stab, src, (unsigned)ncand, dck, dib, dfb,
                            r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], c->vol.max_weight);
    e = hipGetLastError();
  }
  const hipError_t se = hipStreamSynchronize(c->stream);     // on success and on failure alike: nothing still reads the caller's arrays or the temporaries
  return (int)(e != hipSuccess ? e : se);
}
