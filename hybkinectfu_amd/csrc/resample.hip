// resample.hip -- merging a map under a rigid transform: the incoming map is resampled at the destination's voxel centres, trilinearly, through a hash
// table of its own, and the resampled bricks meet the held ones under kf_merge_brick_store's rule (store_merge.h).  No reference counterpart.
// The rule is written out above kf_merge_brick_store_rigid in include/hybkf.h; the host side (is it a transform, the candidate bricks, a candidate's base
// corner in fp64, the source table) is rigid_keys.h.
#include "kf_internal.h"
#include "brick_key.h"
#include "brick_find.h"
#include "store_merge.h"
#include "brick_keys_unique.h"
#include "rigid_keys.h"
#include "resample_shared.h"
#include <stdint.h>
#include <new>
#include <vector>

// one resampled voxel; c: the colour packed as the slot holds it (x | y << 8 | z << 16)
struct KfResampled { float t, w; unsigned c; };

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
// leaves the voxel unobserved: (0, 0, 0).  s_src: the 27 source slots of bricks (b0x.., b0y.., b0z..) + [0, 3)^3; a corner outside them reads as unobserved
// (the caller's bound shows that none lies outside; the test keeps a rounding surprise from indexing past the table).
template <bool COLOR>
__device__ __forceinline__ KfResampled resample_voxel(const KfResampleSource& src, const unsigned* s_src, float ux, float uy, float uz, int ibx, int iby, int ibz,
                                                      int b0x, int b0y, int b0z) {
  const float nx = floorf(ux), ny = floorf(uy), nz = floorf(uz);
  const float fx = ux - nx, fy = uy - ny, fz = uz - nz;
  const int ix = ibx + (int)nx, iy = iby + (int)ny, iz = ibz + (int)nz;
  float t[8];
  unsigned cc[8];                                            // the corners' colours, packed; a channel becomes a float where it is lerped
  float wmin = 3.0e38f;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int dx = k & 1, dy = (k >> 1) & 1, dz = k >> 2;
    const bool used = ok && (!dx || fx > 0.f) && (!dy || fy > 0.f) && (!dz || fz > 0.f);
    const int x = ix + dx, y = iy + dy, z = iz + dz;
    const unsigned tx = (unsigned)((x >> 3) - b0x), ty = (unsigned)((y >> 3) - b0y), tz = (unsigned)((z >> 3) - b0z);
    const unsigned slot = (used && tx < 3u && ty < 3u && tz < 3u) ? s_src[(tz * 3u + ty) * 3u + tx] : KF_BRICK_NO_SLOT;
    float w = 0.f;
    t[k] = 0.f; cc[k] = 0u;
    if (slot != KF_BRICK_NO_SLOT) {
      const size_t o = (size_t)slot * KF_BRICK_VOX + (size_t)(((z & 7) << 6) | ((y & 7) << 3) | (x & 7));
      w = src.weight[o];
      t[k] = src.tsdf[o];
      if (COLOR && src.color) cc[k] = (unsigned)src.color[3 * o] | ((unsigned)src.color[3 * o + 1] << 8) | ((unsigned)src.color[3 * o + 2] << 16);
    }
    if (used) { ok = w > 0.f; wmin = fminf(wmin, w); }
  }
  KfResampled r = {0.f, 0.f, 0u};
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
// The source range of one brick: u_j = sum_i r_ij l_i + fb_j spans at most 7 (|r_0j| + |r_1j| + |r_2j|) <= 7 sqrt(3) (1 + 1e-5) < 12.13 (a column of R has a
// norm within 1e-5 of 1).  lo_j = sum_i min(0, 7 r_ij) + fb_j - 0.01 lies below every u_j the lanes compute (their roundings are far below 0.01), so with
// n0 = floor(lo_j) every corner floor(u_j) + {0, 1} lies in [n0, n0 + 14]: 15 integers, at most three source bricks per axis from brick (ib + n0) >> 3 on.
// Those 27 slots are looked up once, by the first 27 lanes, into LDS; when the source holds none of them the brick is done.
// After the workgroup-wide "any weight > 0" the path is k_store_merge's from its key look-up on.  Candidate keys are unique: no two workgroups meet in a slot.
template <bool COLOR>
__global__ void __launch_bounds__(256) k_store_resample_merge(KfBrickStore st, KfBrickStore stab, KfResampleSource src, unsigned count,
                                                              const int32_t* __restrict__ ckeys, const int32_t* __restrict__ cib, const float* __restrict__ cfb,
                                                              float r00, float r01, float r02, float r10, float r11, float r12, float r20, float r21, float r22,
                                                              float max_weight) {
  __shared__ unsigned s_src[27];
  __shared__ unsigned s_slot, s_fresh;
  __shared__ unsigned long long s_pend;
  const float lx = (float)((threadIdx.x & 3u) << 1), ly = (float)((threadIdx.x >> 2) & 7u), lz = (float)(threadIdx.x >> 5);
  for (unsigned e = blockIdx.x; e < count; e += gridDim.x) {
    const int ibx = cib[3 * e], iby = cib[3 * e + 1], ibz = cib[3 * e + 2];
    const float fbx = cfb[3 * e], fby = cfb[3 * e + 1], fbz = cfb[3 * e + 2];
    const int b0x = (ibx + (int)floorf(((least7(r00) + least7(r10)) + least7(r20)) + fbx - 0.01f)) >> 3;
    const int b0y = (iby + (int)floorf(((least7(r01) + least7(r11)) + least7(r21)) + fby - 0.01f)) >> 3;
    const int b0z = (ibz + (int)floorf(((least7(r02) + least7(r12)) + least7(r22)) + fbz - 0.01f)) >> 3;
    bool any = false;
    if (threadIdx.x < 27u) {                                                  // everybody has read the last iteration's slots: the barriers below
      const int bx = b0x + (int)(threadIdx.x % 3u), by = b0y + (int)((threadIdx.x / 3u) % 3u), bz = b0z + (int)(threadIdx.x / 9u);
      unsigned slot = KF_BRICK_NO_SLOT;                                       // (a brick outside the key range has no key: packed, it would alias another)
      if (kf_brick_key_in_range(bx) && kf_brick_key_in_range(by) && kf_brick_key_in_range(bz)) slot = store_find(stab, kf_brick_key_pack(bx, by, bz));
      s_src[threadIdx.x] = slot;
      any = slot != KF_BRICK_NO_SLOT;
    }
    if (!__syncthreads_or(any)) continue;                                     // (workgroup-uniform) nothing of the source near this brick
    // u_j = ((r0j lx + r1j ly) + r2j lz) + fb_j, for the lane's voxel and its +x neighbour
    const float u0x = ((r00 * lx + r10 * ly) + r20 * lz) + fbx, u0y = ((r01 * lx + r11 * ly) + r21 * lz) + fby, u0z = ((r02 * lx + r12 * ly) + r22 * lz) + fbz;
    const float lx1 = lx + 1.f;
    const float u1x = ((r00 * lx1 + r10 * ly) + r20 * lz) + fbx, u1y = ((r01 * lx1 + r11 * ly) + r21 * lz) + fby, u1z = ((r02 * lx1 + r12 * ly) + r22 * lz) + fbz;
    const KfResampled v0 = resample_voxel<COLOR>(src, s_src, u0x, u0y, u0z, ibx, iby, ibz, b0x, b0y, b0z);
    const KfResampled v1 = resample_voxel<COLOR>(src, s_src, u1x, u1y, u1z, ibx, iby, ibz, b0x, b0y, b0z);
    if (!__syncthreads_or(v0.w > 0.f || v1.w > 0.f)) continue;                // (workgroup-uniform) resamples to nothing: takes no slot, changes no held one
    const unsigned long long key = kf_brick_key_pack(ckeys[3 * e], ckeys[3 * e + 1], ckeys[3 * e + 2]);
    if (threadIdx.x == 0) {
      unsigned slot = store_find(st, key);
      const bool fresh = slot == KF_BRICK_NO_SLOT;
      if (fresh) slot = store_claim(st, key);
      s_slot = slot; s_fresh = fresh ? 1u : 0u;
      s_pend = fresh ? 0ull : st.pend[slot];
    }
    __syncthreads();
    const unsigned slot = s_slot;
    if (slot == KF_BRICK_NO_SLOT) continue;                                   // the store is full: counted as dropped
    float4* tw = reinterpret_cast<float4*>(st.tw + (size_t)slot * KF_BRICK_VOX) + threadIdx.x;
    if (s_fresh) {                                                            // (workgroup-uniform) k_store_import's write
      *tw = make_float4(v0.t, v0.w, v1.t, v1.w);
      if (COLOR) reinterpret_cast<uint2*>(st.color + (size_t)slot * KF_BRICK_VOX)[threadIdx.x] = make_uint2(v0.c, v1.c);
      if (threadIdx.x == 0) { st.pend[slot] = 0ull; st.key[slot] = key; }
      continue;
    }
    const unsigned pq = (unsigned)(s_pend >> (16u * (threadIdx.x >> 6))) & 0xFFFFu;   // (wave-uniform)
    const float4 h = *tw;
    const float wa0 = kf_pend_weight(h.y, pq, max_weight), wa1 = kf_pend_weight(h.w, pq, max_weight);
    const bool blend0 = v0.w > 0.f && wa0 > 0.f, take0 = v0.w > 0.f && !(wa0 > 0.f), blend1 = v1.w > 0.f && wa1 > 0.f, take1 = v1.w > 0.f && !(wa1 > 0.f);
    const float2 m0 = merge_voxel(h.x, wa0, v0.t, v0.w, max_weight, take0, blend0), m1 = merge_voxel(h.z, wa1, v1.t, v1.w, max_weight, take1, blend1);
    *tw = make_float4(m0.x, m0.y, m1.x, m1.y);
    if (COLOR && src.color) {                                                 // no colour given (kernel-uniform): the held colour stays
      uint2* cp = reinterpret_cast<uint2*>(st.color + (size_t)slot * KF_BRICK_VOX) + threadIdx.x;
      const uint2 ca = *cp;
      *cp = make_uint2(merge_color(ca.x, wa0, v0.c, v0.w, take0, blend0), merge_color(ca.y, wa1, v1.c, v1.w, take1, blend1));
    }
    if (threadIdx.x == 0) st.pend[slot] = 0ull;                               // (st.key[slot] stays)
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
    {
      std::vector<unsigned long long> packed(count);
      for (uint32_t i = 0; i < count; ++i) {
        for (int k = 0; k < 3; ++k) if (!kf_brick_key_in_range(keys[3 * (size_t)i + k])) return KF_ERR_ARG;
        packed[i] = kf_brick_key_pack(keys[3 * (size_t)i], keys[3 * (size_t)i + 1], keys[3 * (size_t)i + 2]);
      }
      if (!kf_brick_keys_unique(packed.data(), packed.size())) return KF_ERR_ARG;
    }
    if (kf_rigid_candidates(count, keys, xf, words) < 0) return KF_ERR_ARG;   // a destination brick outside the key range
    mask = kf_rigid_source_table(count, keys, tkey, tslot);
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
  const bool with_color = color && c->bstore.color;
  const size_t vox = (size_t)count * KF_BRICK_VOX;
  KfResampleTemp tmp;
  float *dt = nullptr, *dw = nullptr, *dfb = nullptr;
  unsigned char* dc = nullptr;
  unsigned long long* dtkey = nullptr;
  unsigned* dtslot = nullptr;
  int32_t *dck = nullptr, *dib = nullptr;
  if (!tmp.get((void**)&dt, vox * sizeof(float)) || !tmp.get((void**)&dw, vox * sizeof(float)) || (with_color && !tmp.get((void**)&dc, vox * 3)) ||
      !tmp.get((void**)&dtkey, tkey.size() * sizeof(unsigned long long)) || !tmp.get((void**)&dtslot, tslot.size() * sizeof(unsigned)) ||
      !tmp.get((void**)&dck, ncand * 3 * sizeof(int32_t)) || !tmp.get((void**)&dib, ncand * 3 * sizeof(int32_t)) || !tmp.get((void**)&dfb, ncand * 3 * sizeof(float)))
    return KF_ERR_ALLOC;                                     // nothing touched
  hipError_t e = hipMemcpyAsync(dt, tsdf, vox * sizeof(float), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dw, weight, vox * sizeof(float), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess && with_color) e = hipMemcpyAsync(dc, color, vox * 3, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dtkey, tkey.data(), tkey.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dtslot, tslot.data(), tslot.size() * sizeof(unsigned), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dck, ckeys.data(), ncand * 3 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dib, cib.data(), ncand * 3 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dfb, cfb.data(), ncand * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    KfBrickStore stab = KfBrickStore{};
    stab.tkey = dtkey; stab.tslot = dtslot; stab.max_bricks = count; stab.mask = mask;
    const KfResampleSource src = {dt, dw, dc};
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
