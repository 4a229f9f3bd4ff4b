// halve.hip -- halving a map's resolution: the incoming map at voxel size s is read through a hash table of its own, every coarse voxel is formed from its
// eight children, and the halved bricks meet the held ones under kf_merge_brick_store's rule (store_merge.h).  No reference counterpart.
// The rule is written out above kf_merge_brick_store_halved in include/hybkf.h; the source table is the rigid merge's (rigid_keys.h).
#include "kf_internal.h"
#include "brick_key.h"
#include "brick_find.h"
#include "store_merge.h"
#include "brick_keys_unique.h"
#include "rigid_keys.h"
#include "resample_shared.h"
#include <stdint.h>
#include <algorithm>
#include <new>
#include <vector>

// one halved voxel; c: the colour packed as the slot holds it (x | y << 8 | z << 16)
struct KfHalved { float t, w; unsigned c; };

// One coarse voxel from its eight children (index dx | dy << 1 | dz << 2): t, w their tsdf and weight (a child whose brick the source does not hold has
// weight 0), cc their colours packed.  An unobserved child adds 0.f to the sum and takes no part in the count, the minimum and the colour.
template <bool COLOR>
__device__ __forceinline__ KfHalved halve_voxel(const float (&t)[8], const float (&w)[8], const unsigned (&cc)[8]) {
  float c[8];
  float wmin = 3.0e38f;
  unsigned n = 0u, sx = 0u, sy = 0u, sz = 0u;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const bool seen = w[k] > 0.f;
    c[k] = seen ? t[k] : 0.f;
    wmin = seen ? fminf(wmin, w[k]) : wmin;
    n += seen ? 1u : 0u;
    if (COLOR) { sx += seen ? (cc[k] & 255u) : 0u; sy += seen ? ((cc[k] >> 8) & 255u) : 0u; sz += seen ? ((cc[k] >> 16) & 255u) : 0u; }
  }
  KfHalved r = {0.f, 0.f, 0u};
  if (n == 0u) return r;
  const float sum = ((c[0] + c[1]) + (c[2] + c[3])) + ((c[4] + c[5]) + (c[6] + c[7]));
  r.t = sum / (float)n; r.w = wmin;
  if (COLOR) r.c = ((2u * sx + n) / (2u * n)) | (((2u * sy + n) / (2u * n)) << 8) | (((2u * sz + n) / (2u * n)) << 16);
  return r;
}

// the four x-adjacent colours of a row, packed one per word, from its 12 bytes (three aligned words: the row starts at a voxel index that is a multiple of 4)
__device__ __forceinline__ void unpack_row_colors(const unsigned char* p, unsigned (&out)[4]) {
  const unsigned* q = reinterpret_cast<const unsigned*>(p);
  const unsigned a = q[0], b = q[1], c = q[2];
  out[0] = a & 0xFFFFFFu;
  out[1] = (a >> 24) | ((b & 0xFFFFu) << 8);
  out[2] = (b >> 16) | ((c & 0xFFu) << 16);
  out[3] = c >> 8;
}

// Halve and merge for kf_merge_brick_store_halved.  One workgroup iteration per coarse brick K of kf_halved_brick_keys' list, 256 lanes x 2 x-adjacent coarse
// voxels (the slot's float4).  Coarse voxel L of the brick covers the fine voxels 16 K + 2 L + d: fine brick 2 K + (L >> 2), in-brick 2 (L & 3) + d.  A lane's
// two coarse voxels (x = 2 px, 2 px + 1) cover four x-adjacent fine voxels of ONE child brick in each of the four rows (dy, dz): an aligned float4 per row and
// plane.  The 8 child slots are looked up once, by the first 8 lanes, into LDS.  After the workgroup-wide "any weight > 0" the path is k_store_merge's from
// its key look-up on.  Coarse keys are unique: no two workgroups meet in a slot.
template <bool COLOR>
__global__ void __launch_bounds__(256) k_store_halve(KfBrickStore st, KfBrickStore stab, KfResampleSource src, unsigned count, const int32_t* __restrict__ ckeys,
                                                     float max_weight) {
  __shared__ unsigned s_src[8];
  __shared__ unsigned s_slot, s_fresh;
  __shared__ unsigned long long s_pend;
  const unsigned px = threadIdx.x & 3u, ly = (threadIdx.x >> 2) & 7u, lz = threadIdx.x >> 5;
  const unsigned child = (px >> 1) | ((ly >> 2) << 1) | ((lz >> 2) << 2);
  const unsigned row0 = (((lz & 3u) << 1) << 6) | (((ly & 3u) << 1) << 3) | ((px & 1u) << 2);   // the row (dy, dz) = (0, 0) in the child brick; +8 per dy, +64 per dz
  for (unsigned e = blockIdx.x; e < count; e += gridDim.x) {
    const int kx = ckeys[3 * e], ky = ckeys[3 * e + 1], kz = ckeys[3 * e + 2];
    if (threadIdx.x < 8u) {                                                   // everybody has read the last iteration's slots: the barriers below
      const int bx = 2 * kx + (int)(threadIdx.x & 1u), by = 2 * ky + (int)((threadIdx.x >> 1) & 1u), bz = 2 * kz + (int)(threadIdx.x >> 2);
      unsigned slot = KF_BRICK_NO_SLOT;                                       // (a brick outside the key range has no key: packed, it would alias another)
      if (kf_brick_key_in_range(bx) && kf_brick_key_in_range(by) && kf_brick_key_in_range(bz)) slot = store_find(stab, kf_brick_key_pack(bx, by, bz));
      s_src[threadIdx.x] = slot;
    }
    __syncthreads();
    const unsigned sslot = s_src[child];
    float t0[8], w0[8], t1[8], w1[8];                                         // the children of the lane's two coarse voxels
    unsigned c0[8], c1[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { t0[k] = t1[k] = 0.f; w0[k] = w1[k] = 0.f; c0[k] = c1[k] = 0u; }
    if (sslot != KF_BRICK_NO_SLOT) {
      const size_t base = (size_t)sslot * KF_BRICK_VOX + row0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {                                           // r = dy | dz << 1
        const size_t o = base + (size_t)(((r & 1) << 3) | ((r >> 1) << 6));
        const float4 tv = *reinterpret_cast<const float4*>(src.tsdf + o), wv = *reinterpret_cast<const float4*>(src.weight + o);
        t0[2 * r] = tv.x; t0[2 * r + 1] = tv.y; t1[2 * r] = tv.z; t1[2 * r + 1] = tv.w;
        w0[2 * r] = wv.x; w0[2 * r + 1] = wv.y; w1[2 * r] = wv.z; w1[2 * r + 1] = wv.w;
        if (COLOR && src.color) {
          unsigned cr[4];
          unpack_row_colors(src.color + 3 * o, cr);
          c0[2 * r] = cr[0]; c0[2 * r + 1] = cr[1]; c1[2 * r] = cr[2]; c1[2 * r + 1] = cr[3];
        }
      }
    }
    const KfHalved v0 = halve_voxel<COLOR>(t0, w0, c0), v1 = halve_voxel<COLOR>(t1, w1, c1);
    if (!__syncthreads_or(v0.w > 0.f || v1.w > 0.f)) continue;                // (workgroup-uniform) halves to nothing: takes no slot, changes no held one
    const unsigned long long key = kf_brick_key_pack(kx, ky, kz);
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

// the coarse bricks of a map as words that sort by (z, y, x), unique; false for a key component outside the key range
static bool halved_words(uint32_t count, const int32_t* keys, std::vector<uint64_t>& words) {
  words.clear();
  words.reserve(count);
  for (uint32_t i = 0; i < count; ++i) {
    const int32_t* k = keys + 3 * (size_t)i;
    for (int j = 0; j < 3; ++j) if (!kf_brick_key_in_range(k[j])) return false;
    words.push_back(kf_rigid_order_word(k[0] >> 1, k[1] >> 1, k[2] >> 1));   // (>> of a negative int32 is the arithmetic shift: -1 -> -1, -3 -> -2)
  }
  std::sort(words.begin(), words.end());
  words.erase(std::unique(words.begin(), words.end()), words.end());
  return true;
}

extern "C" int64_t kf_halved_brick_keys(uint32_t count, const int32_t* keys, int32_t* out_keys, int64_t cap) {
  if ((count && !keys) || (cap > 0 && !out_keys)) return -1;
  try {                                                      // (no exception crosses the C boundary)
    std::vector<uint64_t> words;
    if (!halved_words(count, keys, words)) return -1;
    const int64_t n = (int64_t)words.size();
    for (int64_t i = 0; i < n && i < cap; ++i) kf_rigid_word_key(words[(size_t)i], out_keys + 3 * i);
    return n;
  } catch (const std::bad_alloc&) { return -1; }
}

extern "C" int kf_merge_brick_store_halved(kf_ctx* c, uint32_t count, const int32_t* keys, const float* tsdf, const float* weight, const uint8_t* color) {
  if (!c) return KF_ERR_ARG;
  if (c->vol.bz0 != 0 || c->vol.bz1 != c->vol.nb) return KF_ERR_ARG;       // a z-slab context has no store
  if (!c->bstore.max_bricks) return KF_ERR_STATE;
  if (color && !c->bstore.color) return KF_ERR_STATE;
  if (count == 0) return 0;                                  // nothing to merge: the arrays are not looked at
  if (!keys || !tsdf || !weight) return KF_ERR_ARG;
  if (count > (1u << 30)) return KF_ERR_ALLOC;               // (as kf_merge_brick_store_rigid: the source table's probe counts entries in 32 bits)
  std::vector<unsigned long long> tkey;
  std::vector<unsigned> tslot;
  std::vector<int32_t> ckeys;
  uint32_t mask = 0;
  try {                                                      // (no exception crosses the C boundary)
    std::vector<uint64_t> words;
    if (!halved_words(count, keys, words)) return KF_ERR_ARG;
    {
      std::vector<unsigned long long> packed(count);
      for (uint32_t i = 0; i < count; ++i) packed[i] = kf_brick_key_pack(keys[3 * (size_t)i], keys[3 * (size_t)i + 1], keys[3 * (size_t)i + 2]);
      if (!kf_brick_keys_unique(packed.data(), packed.size())) return KF_ERR_ARG;
    }
    mask = kf_rigid_source_table(count, keys, tkey, tslot);
    ckeys.resize(words.size() * 3);
    for (size_t i = 0; i < words.size(); ++i) kf_rigid_word_key(words[i], ckeys.data() + 3 * i);
  } catch (const std::bad_alloc&) { return KF_ERR_ALLOC; }
  const size_t ncand = ckeys.size() / 3;                     // (1 <= ncand <= count)
  KF_CHECK(hipSetDevice(c->cfg.device));
  const bool with_color = color && c->bstore.color;
  const size_t vox = (size_t)count * KF_BRICK_VOX;
  KfResampleTemp tmp;
  float *dt = nullptr, *dw = nullptr;
  unsigned char* dc = nullptr;
  unsigned long long* dtkey = nullptr;
  unsigned* dtslot = nullptr;
  int32_t* dck = nullptr;
  if (!tmp.get((void**)&dt, vox * sizeof(float)) || !tmp.get((void**)&dw, vox * sizeof(float)) || (with_color && !tmp.get((void**)&dc, vox * 3)) ||
      !tmp.get((void**)&dtkey, tkey.size() * sizeof(unsigned long long)) || !tmp.get((void**)&dtslot, tslot.size() * sizeof(unsigned)) ||
      !tmp.get((void**)&dck, ncand * 3 * sizeof(int32_t)))
    return KF_ERR_ALLOC;                                     // nothing touched
  hipError_t e = hipMemcpyAsync(dt, tsdf, vox * sizeof(float), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dw, weight, vox * sizeof(float), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess && with_color) e = hipMemcpyAsync(dc, color, vox * 3, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dtkey, tkey.data(), tkey.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dtslot, tslot.data(), tslot.size() * sizeof(unsigned), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dck, ckeys.data(), ncand * 3 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    KfBrickStore stab = KfBrickStore{};
    stab.tkey = dtkey; stab.tslot = dtslot; stab.max_bricks = count; stab.mask = mask;
    const KfResampleSource src = {dt, dw, dc};
    const dim3 grid(ncand > 4096u ? 4096u : (unsigned)ncand), block(256);   // store_pass's cap
    if (c->bstore.color) hipLaunchKernelGGL(k_store_halve<true>, grid, block, 0, c->stream, c->bstore, stab, src, (unsigned)ncand, dck, c->vol.max_weight);
    else hipLaunchKernelGGL(k_store_halve<false>, grid, block, 0, c->stream, c->bstore, stab, src, (unsigned)ncand, dck, c->vol.max_weight);
    e = hipGetLastError();
  }
  const hipError_t se = hipStreamSynchronize(c->stream);     // on success and on failure alike: nothing still reads the caller's arrays or the temporaries
  return (int)(e != hipSuccess ? e : se);
}
