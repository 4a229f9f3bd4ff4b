// halve.hip -- halving a map's resolution: the incoming map at voxel size s is read through a hash table of its own, every coarse voxel is formed from its
// eight children, and the halved bricks meet the held ones under kf_merge_brick_store's rule (store_merge.h: store_merge_pair).  No reference counterpart.
// The rule is written out above kf_merge_brick_store_halved in include/hybkf.h; the source keys' check and table (rigid_keys.h: kf_source_keys_table) and
// the upload (resample_shared.h: kf_source_map_upload) are the rigid merge's.
#include "kf_internal.h"
#include "brick_key.h"
#include "brick_find.h"
#include "store_merge.h"
#include "rigid_keys.h"
#include "resample_shared.h"
#include <stdint.h>
#include <algorithm>
#include <new>
#include <vector>

// One coarse voxel from its eight children (index dx | dy << 1 | dz << 2): t, w their tsdf and weight (a child whose brick the source does not hold has
// weight 0), cc their colours packed.  An unobserved child adds 0.f to the sum and takes no part in the count, the minimum and the colour.
template <bool COLOR>
__device__ __forceinline__ KfIncoming halve_voxel(const float (&t)[8], const float (&w)[8], const unsigned (&cc)[8]) {
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
  KfIncoming r = {0.f, 0.f, 0u};
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
// plane.  The 8 child slots are looked up once, by the first 8 lanes, into LDS.  What the lanes halve meets the store under store_merge_pair.  Coarse keys
// are unique: no two workgroups meet in a slot.
template <bool COLOR>
__global__ void __launch_bounds__(256) k_store_halve(KfBrickStore st, KfBrickStore stab, KfResampleSource src, unsigned count, const int32_t* __restrict__ ckeys,
                                                     float max_weight) {
  __shared__ unsigned s_src[8];
  __shared__ KfMergeShared sh;
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
    const KfIncoming v0 = halve_voxel<COLOR>(t0, w0, c0), v1 = halve_voxel<COLOR>(t1, w1, c1);
    store_merge_pair<COLOR>(st, kf_brick_key_pack(kx, ky, kz), v0, v1, src.color != nullptr, max_weight, sh);
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
  if (!kf_whole_volume(c)) return KF_ERR_ARG;       // a z-slab context has no store
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
    if (!kf_source_keys_table(count, keys, tkey, tslot, mask)) return KF_ERR_ARG;
    ckeys.resize(words.size() * 3);
    for (size_t i = 0; i < words.size(); ++i) kf_rigid_word_key(words[i], ckeys.data() + 3 * i);
  } catch (const std::bad_alloc&) { return KF_ERR_ALLOC; }
  const size_t ncand = ckeys.size() / 3;                     // (1 <= ncand <= count)
  KF_CHECK(hipSetDevice(c->cfg.device));
  KfResampleTemp tmp;
  int32_t* dck = nullptr;
  KfBrickStore stab;
  KfResampleSource src;
  hipError_t e;
  if (!tmp.get((void**)&dck, ncand * 3 * sizeof(int32_t)) || !kf_source_map_upload(c, tmp, count, tsdf, weight, color, tkey, tslot, mask, stab, src, e))
    return KF_ERR_ALLOC;                                     // nothing touched  (a colour without a colour plane was refused above)
  if (e == hipSuccess) e = hipMemcpyAsync(dck, ckeys.data(), ncand * 3 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    const dim3 grid(ncand > 4096u ? 4096u : (unsigned)ncand), block(256);   // store_pass's cap
    if (c->bstore.color) hipLaunchKernelGGL(k_store_halve<true>, grid, block, 0, c->stream, c->bstore, stab, src, (unsigned)ncand, dck, c->vol.max_weight);
    else hipLaunchKernelGGL(k_store_halve<false>, grid, block, 0, c->stream, c->bstore, stab, src, (unsigned)ncand, dck, c->vol.max_weight);
    e = hipGetLastError();
  }
  const hipError_t se = hipStreamSynchronize(c->stream);     // on success and on failure alike: nothing still reads the caller's arrays or the temporaries
  return (int)(e != hipSuccess ? e : se);
}
