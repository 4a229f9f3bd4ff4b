// brickstore.hip -- the brick store: what the moving volume leaves behind, kept on the device and handed back when the window returns.
// No reference counterpart: the reference's cube never moves (src/HybKinectfu.cpp:51-54), so nothing ever leaves it.
//
// kf_shift_volume (shift.hip) overwrites every brick that leaves the window.  With a store reserved it first copies each OBSERVED departing brick --
// 4 KiB of (tsdf, weight), 2 KiB of colour, the 8-byte deferred-weight word -- into a slot keyed by the brick's world coordinate (brick_key.h), and
// after the move it looks every entering brick up and, on a hit, copies the slot back and restates the brick's flags, its has-negative bit and the
// skip tables as k_shift_bricks does for a brick it moves.  The round trip is a verbatim copy both ways: every bit comes back.
//
// The hash table (KfBrickStore, kf_internal.h) is written by the eviction launch only and read by the restore launch only; stream order separates the
// two, so a look-up never meets a half-made entry.  Inside one eviction launch every key occurs once (the departing boxes are disjoint), hence a
// key is either in the table since an earlier launch -- found by a plain read-only probe, its slot overwritten: the window's copy is the newer one --
// or new: then the brick takes a slot first and claims a table entry second.  A brick that finds no free slot is counted as dropped and claims
// nothing, so the table never holds a key without a slot and never fills up: a later look-up of a dropped key misses.  No kernel here deletes: erase.hip does.
#include "kf_internal.h"
#include "brick_key.h"
#include "brick_find.h"
#include "store_merge.h"
#include "brick_keys_unique.h"
#include "strip_boxes.h"
#include <stdint.h>
#include <new>
#include <vector>

// Up to three disjoint boxes of bricks (half-open), numbered one behind the other: iteration i < end[0] lies in box 0, i < end[1] in box 1, ...
// (end[] of a missing box = the total).  Constant indices only: a by-value kernel argument indexed at run time would be copied to scratch.
struct KfBrickBoxes { int lo[3][3], hi[3][3]; unsigned end[3]; };

__device__ __forceinline__ void box_brick(const KfBrickBoxes& b, unsigned i, int& bx, int& by, int& bz) {
  const int k = i < b.end[0] ? 0 : (i < b.end[1] ? 1 : 2);
  const unsigned j = i - (k == 0 ? 0u : (k == 1 ? b.end[0] : b.end[1]));
  const int lx = k == 0 ? b.lo[0][0] : (k == 1 ? b.lo[1][0] : b.lo[2][0]), hx = k == 0 ? b.hi[0][0] : (k == 1 ? b.hi[1][0] : b.hi[2][0]);
  const int ly = k == 0 ? b.lo[0][1] : (k == 1 ? b.lo[1][1] : b.lo[2][1]), hy = k == 0 ? b.hi[0][1] : (k == 1 ? b.hi[1][1] : b.hi[2][1]);
  const int lz = k == 0 ? b.lo[0][2] : (k == 1 ? b.lo[1][2] : b.lo[2][2]);
  const unsigned ex = (unsigned)(hx - lx), ey = (unsigned)(hy - ly);
  bx = lx + (int)(j % ex); by = ly + (int)((j / ex) % ey); bz = lz + (int)(j / (ex * ey));
}

// Eviction, before anything moves.  One workgroup iteration handles one departing brick of the window, 256 lanes x one float4 (two voxels), for
// colour one uint2 each, as k_shift_bricks does.  A brick with no voxel of weight > 0 takes no slot.  (ox, oy, oz): the window's origin in bricks.
template <bool COLOR>
__global__ void __launch_bounds__(256) k_store_evict(KfVolume v, KfBrickStore st, KfBrickBoxes boxes, unsigned total, int ox, int oy, int oz) {
  __shared__ unsigned s_slot;
  const unsigned nb = (unsigned)v.nb;
  for (unsigned i = blockIdx.x; i < total; i += gridDim.x) {
    int bx, by, bz;
    box_brick(boxes, i, bx, by, bz);
    const size_t src = ((size_t)bz * nb + (size_t)by) * nb + (size_t)bx;
    const float4 q = reinterpret_cast<const float4*>(v.tw + src * KF_BRICK_VOX)[threadIdx.x];
    if (!__syncthreads_or(q.y > 0.f || q.w > 0.f)) continue;                  // (workgroup-uniform) never observed: nothing to keep
    const unsigned long long key = kf_brick_key_pack(ox + bx, oy + by, oz + bz);
    if (threadIdx.x == 0) s_slot = store_claim(st, key);                      // everybody has read the last iteration's slot: the barrier above
    __syncthreads();
    const unsigned slot = s_slot;
    if (slot == KF_BRICK_NO_SLOT) continue;
    reinterpret_cast<float4*>(st.tw + (size_t)slot * KF_BRICK_VOX)[threadIdx.x] = q;
    if (COLOR) reinterpret_cast<uint2*>(st.color + (size_t)slot * KF_BRICK_VOX)[threadIdx.x] = reinterpret_cast<const uint2*>(v.color + src * KF_BRICK_VOX)[threadIdx.x];
    if (threadIdx.x == 0) { st.pend[slot] = v.pend[src]; st.key[slot] = key; }   // the deferred-weight word is flushed: 0, 1 or KF_PEND_SAT per quarter
  }
}

// Restore, after the move.  One workgroup iteration handles one brick that has entered the window: k_shift_bricks has left it never observed (zero
// voxels, zero flags, zero deferred-weight word) and the shift has cleared negbits and the skip tables before the move, so a hit overwrites the
// brick and ORs into the tables exactly as a moved brick does (kf_restate_brick).  The store is only read, but for the count of restored bricks.
template <bool COLOR>
__global__ void __launch_bounds__(256) k_store_restore(KfVolume v, KfBrickStore st, KfBrickBoxes boxes, unsigned total, int ox, int oy, int oz) {
  __shared__ unsigned s_slot[2];                         // double-buffered by iteration: a miss goes on without a second barrier
  const unsigned nb = (unsigned)v.nb;
  unsigned par = 0;
  for (unsigned i = blockIdx.x; i < total; i += gridDim.x, par ^= 1u) {
    int bx, by, bz;
    box_brick(boxes, i, bx, by, bz);
    if (threadIdx.x == 0) s_slot[par] = store_find(st, kf_brick_key_pack(ox + bx, oy + by, oz + bz));
    __syncthreads();
    const unsigned slot = s_slot[par];
    if (slot == KF_BRICK_NO_SLOT) continue;                                   // (workgroup-uniform)
    const size_t dst = ((size_t)bz * nb + (size_t)by) * nb + (size_t)bx;
    const float4 q = reinterpret_cast<const float4*>(st.tw + (size_t)slot * KF_BRICK_VOX)[threadIdx.x];
    reinterpret_cast<float4*>(v.tw + dst * KF_BRICK_VOX)[threadIdx.x] = q;
    if (COLOR) reinterpret_cast<uint2*>(v.color + dst * KF_BRICK_VOX)[threadIdx.x] = reinterpret_cast<const uint2*>(st.color + (size_t)slot * KF_BRICK_VOX)[threadIdx.x];
    const int obs = __syncthreads_or(q.y > 0.f || q.w > 0.f), neg = __syncthreads_or(q.x < 0.f || q.z < 0.f);
    if (threadIdx.x == 0) {
      kf_restate_brick(v, dst, bx, by, bz, st.pend[slot], (obs ? KF_FLAG_OBSERVED : 0u) | (neg ? KF_FLAG_HASNEG : 0u));
      atomicAdd(&st.cnt->restored, 1ull);
    }
  }
}

// entries [first, first + count) for kf_read_brick_store: a workgroup per entry, the weights as kf_download_volume reports them (the deferred-weight word applied)
__global__ void __launch_bounds__(256) k_store_export(KfBrickStore st, unsigned first, unsigned count, float max_weight, int32_t* __restrict__ keys,
                                                      float* __restrict__ tsdf, float* __restrict__ weight, unsigned char* __restrict__ color) {
  for (unsigned e = blockIdx.x; e < count; e += gridDim.x) {
    const size_t slot = (size_t)first + e;
    const unsigned long long pend = st.pend[slot];
    for (unsigned k = threadIdx.x; k < KF_BRICK_VOX; k += 256u) {
      const float2 q = st.tw[slot * KF_BRICK_VOX + k];
      const size_t o = (size_t)e * KF_BRICK_VOX + k;
      if (tsdf) tsdf[o] = q.x;
      if (weight) weight[o] = kf_pend_weight(q.y, (unsigned)(pend >> (16u * (k >> 7))) & 0xFFFFu, max_weight);
      if (color && st.color) { const uchar4 cc = st.color[slot * KF_BRICK_VOX + k]; color[3 * o] = cc.x; color[3 * o + 1] = cc.y; color[3 * o + 2] = cc.z; }
    }
    if (keys && threadIdx.x == 0) { int32_t xyz[3]; kf_brick_key_unpack(st.key[slot], xyz); keys[3 * e] = xyz[0]; keys[3 * e + 1] = xyz[1]; keys[3 * e + 2] = xyz[2]; }
  }
}

// Import for kf_write_brick_store, k_store_export's inverse: staged entries [0, count) in kf_read_brick_store's layout -> slots.  One workgroup iteration
// per entry, each lane two voxels: a float2 of tsdf and a float2 of weight in, one float4 (t, w, t, w) out; for colour six bytes in (three 16-bit loads, the
// staged bytes are 2-byte aligned) and one uint2 out, the fourth byte 0 as kf_upload_volume writes it.  An entry with no weight > 0 takes no slot, as in
// k_store_evict.  The weights are TRUE weights, so the deferred-weight word is 0: nothing is pending on them.  Every key occurs once per launch (the caller
// has checked), so store_claim's reasoning holds: no two workgroups settle the same key.
template <bool COLOR>
__global__ void __launch_bounds__(256) k_store_import(KfBrickStore st, unsigned count, const int32_t* __restrict__ keys, const float* __restrict__ tsdf,
                                                      const float* __restrict__ weight, const unsigned char* __restrict__ color) {
  __shared__ unsigned s_slot;
  for (unsigned e = blockIdx.x; e < count; e += gridDim.x) {
    const size_t o = (size_t)e * KF_BRICK_VOX;
    const float2 t = reinterpret_cast<const float2*>(tsdf + o)[threadIdx.x];
    const float2 w = reinterpret_cast<const float2*>(weight + o)[threadIdx.x];
    if (!__syncthreads_or(w.x > 0.f || w.y > 0.f)) continue;                  // (workgroup-uniform) never observed: nothing to keep
    const unsigned long long key = kf_brick_key_pack(keys[3 * e], keys[3 * e + 1], keys[3 * e + 2]);
    if (threadIdx.x == 0) s_slot = store_claim(st, key);                      // everybody has read the last iteration's slot: the barrier above
    __syncthreads();
    const unsigned slot = s_slot;
    if (slot == KF_BRICK_NO_SLOT) continue;
    reinterpret_cast<float4*>(st.tw + (size_t)slot * KF_BRICK_VOX)[threadIdx.x] = make_float4(t.x, w.x, t.y, w.y);
    if (COLOR) {                                                              // the store has a colour plane; no colour given (kernel-uniform): zeros, never stale bytes
      unsigned c0, c1;
      staged_colors(color, o, c0, c1);
      reinterpret_cast<uint2*>(st.color + (size_t)slot * KF_BRICK_VOX)[threadIdx.x] = make_uint2(c0, c1);
    }
    if (threadIdx.x == 0) { st.pend[slot] = 0ull; st.key[slot] = key; }
  }
}

// Merge for kf_merge_brick_store: k_store_import's shape and staging layout, the keys translated by (ox, oy, oz) bricks; what a lane has loaded -- two voxels
// and, where given, their colours -- meets the store under store_merge_pair (store_merge.h), which k_store_resample_merge and k_store_halve end in too.
template <bool COLOR>
__global__ void __launch_bounds__(256) k_store_merge(KfBrickStore st, unsigned count, const int32_t* __restrict__ keys, const float* __restrict__ tsdf,
                                                     const float* __restrict__ weight, const unsigned char* __restrict__ color, int ox, int oy, int oz,
                                                     float max_weight) {
  __shared__ KfMergeShared sh;
  for (unsigned e = blockIdx.x; e < count; e += gridDim.x) {
    const size_t o = (size_t)e * KF_BRICK_VOX;
    const float2 t = reinterpret_cast<const float2*>(tsdf + o)[threadIdx.x];
    const float2 w = reinterpret_cast<const float2*>(weight + o)[threadIdx.x];
    unsigned cb0 = 0u, cb1 = 0u;                                              // the incoming colours of the lane's two voxels, packed
    if (COLOR) staged_colors(color, o, cb0, cb1);
    const KfIncoming v0 = {t.x, w.x, cb0}, v1 = {t.y, w.y, cb1};
    store_merge_pair<COLOR>(st, kf_brick_key_pack(keys[3 * e] + ox, keys[3 * e + 1] + oy, keys[3 * e + 2] + oz), v0, v1, color != nullptr, max_weight, sh);
  }
}

// The bricks that leave under a shift of s bricks (source brick q leaves when q - s lies outside [0, nb) on some axis), as up to three disjoint boxes:
// the strip rule on bricks (strip_boxes.h, reach 0): along one axis with s > 0 the bricks [0, s) leave, with s < 0 the bricks [nb + s, nb).  The bricks
// that ENTER (destination brick b enters when b + s lies outside) are the ones that would leave under -s.  Returns the number of bricks.
static unsigned brick_boxes(const int s[3], int nb, bool entering, KfBrickBoxes& out) {
  const int64_t sign = entering ? -1 : 1;
  const int n = kf_strip_boxes(sign * s[0], sign * s[1], sign * s[2], nb, 0, out.lo, out.hi);
  unsigned total = 0;
  for (int k = 0; k < 3; ++k) {
    if (k < n) total += (unsigned)(out.hi[k][0] - out.lo[k][0]) * (unsigned)(out.hi[k][1] - out.lo[k][1]) * (unsigned)(out.hi[k][2] - out.lo[k][2]);   // <= nb^3 <= 2^30
    else for (int j = 0; j < 3; ++j) { out.lo[k][j] = 0; out.hi[k][j] = 1; }                                                  // (kf_create: at most 1024 bricks per axis)
    out.end[k] = total;
  }
  return total;
}

static int store_pass(kf_ctx* c, const int s[3], const int32_t origin_vox[3], bool restore) {
  KfBrickBoxes boxes;
  const unsigned total = brick_boxes(s, c->vol.nb, restore, boxes);
  if (total == 0) return 0;
  const dim3 grid(total > 4096u ? 4096u : total), block(256);
  const int ox = origin_vox[0] / KF_BRICK, oy = origin_vox[1] / KF_BRICK, oz = origin_vox[2] / KF_BRICK;   // exact: the origin is a sum of whole bricks
  if (restore) {
    if (c->vol.color) hipLaunchKernelGGL(k_store_restore<true>, grid, block, 0, c->stream, c->vol, c->bstore, boxes, total, ox, oy, oz);
    else hipLaunchKernelGGL(k_store_restore<false>, grid, block, 0, c->stream, c->vol, c->bstore, boxes, total, ox, oy, oz);
  } else {
    if (c->vol.color) hipLaunchKernelGGL(k_store_evict<true>, grid, block, 0, c->stream, c->vol, c->bstore, boxes, total, ox, oy, oz);
    else hipLaunchKernelGGL(k_store_evict<false>, grid, block, 0, c->stream, c->vol, c->bstore, boxes, total, ox, oy, oz);
  }
  return (int)hipGetLastError();
}
int kf_brick_store_evict(kf_ctx* c, const int s[3], const int32_t origin_vox[3]) { return store_pass(c, s, origin_vox, false); }
int kf_brick_store_restore(kf_ctx* c, const int s[3], const int32_t origin_vox[3]) { return store_pass(c, s, origin_vox, true); }

int kf_brick_store_reset(kf_ctx* c) {
  KfBrickStore& st = c->bstore;
  KF_CHECK(hipMemsetAsync(st.tkey, 0xFF, ((size_t)st.mask + 1) * sizeof(unsigned long long), c->stream));   // every entry KF_BRICK_KEY_EMPTY
  KF_CHECK(hipMemsetAsync(st.cnt, 0, sizeof(KfBrickStoreCounts), c->stream));
  return 0;
}
void kf_brick_store_free(kf_ctx* c) {
  KfBrickStore& st = c->bstore;
  void* ptrs[] = {st.tw, st.color, st.pend, st.key, st.tkey, st.tslot, st.cnt};
  for (void* p : ptrs) if (p) hipFree(p);
  st = KfBrickStore{};
  if (c->bstore_stage) { hipFree(c->bstore_stage); c->bstore_stage = nullptr; }
}

extern "C" int kf_brick_store_reserve(kf_ctx* c, uint32_t max_bricks) {
  if (!c) return KF_ERR_ARG;
  if (!kf_whole_volume(c)) return KF_ERR_ARG;       // a z-slab context cannot shift: nothing would ever use the store
  KF_CHECK(hipSetDevice(c->cfg.device));
  KF_CHECK(hipStreamSynchronize(c->stream));                 // whatever still reads or writes the old store
  kf_brick_store_free(c);
  if (max_bricks == 0) return 0;
  uint64_t cap = 2;
  while (cap < 2ull * max_bricks) cap <<= 1;                 // the next power of two >= 2 * max_bricks
  if (cap > (1ull << 31)) return KF_ERR_ALLOC;              // (the probe loops count entries in 32 bits; 2^30 bricks would be 4 TiB anyway)
  KfBrickStore st = KfBrickStore{};
  hipError_t e = hipMalloc((void**)&st.tw, (size_t)max_bricks * KF_BRICK_VOX * sizeof(float2));
  if (e == hipSuccess && c->vol.color) e = hipMalloc((void**)&st.color, (size_t)max_bricks * KF_BRICK_VOX * sizeof(uchar4));
  if (e == hipSuccess) e = hipMalloc((void**)&st.pend, (size_t)max_bricks * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMalloc((void**)&st.key, (size_t)max_bricks * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMalloc((void**)&st.tkey, (size_t)cap * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMalloc((void**)&st.tslot, (size_t)cap * sizeof(unsigned));
  if (e == hipSuccess) e = hipMalloc((void**)&st.cnt, sizeof(KfBrickStoreCounts));
  c->bstore = st;
  if (e != hipSuccess) { kf_brick_store_free(c); (void)hipGetLastError(); return KF_ERR_ALLOC; }
  c->bstore.max_bricks = max_bricks; c->bstore.mask = (unsigned)(cap - 1);
  const int rs = kf_brick_store_reset(c);
  if (rs) { kf_brick_store_free(c); return rs; }
  KF_CHECK(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int kf_brick_store_clear(kf_ctx* c) {
  if (!c) return KF_ERR_ARG;
  if (!c->bstore.max_bricks) return KF_ERR_STATE;
  return kf_brick_store_reset(c);
}

extern "C" int kf_brick_store_count(kf_ctx* c, uint32_t* held, uint64_t* dropped, uint64_t* restored) {
  if (!c) return KF_ERR_ARG;
  if (held) *held = 0;
  if (dropped) *dropped = 0;
  if (restored) *restored = 0;
  if (!c->bstore.max_bricks) return 0;
  KF_CHECK(hipMemcpyAsync(c->host_pinned, c->bstore.cnt, sizeof(KfBrickStoreCounts), hipMemcpyDeviceToHost, c->stream));
  KF_CHECK(hipStreamSynchronize(c->stream));
  const KfBrickStoreCounts* h = (const KfBrickStoreCounts*)c->host_pinned;
  if (held) *held = h->held;
  if (dropped) *dropped = h->dropped;
  if (restored) *restored = h->restored;
  return 0;
}

extern "C" int kf_read_brick_store(kf_ctx* c, uint32_t first, uint32_t count, int32_t* keys, float* tsdf, float* weight, uint8_t* color) {
  if (!c) return KF_ERR_ARG;
  uint32_t held = 0;
  { const int cs = kf_brick_store_count(c, &held, nullptr, nullptr); if (cs) return cs; }
  if ((uint64_t)first + count > held) return KF_ERR_ARG;
  if (count == 0) return 0;
  const size_t n = (size_t)count * KF_BRICK_VOX;
  const bool with_color = color && c->bstore.color;
  int32_t* dk = nullptr; float *dt = nullptr, *dw = nullptr; unsigned char* dc = nullptr;
  hipError_t e = hipSuccess;
  if (keys) e = hipMalloc((void**)&dk, (size_t)count * 3 * sizeof(int32_t));
  if (e == hipSuccess && tsdf) e = hipMalloc((void**)&dt, n * sizeof(float));
  if (e == hipSuccess && weight) e = hipMalloc((void**)&dw, n * sizeof(float));
  if (e == hipSuccess && with_color) e = hipMalloc((void**)&dc, n * 3);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_store_export, dim3(count > 4096u ? 4096u : count), dim3(256), 0, c->stream, c->bstore, first, count, c->vol.max_weight, dk, dt, dw, dc);
    if (dk) e = hipMemcpyAsync(keys, dk, (size_t)count * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && dt) e = hipMemcpyAsync(tsdf, dt, n * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && dw) e = hipMemcpyAsync(weight, dw, n * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && dc) e = hipMemcpyAsync(color, dc, n * 3, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  } else (void)hipGetLastError();
  if (dk) hipFree(dk);
  if (dt) hipFree(dt);
  if (dw) hipFree(dw);
  if (dc) hipFree(dc);
  return e == hipSuccess ? 0 : (int)e;
}

// Capture: every observed brick of the window into the store, under the window's origin -- the eviction of a shift that makes everything leave (one box of
// all nb^3 bricks), without the shift.  Pending weights are flushed first, as the shift does, so the slots hold what a departing brick would have held.
int kf_brick_store_capture_enqueue(kf_ctx* c) {
  { const int fs = kf_flush_pending(c); if (fs) return fs; }
  const int all[3] = {c->vol.nb, 0, 0};
  return kf_brick_store_evict(c, all, c->origin_vox);
}
extern "C" int kf_brick_store_capture(kf_ctx* c) {
  if (!c) return KF_ERR_ARG;
  if (!kf_whole_volume(c)) return KF_ERR_ARG;
  if (!c->bstore.max_bricks) return KF_ERR_STATE;
  if (!kf_window_in_key_range(c->origin_vox, c->vol.nb)) return KF_ERR_ARG;   // (a window that shifts with a store reserved never leaves the key range; one that moved before the reserve may have)
  KF_CHECK(hipSetDevice(c->cfg.device));
  return kf_brick_store_capture_enqueue(c);
}

// kf_write_brick_store: the staging buffer holds KF_BSTORE_STAGE_BRICKS entries, plane after plane -- keys, tsdf, weight, colour bytes -- each plane 16-byte aligned
#define KF_BSTORE_STAGE_BRICKS 256u
// kf_write_brick_store and kf_merge_brick_store: the checks, the staging and the chunked launches are one path.  off == nullptr: a write (the keys as they
// are, k_store_import); else a merge (the keys translated by off, whole bricks, k_store_merge).  Refused before anything is touched.
static int store_put(kf_ctx* c, uint32_t count, const int32_t* keys, const float* tsdf, const float* weight, const uint8_t* color, const int32_t* off) {
  if (!c) return KF_ERR_ARG;
  if (!c->bstore.max_bricks) return KF_ERR_STATE;
  if (color && !c->bstore.color) return KF_ERR_STATE;
  if (count == 0) return 0;                                  // nothing to write: the arrays are not looked at
  if (!keys || !tsdf || !weight) return KF_ERR_ARG;
  try {                                                      // (no exception crosses the C boundary)
    std::vector<unsigned long long> packed(count);
    for (uint32_t i = 0; i < count; ++i) {
      int32_t k3[3];
      for (int k = 0; k < 3; ++k) {
        const int64_t t = (int64_t)keys[3 * (size_t)i + k] + (off ? off[k] : 0);   // (64 bits: the sum of two int32 cannot overflow)
        if (!kf_brick_key_in_range(t)) return KF_ERR_ARG;
        k3[k] = (int32_t)t;
      }
      packed[i] = kf_brick_key_pack(k3[0], k3[1], k3[2]);
    }
    if (!kf_brick_keys_unique(packed.data(), packed.size())) return KF_ERR_ARG;
  } catch (const std::bad_alloc&) { return KF_ERR_ALLOC; }
  KF_CHECK(hipSetDevice(c->cfg.device));
  const size_t cap = KF_BSTORE_STAGE_BRICKS, plane = cap * KF_BRICK_VOX * sizeof(float);
  const size_t off_t = cap * 3 * sizeof(int32_t), off_w = off_t + plane, off_c = off_w + plane, bytes = off_c + cap * KF_BRICK_VOX * 3;
  if (!c->bstore_stage && hipMalloc(&c->bstore_stage, bytes) != hipSuccess) { c->bstore_stage = nullptr; (void)hipGetLastError(); return KF_ERR_ALLOC; }
  unsigned char* base = (unsigned char*)c->bstore_stage;
  int32_t* dk = (int32_t*)base; float *dt = (float*)(base + off_t), *dw = (float*)(base + off_w); unsigned char* dc = base + off_c;
  const bool with_color = color && c->bstore.color;
  const unsigned char* kc = with_color ? dc : (unsigned char*)nullptr;
  hipError_t e = hipSuccess;
  for (uint32_t first = 0; first < count && e == hipSuccess; first += KF_BSTORE_STAGE_BRICKS) {   // stream order: a chunk's launch has read the buffer before the next chunk's copies write it
    const uint32_t n = count - first < KF_BSTORE_STAGE_BRICKS ? count - first : KF_BSTORE_STAGE_BRICKS;
    const size_t vox = (size_t)n * KF_BRICK_VOX, at = (size_t)first * KF_BRICK_VOX;
    e = hipMemcpyAsync(dk, keys + 3 * (size_t)first, (size_t)n * 3 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dt, tsdf + at, vox * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dw, weight + at, vox * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && with_color) e = hipMemcpyAsync(dc, color + 3 * at, vox * 3, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) break;
    const dim3 grid(n), block(256);                          // n <= KF_BSTORE_STAGE_BRICKS: below store_pass's cap of 4096 workgroups
    if (!off) {                                              // (k_store_import is named first: instantiations are emitted in this order, and its listing stays what it was)
      if (c->bstore.color) hipLaunchKernelGGL(k_store_import<true>, grid, block, 0, c->stream, c->bstore, n, dk, dt, dw, kc);
      else hipLaunchKernelGGL(k_store_import<false>, grid, block, 0, c->stream, c->bstore, n, dk, dt, dw, (unsigned char*)nullptr);
    } else {
      if (c->bstore.color) hipLaunchKernelGGL(k_store_merge<true>, grid, block, 0, c->stream, c->bstore, n, dk, dt, dw, kc, (int)off[0], (int)off[1], (int)off[2], c->vol.max_weight);
      else hipLaunchKernelGGL(k_store_merge<false>, grid, block, 0, c->stream, c->bstore, n, dk, dt, dw, (unsigned char*)nullptr, (int)off[0], (int)off[1], (int)off[2], c->vol.max_weight);
    }
    e = hipGetLastError();
  }
  const hipError_t se = hipStreamSynchronize(c->stream);     // on success and on failure alike: no copy out of the caller's arrays is still queued when the call returns
  return (int)(e != hipSuccess ? e : se);
}
extern "C" int kf_write_brick_store(kf_ctx* c, uint32_t count, const int32_t* keys, const float* tsdf, const float* weight, const uint8_t* color) {
  return store_put(c, count, keys, tsdf, weight, color, nullptr);
}
extern "C" int kf_merge_brick_store(kf_ctx* c, uint32_t count, const int32_t* keys, const float* tsdf, const float* weight, const uint8_t* color,
                                    const int32_t offset_brick[3]) {
  static const int32_t zero[3] = {0, 0, 0};
  return store_put(c, count, keys, tsdf, weight, color, offset_brick ? offset_brick : zero);
}
