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
// nothing, so the table never holds a key without a slot and never fills up: a later look-up of a dropped key misses.  Nothing is ever deleted.
#include "kf_internal.h"
#include "brick_key.h"
#include "brick_find.h"
#include <stdint.h>

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

// one lane per departing brick: the slot the brick is written to, or KF_BRICK_NO_SLOT when the store is full (counted as dropped)
__device__ __forceinline__ unsigned store_claim(const KfBrickStore& st, unsigned long long key) {
  const unsigned known = store_find(st, key);              // (other workgroups insert OTHER keys meanwhile: whether this one is there cannot change)
  if (known != KF_BRICK_NO_SLOT) return known;
  const unsigned slot = atomicAdd(&st.cnt->held, 1u);      // first sight: the next slot.  Once `held` has reached max_bricks every taker fails and undoes
  if (slot >= st.max_bricks) {                             // its own step, so a successful taker always saw the number of successes before it
    atomicSub(&st.cnt->held, 1u);
    atomicAdd(&st.cnt->dropped, 1ull);
    return KF_BRICK_NO_SLOT;
  }
  unsigned h = kf_brick_key_hash(key, st.mask);
  for (unsigned p = 0; p <= st.mask; ++p, h = (h + 1u) & st.mask) {   // at most max_bricks <= (mask + 1) / 2 entries are taken: a free one exists
    if (atomicCAS(&st.tkey[h], KF_BRICK_KEY_EMPTY, key) == KF_BRICK_KEY_EMPTY) { st.tslot[h] = slot; return slot; }
  }
  return KF_BRICK_NO_SLOT;                                 // (not reached)
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
// brick and ORs into the tables exactly as a moved brick does.  The store is only read, but for the count of restored bricks.
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
      v.pend[dst] = st.pend[slot];
      v.flags[dst] = (uint8_t)((obs ? KF_FLAG_OBSERVED : 0u) | (neg ? KF_FLAG_HASNEG : 0u));
      if (neg) {
        atomicOr(&v.negbits[dst >> 5], 1u << (dst & 31));
        kf_mark_macro(v, bx, by, bz);
      }
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

// The bricks that leave under a shift of s bricks (source brick q leaves when q - s lies outside [0, nb) on some axis), as up to three disjoint boxes:
// the x strip in full, the y strip without the x strip, the z strip without both -- departing_boxes' decomposition (shift.hip), on bricks.  Along one
// axis with s > 0 the bricks [0, s) leave, with s < 0 the bricks [nb + s, nb).  The bricks that ENTER (destination brick b enters when b + s lies
// outside) are the ones that would leave under -s.  Returns the number of bricks.
static unsigned brick_boxes(const int s[3], int nb, bool entering, KfBrickBoxes& out) {
  int slo[3], shi[3], klo[3], khi[3];                      // per axis: the strip, and what is left of the axis without it
  for (int k = 0; k < 3; ++k) {
    const int64_t ss = entering ? -(int64_t)s[k] : (int64_t)s[k];
    if (ss > 0) { slo[k] = 0; shi[k] = (int)(ss > nb ? nb : ss); klo[k] = shi[k]; khi[k] = nb; }
    else if (ss < 0) { shi[k] = nb; slo[k] = (int)(nb + ss < 0 ? 0 : nb + ss); klo[k] = 0; khi[k] = slo[k]; }
    else { slo[k] = shi[k] = 0; klo[k] = 0; khi[k] = nb; }
  }
  int n = 0;
  unsigned total = 0;
  for (int k = 0; k < 3; ++k) {
    if (slo[k] >= shi[k]) continue;
    uint64_t vol = 1;
    for (int j = 0; j < 3; ++j) {
      out.lo[n][j] = j < k ? klo[j] : (j == k ? slo[j] : 0);
      out.hi[n][j] = j < k ? khi[j] : (j == k ? shi[j] : nb);
      vol *= out.lo[n][j] < out.hi[n][j] ? (uint64_t)(out.hi[n][j] - out.lo[n][j]) : 0u;
    }
    if (vol == 0) continue;
    total += (unsigned)vol;                                // <= nb^3 <= 2^30 (kf_create: at most 1024 bricks per axis)
    out.end[n++] = total;
  }
  for (int k = n; k < 3; ++k) {
    out.end[k] = total;
    for (int j = 0; j < 3; ++j) { out.lo[k][j] = 0; out.hi[k][j] = 1; }
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
}

extern "C" int kf_brick_store_reserve(kf_ctx* c, uint32_t max_bricks) {
  if (!c) return KF_ERR_ARG;
  if (c->vol.bz0 != 0 || c->vol.bz1 != c->vol.nb) return KF_ERR_ARG;       // a z-slab context cannot shift: nothing would ever use the store
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
