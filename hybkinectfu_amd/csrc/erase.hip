// erase.hip -- erasing from the map: a box of voxels cleared in the brick store (or everything but the box), weakly observed bricks thrown out, the
// emptied bricks dropped and their slots handed back.  No reference counterpart: the reference's cube never forgets.
// The contract is written out above kf_brick_store_erase_box in include/hybkf.h, the argument in DESIGN.md 4e-7.
//
// Every other kernel of the store relies on three things: slots [0, held) are the entries, every held key is found by a probe that ends at the first
// free table entry, and store_claim hands out slot `held`.  So a removal may neither leave a gap in [0, held) nor empty a table entry in place (that would
// cut the probe chains running through it).  The erase therefore works in launches chained by stream order -- no launch reads what another lane of the
// SAME launch has stored, and every loop is bounded by data read at its start:
//   1. mark:    one workgroup iteration per held slot decides keep[slot] (and, for a brick the box cuts, clears the voxels and zeroes the word);
//   2. scan:    keep[] becomes its exclusive prefix, keep[held] = M, the number of bricks kept (scan.h);
//   3. holes:   the removed slots below M, listed by rank;  4. move: the r-th kept slot at or above M goes into the r-th hole.  There are as many of one
//               as of the other, sources lie at >= M and destinations below M: no copy of the store is needed and no two workgroups meet in a slot;
//   5. rebuild: the table is emptied and every slot below M claims an entry as store_claim claims one; then held = M.
#include "kf_internal.h"
#include "brick_key.h"
#include "erase_box.h"
#include "scan.h"
#include <stdint.h>
#include <math.h>

static_assert(KF_ERASE_INSIDE == KF_ERASE_BOX_INSIDE && KF_ERASE_OUTSIDE == KF_ERASE_BOX_OUTSIDE, "erase_box.h restates the public modes");

// what the call returns, on the device: zeroed before the mark pass, read once at the end
struct KfEraseResult { unsigned long long cleared; unsigned kept, pad_; };

// the workgroup's count of cleared observed voxels, one atomic add: `wave_n` is wave-uniform (sums of ballot counts)
__device__ __forceinline__ void erase_add_cleared(unsigned wave_n, unsigned long long* cleared) {
  __shared__ unsigned s_n[4];
  if ((threadIdx.x & 63u) == 0u) s_n[threadIdx.x >> 6] = wave_n;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long n = (unsigned long long)s_n[0] + s_n[1] + s_n[2] + s_n[3];
    if (n) atomicAdd(cleared, n);
  }
}

// Mark and clear for kf_brick_store_erase_box.  One workgroup iteration per held slot, 256 lanes x one float4 (voxels 2t and 2t + 1) and one uint2 of
// colour, as the other store kernels.  The brick's class comes from its key (workgroup-uniform).  Untouched: nothing is read but the key.  Removed and cut:
// the TRUE weights (the slot's deferred-weight word applied, as k_store_export applies it) say which cleared voxels were observed and whether anything is
// left.  A cut brick that keeps something is written back: cleared voxels (+0, +0) and colour 0 0 0 0, the others with their true weight, the word 0 --
// thread 0 is the only one to write the word, every lane has its copy from before the barrier.
template <bool COLOR>
__global__ void __launch_bounds__(256) k_store_erase_mark(KfBrickStore st, unsigned held, KfEraseBox box, int mode, float max_weight, unsigned* __restrict__ keep,
                                                          unsigned long long* __restrict__ cleared) {
  const unsigned k0 = 2u * threadIdx.x;                                       // the lane's first voxel: x = k0 & 7 (even), y, z shared by both
  const int vx = (int)(k0 & 7u), vy = (int)((k0 >> 3) & 7u), vz = (int)(k0 >> 6);
  unsigned wave_n = 0u;
  for (unsigned slot = blockIdx.x; slot < held; slot += gridDim.x) {
    int32_t key[3];
    kf_brick_key_unpack(st.key[slot], key);
    const int cls = kf_erase_brick_class(box, mode, key[0], key[1], key[2]);  // (workgroup-uniform)
    if (cls == KF_BRICK_UNTOUCHED) { if (threadIdx.x == 0) keep[slot] = 1u; continue; }
    float4* tw = reinterpret_cast<float4*>(st.tw + (size_t)slot * KF_BRICK_VOX) + threadIdx.x;
    const float4 q = *tw;
    const unsigned pq = (unsigned)(st.pend[slot] >> (16u * (threadIdx.x >> 6))) & 0xFFFFu;   // (wave-uniform)
    const float w0 = kf_pend_weight(q.y, pq, max_weight), w1 = kf_pend_weight(q.w, pq, max_weight);
    const int gx = 8 * key[0] + vx, gy = 8 * key[1] + vy, gz = 8 * key[2] + vz;
    const bool c0 = cls == KF_BRICK_REMOVED || kf_erase_voxel_cleared(box, mode, gx, gy, gz);
    const bool c1 = cls == KF_BRICK_REMOVED || kf_erase_voxel_cleared(box, mode, gx + 1, gy, gz);
    wave_n += (unsigned)__popcll(__ballot(c0 && w0 > 0.f)) + (unsigned)__popcll(__ballot(c1 && w1 > 0.f));
    const int left = __syncthreads_or((!c0 && w0 > 0.f) || (!c1 && w1 > 0.f));   // the barrier: every lane has read the word
    if (threadIdx.x == 0) keep[slot] = left ? 1u : 0u;
    if (!left) continue;                                                       // (workgroup-uniform) removed: the slot's bytes no longer matter
    *tw = make_float4(c0 ? 0.f : q.x, c0 ? 0.f : w0, c1 ? 0.f : q.z, c1 ? 0.f : w1);
    if (COLOR) {
      uint2* cp = reinterpret_cast<uint2*>(st.color + (size_t)slot * KF_BRICK_VOX) + threadIdx.x;
      const uint2 cc = *cp;
      *cp = make_uint2(c0 ? 0u : cc.x, c1 ? 0u : cc.y);
    }
    if (threadIdx.x == 0) st.pend[slot] = 0ull;
  }
  erase_add_cleared(wave_n, cleared);
}

// Mark for kf_brick_store_erase_weak: a brick stays when some voxel's TRUE weight reaches min_weight.  Nothing is written but keep[].
__global__ void __launch_bounds__(256) k_store_weak_mark(KfBrickStore st, unsigned held, float min_weight, float max_weight, unsigned* __restrict__ keep) {
  for (unsigned slot = blockIdx.x; slot < held; slot += gridDim.x) {
    const float4 q = reinterpret_cast<const float4*>(st.tw + (size_t)slot * KF_BRICK_VOX)[threadIdx.x];
    const unsigned pq = (unsigned)(st.pend[slot] >> (16u * (threadIdx.x >> 6))) & 0xFFFFu;   // (wave-uniform)
    const float w = fmaxf(kf_pend_weight(q.y, pq, max_weight), kf_pend_weight(q.w, pq, max_weight));
    const int stays = __syncthreads_or(w >= min_weight);
    if (threadIdx.x == 0) keep[slot] = stays ? 1u : 0u;
  }
}

// After the scan: keep[i] = kept slots before i, keep[held] = M; slot i was kept iff keep[i + 1] != keep[i].
// The holes -- removed slots below M -- by rank: the hole at i has i - keep[i] holes before it.  One lane per slot.
__global__ void __launch_bounds__(256) k_store_erase_holes(const unsigned* __restrict__ keep, unsigned held, unsigned* __restrict__ holes) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  const unsigned M = keep[held];
  if (i >= M || i >= held) return;
  const unsigned before = keep[i];
  if (keep[i + 1] == before) holes[i - before] = i;
}

// The movers -- kept slots at or above M -- by rank: the mover at j has keep[j] - keep[M] movers before it, and goes into the hole of that rank.  One
// workgroup iteration per slot of [M, held): 4 KiB of pairs, 2 KiB of colour, the word and the key.  Sources lie at >= M, destinations below M.
template <bool COLOR>
__global__ void __launch_bounds__(256) k_store_erase_move(KfBrickStore st, const unsigned* __restrict__ keep, unsigned held, const unsigned* __restrict__ holes) {
  const unsigned M = keep[held];
  if (M >= held) return;                                                       // nothing was removed
  const unsigned base = keep[M];
  for (unsigned j = M + blockIdx.x; j < held; j += gridDim.x) {
    const unsigned before = keep[j];
    if (keep[j + 1] == before) continue;                                       // (workgroup-uniform) a removed slot
    const unsigned dst = holes[before - base];
    reinterpret_cast<float4*>(st.tw + (size_t)dst * KF_BRICK_VOX)[threadIdx.x] = reinterpret_cast<const float4*>(st.tw + (size_t)j * KF_BRICK_VOX)[threadIdx.x];
    if (COLOR) reinterpret_cast<uint2*>(st.color + (size_t)dst * KF_BRICK_VOX)[threadIdx.x] = reinterpret_cast<const uint2*>(st.color + (size_t)j * KF_BRICK_VOX)[threadIdx.x];
    if (threadIdx.x == 0) { st.pend[dst] = st.pend[j]; st.key[dst] = st.key[j]; }
  }
}

// The table has been emptied by the launch before.  One lane per kept slot claims an entry: store_claim's 64-bit compare-and-swap probe, then the slot.
// All keys are distinct and look-ups happen in later launches only -- the condition the eviction relies on.  Lane 0 states the new count.
__global__ void __launch_bounds__(256) k_store_erase_rebuild(KfBrickStore st, const unsigned* __restrict__ keep, unsigned held) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  const unsigned M = keep[held];
  if (i == 0) st.cnt->held = M;
  if (i >= M) return;
  const unsigned long long key = st.key[i];
  unsigned h = kf_brick_key_hash(key, st.mask);
  for (unsigned p = 0; p <= st.mask; ++p, h = (h + 1u) & st.mask) {          // at most max_bricks <= (mask + 1) / 2 entries are taken: a free one exists
    if (atomicCAS(&st.tkey[h], KF_BRICK_KEY_EMPTY, key) == KF_BRICK_KEY_EMPTY) { st.tslot[h] = i; return; }
  }
}

// the context's scratch for a store of max_bricks slots, in 32-bit words: the result (4), keep[] and its total (max_bricks + 1, padded to whole 16-byte
// vectors), the holes (max_bricks), the scan's chunk sums
struct EraseScratch { KfEraseResult* res; unsigned *keep, *holes, *partials; };
static int erase_scratch(kf_ctx* c, EraseScratch& s) {
  const size_t n = c->bstore.max_bricks;
  const size_t keep_words = (n + 1 + 3) & ~(size_t)3, chunks = (n + KF_SCAN_CHUNK - 1) / KF_SCAN_CHUNK;
  if (c->erase_scratch && c->erase_scratch_bricks != c->bstore.max_bricks) {  // the store was reserved anew at another size since
    KF_CHECK(hipStreamSynchronize(c->stream));
    hipFree(c->erase_scratch);
    c->erase_scratch = nullptr;
  }
  if (!c->erase_scratch) {
    if (hipMalloc(&c->erase_scratch, (4 + keep_words + n + chunks) * sizeof(unsigned)) != hipSuccess) { c->erase_scratch = nullptr; (void)hipGetLastError(); return KF_ERR_ALLOC; }
    c->erase_scratch_bricks = c->bstore.max_bricks;
  }
  unsigned* w = (unsigned*)c->erase_scratch;
  s.res = (KfEraseResult*)w; s.keep = w + 4; s.holes = s.keep + keep_words; s.partials = s.holes + n;
  return 0;
}
void kf_erase_scratch_free(kf_ctx* c) {
  if (c->erase_scratch) { hipFree(c->erase_scratch); c->erase_scratch = nullptr; }
  c->erase_scratch_bricks = 0;
}

static inline unsigned erase_grid(unsigned n) { return n > 4096u ? 4096u : n; }   // store_pass's cap

// both entry points: the count read once, the mark pass (box: a box erase; else a weak one), launches 2-5, the result read once
static int erase_run(kf_ctx* c, const KfEraseBox* box, int mode, float min_weight, uint32_t* bricks_removed, uint64_t* voxels_cleared) {
  if (bricks_removed) *bricks_removed = 0;
  if (voxels_cleared) *voxels_cleared = 0;
  KF_CHECK(hipSetDevice(c->cfg.device));
  uint32_t held = 0;
  { const int cs = kf_brick_store_count(c, &held, nullptr, nullptr); if (cs) return cs; }   // blocks: sizes the launches
  if (held == 0) return 0;
  EraseScratch s;
  { const int as = erase_scratch(c, s); if (as) return as; }
  const KfBrickStore& st = c->bstore;
  const dim3 block(256), per_brick(erase_grid(held)), per_lane((held + 255u) / 256u);
  KF_CHECK(hipMemsetAsync(s.res, 0, sizeof(KfEraseResult), c->stream));
  if (box) {
    if (st.color) hipLaunchKernelGGL(k_store_erase_mark<true>, per_brick, block, 0, c->stream, st, held, *box, mode, c->vol.max_weight, s.keep, &s.res->cleared);
    else hipLaunchKernelGGL(k_store_erase_mark<false>, per_brick, block, 0, c->stream, st, held, *box, mode, c->vol.max_weight, s.keep, &s.res->cleared);
  } else hipLaunchKernelGGL(k_store_weak_mark, per_brick, block, 0, c->stream, st, held, min_weight, c->vol.max_weight, s.keep);
  kf_scan_in_place(s.keep, held, s.partials, &s.res->kept, c->stream);
  hipLaunchKernelGGL(k_store_erase_holes, per_lane, block, 0, c->stream, s.keep, held, s.holes);
  if (st.color) hipLaunchKernelGGL(k_store_erase_move<true>, per_brick, block, 0, c->stream, st, s.keep, held, s.holes);
  else hipLaunchKernelGGL(k_store_erase_move<false>, per_brick, block, 0, c->stream, st, s.keep, held, s.holes);
  KF_CHECK(hipGetLastError());
  KF_CHECK(hipMemsetAsync(st.tkey, 0xFF, ((size_t)st.mask + 1) * sizeof(unsigned long long), c->stream));   // every entry KF_BRICK_KEY_EMPTY
  hipLaunchKernelGGL(k_store_erase_rebuild, per_lane, block, 0, c->stream, st, s.keep, held);
  KF_CHECK(hipGetLastError());
  KF_CHECK(hipMemcpyAsync(c->host_pinned, s.res, sizeof(KfEraseResult), hipMemcpyDeviceToHost, c->stream));
  KF_CHECK(hipStreamSynchronize(c->stream));
  const KfEraseResult* r = (const KfEraseResult*)c->host_pinned;
  if (bricks_removed) *bricks_removed = held - r->kept;
  if (voxels_cleared) *voxels_cleared = r->cleared;
  return 0;
}

extern "C" int kf_brick_store_erase_box(kf_ctx* c, const int32_t lo_vox[3], const int32_t hi_vox[3], int mode, uint32_t* bricks_removed, uint64_t* voxels_cleared) {
  if (!c || !lo_vox || !hi_vox || (mode != KF_ERASE_INSIDE && mode != KF_ERASE_OUTSIDE)) return KF_ERR_ARG;
  if (!kf_whole_volume(c)) return KF_ERR_ARG;       // a z-slab context has no store
  if (!c->bstore.max_bricks) return KF_ERR_STATE;
  const KfEraseBox box = kf_erase_box_clamped(lo_vox, hi_vox);
  return erase_run(c, &box, mode, 0.f, bricks_removed, voxels_cleared);
}

extern "C" int kf_brick_store_erase_weak(kf_ctx* c, float min_weight, uint32_t* bricks_removed) {
  if (!c || isnan(min_weight)) return KF_ERR_ARG;
  if (!kf_whole_volume(c)) return KF_ERR_ARG;       // a z-slab context has no store
  if (!c->bstore.max_bricks) return KF_ERR_STATE;
  return erase_run(c, nullptr, 0, min_weight, bricks_removed, nullptr);
}
