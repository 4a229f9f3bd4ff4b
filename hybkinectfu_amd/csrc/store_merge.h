// store_merge.h -- what the kernels that write into the brick store share (device): the slot claim (brickstore.hip: eviction, import, merge; resample.hip)
// and the voxel rule of a map merge (k_store_merge, k_store_resample_merge).
#pragma once
#include "kf_internal.h"
#include "brick_key.h"
#include "brick_find.h"

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

// one voxel of kf_merge_brick_store's rule: a (held, TRUE weight) with b (incoming) -> the weighted running average of tsdfVolume.h:65-70, map to map.
// One rounded fp32 operation per source operation (-ffp-contract=off; `/` is the correctly rounded division).  `blend`: both weights > 0, the colour is averaged
// too; `take`: only b has been observed, b is copied verbatim -- (tb * wb) / wb is not always tb.  Neither: a stays, its weight stored as the true one.
// (The two flags travel by value: as reference parameters they were kept in scratch.)
__device__ __forceinline__ float2 merge_voxel(float ta, float wa, float tb, float wb, float max_weight, bool take, bool blend) {
  if (blend) {
    const float s = wa + wb;
    return make_float2((ta * wa + tb * wb) / s, fminf(s, max_weight));
  }
  return take ? make_float2(tb, wb) : make_float2(ta, wa);
}
__device__ __forceinline__ unsigned merge_channel(unsigned ca, float wa, unsigned cb, float wb) {
  return (unsigned)(unsigned char)fminf(255.f, ((float)ca * wa + (float)cb * wb) / (wa + wb));
}
// the packed colour (x | y << 8 | z << 16, fourth byte 0) of one voxel
__device__ __forceinline__ unsigned merge_color(unsigned ca, float wa, unsigned cb, float wb, bool take, bool blend) {
  if (take) return cb;
  if (!blend) return ca;
  return merge_channel(ca & 255u, wa, cb & 255u, wb) | (merge_channel((ca >> 8) & 255u, wa, (cb >> 8) & 255u, wb) << 8) |
         (merge_channel((ca >> 16) & 255u, wa, (cb >> 16) & 255u, wb) << 16);
}
