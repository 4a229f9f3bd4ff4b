// store_merge.h -- what the kernels that write into the brick store share (device): the slot claim (brickstore.hip: eviction, import, merge; resample.hip;
// halve.hip), the unpacking of staged colour bytes (k_store_import, k_store_merge) and the rule of a map merge, voxel by voxel and as the whole tail of a
// merging kernel's loop body (store_merge_pair: k_store_merge, k_store_resample_merge, k_store_halve).
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

// the packed colours of a lane's two voxels from the staged bytes of entry offset o (in voxels): six bytes, c0 c1 | c2 c0' | c1' c2', as three 16-bit loads (the
// staged bytes are 2-byte aligned).  No colour given: zeros.
__device__ __forceinline__ void staged_colors(const unsigned char* color, size_t o, unsigned& c0, unsigned& c1) {
  c0 = 0u; c1 = 0u;
  if (!color) return;
  const unsigned short* cs = reinterpret_cast<const unsigned short*>(color + 3 * o) + 3u * threadIdx.x;
  const unsigned a = cs[0], b = cs[1], c = cs[2];
  c0 = a | ((b & 255u) << 16); c1 = (b >> 8) | (c << 8);
}

// one incoming voxel of a merge; c: the colour packed as the slot holds it (x | y << 8 | z << 16)
struct KfIncoming { float t, w; unsigned c; };
// what thread 0 tells the workgroup about the key's slot; the kernel declares one __shared__
struct KfMergeShared { unsigned slot, fresh; unsigned long long pend; };

// The tail of a merging kernel's loop body: the brick `key` whose lane holds the incoming voxels v0, v1 (x-adjacent: the slot's float4) meets the store.  Called
// by all 256 lanes of the workgroup; every return is workgroup-uniform.  Thread 0 looks the key up; a key the store does not hold claims a slot and is written
// as k_store_import writes it, bit for bit.  A held slot is read, merged voxel by voxel and written back in place, the held weight being the TRUE weight (the
// slot's deferred-weight word applied as k_store_export applies it; a lane's two voxels lie in quarter threadIdx.x >> 6).  Every weight written is a true
// weight, so the word becomes 0.  Thread 0 reads the word before the second barrier and is the only one to write it, and every key occurs once per launch: no
// two workgroups, and no two lanes, meet in a slot.  color_given: kernel-uniform; without it a held colour stays and a fresh one is v.c (zeros).
// The function owns its first barrier, so "everybody has read the last call's words in sh" holds by construction: a lane reads sh only between the second
// barrier of a call and the first of the next.  (The flags and the incoming voxels travel by value, as merge_voxel's do.)
template <bool COLOR>
__device__ __forceinline__ void store_merge_pair(const KfBrickStore& st, unsigned long long key, KfIncoming v0, KfIncoming v1, bool color_given, float max_weight,
                                                 KfMergeShared& sh) {
  if (!__syncthreads_or(v0.w > 0.f || v1.w > 0.f)) return;                    // (workgroup-uniform) nothing observed: takes no slot, changes no held one
  if (threadIdx.x == 0) {
    unsigned slot = store_find(st, key);
    const bool fresh = slot == KF_BRICK_NO_SLOT;
    if (fresh) slot = store_claim(st, key);
    sh.slot = slot; sh.fresh = fresh ? 1u : 0u;
    sh.pend = fresh ? 0ull : st.pend[slot];
  }
  __syncthreads();
  const unsigned slot = sh.slot;
  if (slot == KF_BRICK_NO_SLOT) return;                                       // (workgroup-uniform) the store is full: counted as dropped
  float4* tw = reinterpret_cast<float4*>(st.tw + (size_t)slot * KF_BRICK_VOX) + threadIdx.x;
  if (sh.fresh) {                                                             // (workgroup-uniform) k_store_import's write
    *tw = make_float4(v0.t, v0.w, v1.t, v1.w);
    if (COLOR) reinterpret_cast<uint2*>(st.color + (size_t)slot * KF_BRICK_VOX)[threadIdx.x] = make_uint2(v0.c, v1.c);
    if (threadIdx.x == 0) { st.pend[slot] = 0ull; st.key[slot] = key; }
    return;
  }
  const unsigned pq = (unsigned)(sh.pend >> (16u * (threadIdx.x >> 6))) & 0xFFFFu;   // (wave-uniform)
  const float4 h = *tw;
  const float wa0 = kf_pend_weight(h.y, pq, max_weight), wa1 = kf_pend_weight(h.w, pq, max_weight);
  const bool blend0 = v0.w > 0.f && wa0 > 0.f, take0 = v0.w > 0.f && !(wa0 > 0.f), blend1 = v1.w > 0.f && wa1 > 0.f, take1 = v1.w > 0.f && !(wa1 > 0.f);
  const float2 m0 = merge_voxel(h.x, wa0, v0.t, v0.w, max_weight, take0, blend0), m1 = merge_voxel(h.z, wa1, v1.t, v1.w, max_weight, take1, blend1);
  *tw = make_float4(m0.x, m0.y, m1.x, m1.y);
  if (COLOR && color_given) {                                                 // no colour given (kernel-uniform): the held colour stays
    uint2* cp = reinterpret_cast<uint2*>(st.color + (size_t)slot * KF_BRICK_VOX) + threadIdx.x;
    const uint2 ca = *cp;
    *cp = make_uint2(merge_color(ca.x, wa0, v0.c, v0.w, take0, blend0), merge_color(ca.y, wa1, v1.c, v1.w, take1, blend1));
  }
  if (threadIdx.x == 0) st.pend[slot] = 0ull;                                 // (st.key[slot] stays)
}
