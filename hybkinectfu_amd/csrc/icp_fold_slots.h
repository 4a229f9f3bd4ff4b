// icp_fold_slots.h -- the counting rules of the persistent tracking loops (track.hip) that the host shares with the device: how many workgroups publish
// partial sums at a pyramid level (icp_level_geometry), how many tagged words a lane of the fold polls per batch (icp_fold_batch_slots), and which lane polls
// which pair of words (icp_fold_pair_lane and its neighbours).  Plain C++ apart from the __host__ __device__ marks: tests/icp_fold_slots_main.cpp and
// tests/icp_pair_slots_main.cpp compile this header alone and run it under sanitizers.  No reference counterpart.
#pragma once

#ifndef __host__
#define __host__
#define __device__
#endif

// 512 lanes x up to ICP_PX (3) pixels per workgroup: 200 workgroups at VGA level 0 (few partials to fold, no register spills).
#define ICP_THREADS 512
#ifndef ICP_PX
#define ICP_PX 3
#endif
// Pixels per lane (px_l) and publishing workgroups (grid_l) of a pyramid level with npx pixels, under a launch geometry of loop_grid
// workgroups (= the workgroups level 0 needs at ICP_PX pixels per lane).  Two things pull: fewer pixels per lane shorten the pixel
// phase (a coarse step is mostly latency), but every workgroup that holds pixels is one more publisher the step has to wait for (all
// 256 CUs publishing at every level: +36 us per frame).  Measured at VGA on 200 workgroups, tracking stage in us for (level 0, 1, 2)
// pixels per lane, with the fold's two polls in flight: (3,3,1) 162.4, (3,2,2) 161.9, (3,2,1) 159.4, (3,1,1) 156.3 (with one poll in
// flight (3,2,1) was ahead: 172.6 vs 175.5).  Rule: the fewest pixels per lane the launch can hold.  Host and device, both launch forms.
__host__ __device__ static inline void icp_level_geometry(int npx, int loop_grid, int level, int& px_l, int& grid_l) {
  px_l = ICP_PX;
#ifndef KF_ICP_FIXED_PX
  for (int p = 1; p < ICP_PX; ++p) if ((npx + ICP_THREADS * p - 1) / (ICP_THREADS * p) <= loop_grid) { px_l = p; break; }
#ifdef KF_ICP_PX_L0                                                              // tuning overrides (tools/build_variant.sh)
  if (level == 0) px_l = KF_ICP_PX_L0;
#endif
#ifdef KF_ICP_PX_L1
  if (level == 1) px_l = KF_ICP_PX_L1;
#endif
#ifdef KF_ICP_PX_L2
  if (level == 2) px_l = KF_ICP_PX_L2;
#endif
#endif
  (void)level;
  grid_l = (npx + ICP_THREADS * px_l - 1) / (ICP_THREADS * px_l);
}

// The fold of the tagged partial sums (fold_partials_tagged) deals the publishers w = 0 .. n_wg-1 to `parts` lanes per sum: part p adds w = p, p + parts,
// p + 2 parts, ... in ascending order, ICP_FOLD_BATCH of them per batch -- so batch b covers the publishers [base, base + ICP_FOLD_BATCH * parts) with
// base = b * ICP_FOLD_BATCH * parts, and slot j of part p in it is the publisher base + p + j * parts.
#define ICP_FOLD_BATCH 13
// Slot counts the poll is compiled for, below ICP_FOLD_BATCH (which always is): at VGA and 16 parts the 38 publishers of level 2 need 3 slots, the 150 of
// level 1 ten, the 200 of level 0 all thirteen, and the second batch of the SDF loop's 256 publishers three.  X(n) for every n, ascending.
#ifndef ICP_FOLD_LADDER
#ifdef KF_ICP_FOLD_LADDER_FINE                                                   // tuning variant (tools/build_variant.sh): profiles/icp_fold_shapes.txt
#define ICP_FOLD_LADDER(X) X(2) X(4) X(7) X(10)
#elif defined(KF_ICP_FOLD_LADDER_NONE)                                           // every batch polls ICP_FOLD_BATCH slots
#define ICP_FOLD_LADDER(X)
#else
#define ICP_FOLD_LADDER(X) X(3) X(10)
#endif
#endif
// Slots per lane the poll of the batch at `base` runs with: the slot rows that have a publisher at all, ceil((n_wg - base) / parts) capped at ICP_FOLD_BATCH,
// rounded up to the next compiled count.  The same for every lane of the workgroup.  A lane whose slot j below that count still has no publisher (the
// ragged last row) polls its own first word there and drops the value.
__host__ __device__ static inline int icp_fold_batch_slots(int n_wg, int base, int parts) {
  const int left = n_wg - base;                                                  // (rows <= n without a division: left <= n * parts)
#define ICP_FOLD_RUNG(n) if (left <= (n) * parts) return (n);
  ICP_FOLD_LADDER(ICP_FOLD_RUNG)
#undef ICP_FOLD_RUNG
  return ICP_FOLD_BATCH;
}

// The pair form of the fold (the ICP loops): the sums 2m and 2m + 1 of a publisher lie in one aligned 16-byte unit of its slot row (words 2m, 2m + 1 of 32),
// which a lane of the fold polls with ONE load.  14 pairs cover the 27 sums; the second half of pair 13 is word 27, padding: never added.  The fold's lanes:
// 16 per part (one DPP row), the first 14 of them one pair each, parts * 16 lanes in all -- the first four of a 512-lane workgroup's eight waves; the other
// waves poll nothing.  Which publishers a part adds, and in which order, is the rule above, unchanged.
#define ICP_SUMS 27
#define ICP_FOLD_PAIRS ((ICP_SUMS + 1) / 2)
__host__ __device__ static inline int icp_pair_of_sum(int k) { return k >> 1; }
// does sum `half` (0 / 1) of pair m exist -- or is it the padding word?
__host__ __device__ static inline bool icp_pair_half_is_sum(int m, int half) { return 2 * m + half < ICP_SUMS; }
// lane t of the workgroup -> (part, pair); false: the lane polls nothing
__host__ __device__ static inline bool icp_fold_pair_lane(int t, int parts, int& part, int& m) {
  part = t >> 4; m = t & 15;
  return part < parts && m < ICP_FOLD_PAIRS;
}
// byte offset of pair m of publisher w in a step's slot array (32 eight-byte words per publisher)
__host__ __device__ static inline unsigned icp_pair_byte_offset(int w, int m) { return (unsigned)(w * 32 + 2 * m) * 8u; }
// the pair store (a build variant, -DKF_ICP_STORE16; the product stores single words): the lane that stores pair m after icp_wg_reduce (sum k ends up in lane
// 4 k + 3: the holder of the pair's second sum, which fetches the first from four lanes below and stores the padding half as {0, tag}) -- and the pair a lane
// stores, or -1
__host__ __device__ static inline int icp_pair_store_lane(int m) { return 8 * m + 7; }
__host__ __device__ static inline int icp_pair_stored_by(int t) { return ((t & 7) == 7 && (t >> 3) < ICP_FOLD_PAIRS) ? (t >> 3) : -1; }
