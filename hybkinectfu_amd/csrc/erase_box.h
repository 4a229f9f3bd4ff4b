// erase_box.h -- what kf_brick_store_erase_box decides from coordinates alone: the clamp of the caller's box, the class of a brick against the box
// and the voxel-in-box test (erase.hip; no reference counterpart).  Host and device: the CPU test compiles this header too (tests/map_erase_main.cpp).
// World voxel g lies in brick g >> 3 at in-brick position g & 7 (arithmetic shift: negative coordinates floor); the box is half-open, lo <= g < hi.
#pragma once
#include <stdint.h>

#ifndef __host__
#define __host__
#define __device__
#endif

#define KF_ERASE_BOX_INSIDE 0      // clear the voxels inside the box (KF_ERASE_INSIDE)
#define KF_ERASE_BOX_OUTSIDE 1     // clear the voxels outside the box (KF_ERASE_OUTSIDE)
#define KF_ERASE_VOX_MIN (-(1 << 23))   // the key range in voxels: bricks [-2^20, 2^20), so voxels [-2^23, 2^23)
#define KF_ERASE_VOX_MAX (1 << 23)      // (exclusive: the upper end of a half-open box may equal it)

enum { KF_BRICK_UNTOUCHED = 0, KF_BRICK_CUT = 1, KF_BRICK_REMOVED = 2 };

// a box by value (a kernel argument): named components, so nothing is indexed at run time
struct KfEraseBox { int lx, ly, lz, hx, hy, hz; };

__host__ __device__ static inline int32_t kf_erase_clamp(int32_t v) {
  return v < KF_ERASE_VOX_MIN ? KF_ERASE_VOX_MIN : (v > KF_ERASE_VOX_MAX ? KF_ERASE_VOX_MAX : v);
}
// the caller's box clamped to the key range; an axis with lo >= hi makes the whole box empty: (0, 0, 0) - (0, 0, 0).  After this every difference
// and every brick corner (8 * key + 8) of a key in range fits an int32 with room to spare.
__host__ __device__ static inline KfEraseBox kf_erase_box_clamped(const int32_t lo[3], const int32_t hi[3]) {
  KfEraseBox b = {kf_erase_clamp(lo[0]), kf_erase_clamp(lo[1]), kf_erase_clamp(lo[2]), kf_erase_clamp(hi[0]), kf_erase_clamp(hi[1]), kf_erase_clamp(hi[2])};
  if (b.lx >= b.hx || b.ly >= b.hy || b.lz >= b.hz) { const KfEraseBox e = {0, 0, 0, 0, 0, 0}; return e; }
  return b;
}

// how many of the 8 voxels [8 k, 8 k + 8) of one axis lie in [lo, hi): 0 ... 8
__host__ __device__ static inline int kf_erase_axis_overlap(int k, int lo, int hi) {
  const int a = 8 * k > lo ? 8 * k : lo, b = 8 * k + 8 < hi ? 8 * k + 8 : hi;
  return b > a ? b - a : 0;
}

// the class of brick (kx, ky, kz), a key in range, under a clamped box: how many of its 512 voxels lie inside decides it.
// INSIDE: none -> untouched, all -> removed.  OUTSIDE: all -> untouched, none -> removed.  Anything in between: cut.
__host__ __device__ static inline int kf_erase_brick_class(const KfEraseBox& b, int mode, int kx, int ky, int kz) {
  const int in = kf_erase_axis_overlap(kx, b.lx, b.hx) * kf_erase_axis_overlap(ky, b.ly, b.hy) * kf_erase_axis_overlap(kz, b.lz, b.hz);
  if (in == 0) return mode == KF_ERASE_BOX_INSIDE ? KF_BRICK_UNTOUCHED : KF_BRICK_REMOVED;
  if (in == 512) return mode == KF_ERASE_BOX_INSIDE ? KF_BRICK_REMOVED : KF_BRICK_UNTOUCHED;
  return KF_BRICK_CUT;
}

// is world voxel (gx, gy, gz) to be cleared?  Comparisons only.
__host__ __device__ static inline bool kf_erase_voxel_cleared(const KfEraseBox& b, int mode, int gx, int gy, int gz) {
  const bool in = gx >= b.lx && gx < b.hx && gy >= b.ly && gy < b.hy && gz >= b.lz && gz < b.hz;
  return in == (mode == KF_ERASE_BOX_INSIDE);
}
