// map_tiles.h -- the tile lattice of kf_marching_cubes_map (mapmesh.hip; no reference counterpart).  Plain host C++: the library and the stand-alone
// test program (tests/map_tiles_main.cpp) both include it.
//
// Space is tiled on a lattice fixed in the WORLD, not at the window.  With T = res - 16, tile k of an axis is the frame F_k = k * T - 8 (voxels; a multiple of
// 8 because res is) and owns the frame's local cells [8, res - 8), i.e. the world cells [k * T, (k + 1) * T).  The owned ranges are disjoint and cover the
// axis, and every owned cell lies eight cells inside its frame: no cell is lost to the rim rule of the extraction and none is emitted twice.
#pragma once
#include <stdint.h>

#define KF_MAP_TILE_MARGIN 8

// floor(a / b) for b > 0
static inline int64_t kf_floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// the tiles k of one axis whose frame [F_k, F_k + res) meets the voxel range [lo, hi): k0 <= k < k1 (empty range: k0 >= k1)
static inline void kf_map_tile_range(int64_t lo, int64_t hi, int res, int64_t* k0, int64_t* k1) {
  const int64_t T = (int64_t)res - 2 * KF_MAP_TILE_MARGIN;
  if (lo >= hi) { *k0 = *k1 = 0; return; }
  *k0 = kf_floor_div(lo + KF_MAP_TILE_MARGIN - res, T) + 1;            // k * T - 8 + res > lo
  *k1 = kf_floor_div(hi + KF_MAP_TILE_MARGIN - 1, T) + 1;              // k * T - 8 < hi
}

// The frames (voxel origins, three per tile) of the tiles whose frame meets the store's bounds (bricks, half-open; lo == hi: no store) or the window's
// bricks (origin_vox .. origin_vox + res), in z, then y, then x order, ascending.  Writes the first `cap` of them to `frames` (may be null with cap 0) and
// returns how many there are, or -1 for a res that is no multiple of 8 or below 32.
static inline int64_t kf_map_tiles(const int32_t store_lo[3], const int32_t store_hi[3], const int32_t origin_vox[3], int res, int32_t* frames, int64_t cap) {
  if (res < 32 || (res % 8) != 0) return -1;
  const int64_t T = (int64_t)res - 2 * KF_MAP_TILE_MARGIN;
  const bool have_store = store_lo[0] < store_hi[0] && store_lo[1] < store_hi[1] && store_lo[2] < store_hi[2];
  int64_t s0[3], s1[3], w0[3], w1[3], a0[3], a1[3];                     // tile ranges: the store's, the window's, both
  for (int k = 0; k < 3; ++k) {
    kf_map_tile_range(origin_vox[k], (int64_t)origin_vox[k] + res, res, &w0[k], &w1[k]);
    if (have_store) kf_map_tile_range((int64_t)store_lo[k] * 8, (int64_t)store_hi[k] * 8, res, &s0[k], &s1[k]);
    else { s0[k] = w0[k]; s1[k] = w0[k]; }
    a0[k] = have_store && s0[k] < w0[k] ? s0[k] : w0[k];
    a1[k] = have_store && s1[k] > w1[k] ? s1[k] : w1[k];
  }
  int64_t n = 0;
  for (int64_t z = a0[2]; z < a1[2]; ++z)
    for (int64_t y = a0[1]; y < a1[1]; ++y)
      for (int64_t x = a0[0]; x < a1[0]; ++x) {
        const bool in_w = x >= w0[0] && x < w1[0] && y >= w0[1] && y < w1[1] && z >= w0[2] && z < w1[2];
        const bool in_s = have_store && x >= s0[0] && x < s1[0] && y >= s0[1] && y < s1[1] && z >= s0[2] && z < s1[2];
        if (!in_w && !in_s) continue;
        if (frames && n < cap) {
          frames[3 * n] = (int32_t)(x * T - KF_MAP_TILE_MARGIN); frames[3 * n + 1] = (int32_t)(y * T - KF_MAP_TILE_MARGIN); frames[3 * n + 2] = (int32_t)(z * T - KF_MAP_TILE_MARGIN);
        }
        ++n;
      }
  return n;
}
