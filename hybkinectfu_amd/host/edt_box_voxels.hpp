// edt_box_voxels.hpp -- a box in WORLD metres and a greatest distance in metres as the voxel box and radius kf_map_distance_field takes, and the tile plan
// for boxes beyond its cap (HybKinectfu::distanceField, distanceFieldVoxels).  Plain host C++, fp64; the CPU test compiles this header too
// (tests/map_edt_main.cpp).
#pragma once
#include <math.h>
#include <stdint.h>
#include "erase_box_voxels.hpp"

#define HKF_EDT_TILE 128u          // a tile's greatest edge, voxels: 128 * (128 + 2 * 255)^2 < 2^29, so a tile passes kf_map_distance_field's cap at every radius
#define HKF_EDT_MAX_RADIUS 255u

// The box is hkf_erase_box_voxels': voxel g is in it iff lo_m <= (g + 1/2) * cell < hi_m on every axis, so a corner exactly on a voxel centre takes that voxel
// in at lo and leaves it out at hi.  false: the box is empty on an axis or has a NaN corner; lo_vox and dims are then not to be used.
static inline bool hkf_edt_box_voxels(const float lo_m[3], const float hi_m[3], float cell, int32_t lo_vox[3], uint32_t dims[3]) {
  int32_t hi[3];
  hkf_erase_box_voxels(lo_m, hi_m, cell, lo_vox, hi);
  bool ok = true;
  for (int k = 0; k < 3; ++k) {
    dims[k] = hi[k] > lo_vox[k] ? (uint32_t)((int64_t)hi[k] - (int64_t)lo_vox[k]) : 0u;
    ok = ok && dims[k] > 0u && lo_m[k] == lo_m[k] && hi_m[k] == hi_m[k];
  }
  return ok;
}

// nx * ny * nz of a box the host classes will compute, without overflow: false for a zero dimension or more than HKF_EDT_MAX_VOXELS voxels (the results alone
// are 5 to 7 bytes a voxel on the host; a box of infinite corners is 2^24 per axis, 2^72 voxels, which 64 bits do not hold)
#define HKF_EDT_MAX_VOXELS (1ull << 31)
static inline bool hkf_edt_voxel_count(const uint32_t dims[3], uint64_t* n) {
  *n = 0;
  if (dims[0] == 0u || dims[1] == 0u || dims[2] == 0u) return false;
  const uint64_t a = (uint64_t)dims[0] * dims[1];                  // (< 2^64)
  if (a > HKF_EDT_MAX_VOXELS || a * dims[2] > HKF_EDT_MAX_VOXELS) return false;   // (a <= 2^31 and dims[2] < 2^32: the product fits)
  *n = a * dims[2];
  return true;
}

// floor(maxDist_m / cell) clamped to 1 .. 255 (a NaN gives 1); the caller reports the clamped value back
static inline uint32_t hkf_edt_radius(float maxDist_m, float cell) {
  const double r = floor((double)maxDist_m / (double)cell);
  if (!(r > 1.0)) return 1u;
  return r > (double)HKF_EDT_MAX_RADIUS ? HKF_EDT_MAX_RADIUS : (uint32_t)r;
}

// the tile plan along one axis of n voxels: ceil(n / 128) tiles, tile i = [128 i, min(128 (i + 1), n)) -- they cover the axis once, none is longer than 128
static inline uint32_t hkf_edt_tile_count(uint32_t n) { return (n + HKF_EDT_TILE - 1u) / HKF_EDT_TILE; }
static inline void hkf_edt_tile(uint32_t n, uint32_t i, uint32_t* off, uint32_t* len) {
  *off = i * HKF_EDT_TILE;
  *len = n - *off < HKF_EDT_TILE ? n - *off : HKF_EDT_TILE;
}
