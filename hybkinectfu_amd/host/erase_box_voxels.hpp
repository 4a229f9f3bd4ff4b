// erase_box_voxels.hpp -- a box in WORLD metres as the half-open box of world voxel indices kf_brick_store_erase_box takes (HybKinectfu::eraseMapBox).
// Plain host C++, fp64; the CPU test compiles this header too (tests/map_erase_main.cpp).
#pragma once
#include <math.h>
#include <stdint.h>
#include "../csrc/erase_box.h"

// World metres are the first cube's coordinates: those of the map mesh's vertices and of worldPose.  Voxel g has its centre at (g + 1/2) * cell, and a
// voxel is in the box iff its centre is: lo_m <= (g + 1/2) * cell < hi_m.  So both ends are ceil(x / cell - 1/2): the first voxel whose centre is not
// below x -- inclusive for lo, exclusive for hi; a corner exactly on a centre takes that voxel in at lo and leaves it out at hi.  A result that is not
// finite or lies beyond the key range clamps to it (+inf: 2^23, -inf: -2^23); a NaN gives -2^23 at both ends, so a NaN corner makes its axis empty.
static inline int32_t hkf_erase_voxel_of(double x_m, double cell) {
  const double g = ceil(x_m / cell - 0.5);
  if (!(g > (double)KF_ERASE_VOX_MIN)) return KF_ERASE_VOX_MIN;             // (also NaN)
  if (g > (double)KF_ERASE_VOX_MAX) return KF_ERASE_VOX_MAX;
  return (int32_t)g;
}
static inline void hkf_erase_box_voxels(const float lo_m[3], const float hi_m[3], float cell, int32_t lo_vox[3], int32_t hi_vox[3]) {
  for (int k = 0; k < 3; ++k) {
    lo_vox[k] = hkf_erase_voxel_of((double)lo_m[k], (double)cell);
    hi_vox[k] = hkf_erase_voxel_of((double)hi_m[k], (double)cell);
  }
}
