// strip_boxes.h -- the strip rule of the moving volume: what a move of the window touches at its rim, as up to three disjoint half-open boxes in a fixed
// order -- the x strip in full, the y strip without the x strip, the z strip without both.  Along an axis of length n a move s > 0 takes the strip
// [0, min(n, s + reach)), a move s < 0 the strip [max(0, n + s - reach), n), s == 0 nothing.  Callers: the cells whose 27 voxels include a voxel that leaves
// (reach 1, n = res: kf_shift_volume's stream-out in shift.hip, hkf_departing_boxes in host/recentre.cpp) and the bricks that leave, or with -s enter
// (reach 0, n = nb: brickstore.hip).  Plain C++, no device code: tests/strip_boxes_main.cpp runs it under sanitizers.  No reference counterpart.
#pragma once
#include <stdint.h>

// Returns the number of boxes written to lo[] / hi[] (x, y, z); empty boxes are dropped.  0 < n <= 2^30; 64-bit inside, so any 32-bit move is fine.
static inline int kf_strip_boxes(int64_t sx, int64_t sy, int64_t sz, int64_t n, int64_t reach, int32_t lo[3][3], int32_t hi[3][3]) {
  const int64_t s[3] = {sx, sy, sz};
  int64_t slo[3], shi[3], klo[3], khi[3];                  // per axis: the strip, and what is left of the axis without it
  for (int k = 0; k < 3; ++k) {
    if (s[k] > 0) { slo[k] = 0; shi[k] = s[k] + reach > n ? n : s[k] + reach; klo[k] = shi[k]; khi[k] = n; }
    else if (s[k] < 0) { shi[k] = n; slo[k] = n + s[k] - reach < 0 ? 0 : n + s[k] - reach; klo[k] = 0; khi[k] = slo[k]; }
    else { slo[k] = shi[k] = 0; klo[k] = 0; khi[k] = n; }
  }
  int boxes = 0;
  for (int k = 0; k < 3; ++k) {
    bool empty = false;
    for (int j = 0; j < 3; ++j) {
      const int64_t l = j < k ? klo[j] : (j == k ? slo[j] : 0), h = j < k ? khi[j] : (j == k ? shi[j] : n);
      lo[boxes][j] = (int32_t)l; hi[boxes][j] = (int32_t)h;
      if (l >= h) empty = true;
    }
    if (!empty) ++boxes;
  }
  return boxes;
}
