// recentre.cpp -- the host arithmetic of the moving volume (hybkf_host.hpp): when and how far HybKinectfu::processNewFrame shifts the window, and the
// origin offset that turns volume coordinates into world coordinates for the trajectory recorder and the mesh writers.  No reference counterpart.
// hkf_view_frame: which frame of the map a viewer's world pose looks into (HybKinectfu::renderMapView).
// hkf_departing_boxes: which cells a shift makes unextractable for good -- the boxes kf_shift_volume's stream-out sends to the world soup.
// Nothing here touches the device or another translation unit, so a stand-alone program can run it under a sanitizer (tests/shift_host_main.cpp).
#include "hybkf_host.hpp"
#include "../csrc/strip_boxes.h"
#include <math.h>

extern "C" void hkf_recentre_shift(const float pose[16], float size_m, uint32_t res, float dist, int32_t out[3]) {
  out[0] = out[1] = out[2] = 0;
  if (!(dist > 0.f) || res == 0 || !(size_m > 0.f)) return;
  const float half = size_m * 0.5f;                              // the centre's coordinate and the focus distance along the optical axis
  const float step = 8.f * (size_m / (float)res);                // one brick in metres
  float off[3]; bool far = false;
  for (int i = 0; i < 3; ++i) {
    const float focus = pose[4 * i + 3] + pose[4 * i + 2] * half;  // t + R (0, 0, size / 2)
    off[i] = focus - half;
    if (!(fabsf(off[i]) <= 3.0e38f)) return;                     // NaN / infinite pose: no decision
    if (fabsf(off[i]) > dist) far = true;
  }
  if (!far) return;
  for (int i = 0; i < 3; ++i) {
    float q = truncf(off[i] / step);
    q = q > 1.0e6f ? 1.0e6f : (q < -1.0e6f ? -1.0e6f : q);       // (beyond any volume: keeps the conversion defined)
    out[i] = (int32_t)q * 8;
  }
}

// The frame whose window a view from `world_pose` wants: hkf_recentre_shift's focus, truncation and clamp without its distance test, then the pose in
// that frame's coordinates (the expression of k_shift_pose / hkf_world_pose, the other way round).
extern "C" void hkf_view_frame(const float world_pose[16], float size_m, uint32_t res, int32_t frame[3], float local_pose[16]) {
  frame[0] = frame[1] = frame[2] = 0;
  for (int i = 0; i < 16; ++i) local_pose[i] = world_pose[i];
  if (res == 0 || !(size_m > 0.f)) return;
  const float half = size_m * 0.5f;
  const float cell = size_m / (float)res;
  const float step = 8.f * cell;                                 // one brick in metres
  float off[3];
  for (int i = 0; i < 3; ++i) {
    const float focus = world_pose[4 * i + 3] + world_pose[4 * i + 2] * half;  // t + R (0, 0, size / 2)
    off[i] = focus - half;
    if (!(fabsf(off[i]) <= 3.0e38f)) return;                     // NaN / infinite pose: frame 0, the pose as it came
  }
  for (int i = 0; i < 3; ++i) {
    float q = truncf(off[i] / step);
    q = q > 1.0e6f ? 1.0e6f : (q < -1.0e6f ? -1.0e6f : q);
    frame[i] = (int32_t)q * 8;
    local_pose[4 * i + 3] = world_pose[4 * i + 3] - (float)frame[i] * cell;
  }
}

// The cells whose 27 voxels (x-1 .. x+1 each way) include a voxel that leaves the window when it moves by d: along one axis with d > 0 voxels
// < d leave, so cells [0, d + 1); with d < 0 cells [res + d - 1, res); |d| >= res: every cell.  Over several axes the union, as disjoint boxes
// in a fixed order: the x strip in full, the y strip without the x strip, the z strip without both (strip_boxes.h, reach 1).  Only non-empty boxes are written.
extern "C" int hkf_departing_boxes(const int32_t d[3], uint32_t res, int32_t lo[3][3], int32_t hi[3][3]) {
  if (res == 0 || res > 0x40000000u) return 0;
  return kf_strip_boxes(d[0], d[1], d[2], res, 1, lo, hi);
}

extern "C" void hkf_world_pose(float pose[16], const int32_t o[3], float cell) {
  if (o[0] == 0 && o[1] == 0 && o[2] == 0) return;
  for (int i = 0; i < 3; ++i) pose[4 * i + 3] = pose[4 * i + 3] + (float)o[i] * cell;
}

extern "C" void hkf_world_positions(float* xyz, size_t n, const int32_t o[3], float cell) {
  if (o[0] == 0 && o[1] == 0 && o[2] == 0) return;
  const float t[3] = {(float)o[0] * cell, (float)o[1] * cell, (float)o[2] * cell};
  for (size_t v = 0; v < n; ++v) for (int i = 0; i < 3; ++i) xyz[3 * v + i] = xyz[3 * v + i] + t[i];
}
