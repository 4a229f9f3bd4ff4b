// recentre.cpp -- the host arithmetic of the moving volume (hybkf_host.hpp): when and how far HybKinectfu::processNewFrame shifts the window, and the
// origin offset that turns volume coordinates into world coordinates for the trajectory recorder and the mesh writers.  No reference counterpart.
// Nothing here touches the device or another translation unit, so a stand-alone program can run it under a sanitizer (tests/shift_host_main.cpp).
#include "hybkf_host.hpp"
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

extern "C" void hkf_world_pose(float pose[16], const int32_t o[3], float cell) {
  if (o[0] == 0 && o[1] == 0 && o[2] == 0) return;
  for (int i = 0; i < 3; ++i) pose[4 * i + 3] = pose[4 * i + 3] + (float)o[i] * cell;
}

extern "C" void hkf_world_positions(float* xyz, size_t n, const int32_t o[3], float cell) {
  if (o[0] == 0 && o[1] == 0 && o[2] == 0) return;
  const float t[3] = {(float)o[0] * cell, (float)o[1] * cell, (float)o[2] * cell};
  for (size_t v = 0; v < n; ++v) for (int i = 0; i < 3; ++i) xyz[3 * v + i] = xyz[3 * v + i] + t[i];
}
