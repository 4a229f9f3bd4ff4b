// view_pixel.h -- one display pixel (b, g, r, a from the low byte up) from a raycast hit: what the reference's DataViewer paints on the host
// after a blocking copy of the float4 maps (src/DataViewer.cpp:12-58, called from src/HybKinectfu.cpp:145-158).  Shared by the view march
// (raycast.hip: k_raycast_view) and the pass over the model maps (view.hip: k_view_maps), so both give the same bytes for the same maps.
// fp32 throughout, one rounding per source operation (the library is built with -ffp-contract=off); tests/view_expect.py restates it in numpy.
#pragma once
#include "kf_internal.h"

// `(unsigned char)f` as the reference's host code converts (truncate towards zero, keep the low byte); kf_f2i saturates and maps NaN to 0, where C++
// leaves the cast undefined.  Every value the formulas below produce from a unit normal lies in [0, 255].
__device__ __forceinline__ unsigned kf_view_byte(float f) { return (unsigned)kf_f2i(f) & 255u; }

// v.w == 1: the pixel is a hit (raycastingVolume.cu:90 writes w = 1 with the vertex; every other pixel keeps the zeros of :128-131).
//   KF_VIEW_NORMALS  DataViewer::viewNormal, DataViewer.cpp:24-26: (255 * (n + 1)) / 2 per component -- 127, 127, 127 where there is no normal
//   KF_VIEW_SHADED   one grey level: the cosine between the normal and the direction to the eye (the pose's translation), headlight shading;
//                    32 + 223 * cos on a hit, 0 elsewhere
//   KF_VIEW_COLOR    interpolateColor at the vertex (raycastingVolume.cu:91-92), kept whether or not the gradient succeeded, like KF_MAP_RAYCAST_RGB
// byte 3: 255 on a hit, else 0.
template <int MODE>
__device__ __forceinline__ unsigned kf_view_pixel(float4 v, float4 n, uchar4 c, float3 eye) {
  const bool hit = v.w == 1.0f;
  const unsigned a = hit ? 0xFF000000u : 0u;
  if (MODE == KF_VIEW_NORMALS) {
    const unsigned b0 = kf_view_byte((255.f * (n.x + 1.f)) / 2.f), b1 = kf_view_byte((255.f * (n.y + 1.f)) / 2.f), b2 = kf_view_byte((255.f * (n.z + 1.f)) / 2.f);
    return b0 | (b1 << 8) | (b2 << 16) | a;
  }
  if (MODE == KF_VIEW_SHADED) {
    if (!hit) return 0u;
    const float dx = eye.x - v.x, dy = eye.y - v.y, dz = eye.z - v.z;
    const float s = (dx * dx + dy * dy) + dz * dz;
    float cs = ((n.x * dx + n.y * dy) + n.z * dz) / sqrtf(s);
    cs = fminf(fmaxf(cs, 0.f), 1.f);                                     // (fmaxf(NaN, 0) = 0: a vertex AT the eye is as dark as a grazing one)
    const unsigned g = kf_view_byte(32.f + 223.f * cs);
    return g | (g << 8) | (g << 16) | a;
  }
  return (unsigned)c.x | ((unsigned)c.y << 8) | ((unsigned)c.z << 16) | a;
}
