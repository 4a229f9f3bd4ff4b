// map_sample.h -- the map sampled at a point (device): the trilinear value with its gradient, weight and colour (query_sample) and the nearest voxel
// (query_nearest), over the map as map_lookup.h defines it (query_map: a context's).  Shared by query.hip (kf_map_sample, kf_map_cast_rays) and relocal.hip
// (kf_map_score_poses, kf_map_pose_sums).  No reference counterpart: the value and gradient are align_voxel's lines (align.hip), the colour v_interp_color's
// (vwindow.h).  The contract is written out above kf_map_sample in include/hybkf.h.  Include after kf_internal.h,
// brick_key.h, brick_find.h, resample_shared.h (lerp1) and map_lookup.h.
#pragma once
#include <stdint.h>
#include <math.h>

using namespace mapq;

#define KF_QUERY_LIMIT 8388608.0       // 2^23: positions beyond +-this many voxels read unobserved (the key range, brick_key.h)

// one coordinate of a sample: u = p - 1/2 (voxel g has its centre at g + 1/2), base voxel floor(u), fraction (float)(u - floor(u)) -- the difference is exact
// in fp64 (|u| < 2^24), so one rounding.  false: p is not finite or lies outside the key range.
__device__ __forceinline__ bool query_split(double p, int& n, float& f) {
  if (!(fabs(p) <= KF_QUERY_LIMIT)) return false;
  const double u = p - 0.5, fl = floor(u);
  n = (int)fl;
  f = (float)(u - fl);
  return true;
}

struct QuerySample { float tsdf, weight, gx, gy, gz; uchar4 color; };

// The map at point (px, py, pz), world voxels.  All eight corners n + {0, 1}^3 are read (corner k: x from bit 0, y from bit 1, z from bit 2); false --
// unobserved -- when one of them reads weight 0.  GRAD: the gradient too; COLOR: the colour too (0 on a map without a colour plane).
template <bool GRAD, bool COLOR>
__device__ __forceinline__ bool query_sample(const MapRef& m, double px, double py, double pz, MapBrick& b, QuerySample& s) {
  int nx, ny, nz;
  float fx, fy, fz;
  if (!query_split(px, nx, fx) || !query_split(py, ny, fy) || !query_split(pz, nz, fz)) return false;
  float v[8];
  uchar4 col[8];
  float wmin = 0.f;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    unsigned off;
    const float2 q = map_voxel(m, nx + (k & 1), ny + ((k >> 1) & 1), nz + (k >> 2), b, off);
    v[k] = q.x;
    wmin = k == 0 ? q.y : fminf(wmin, q.y);
    ok = ok && q.y > 0.f;
    if (COLOR) col[k] = q.y > 0.f ? map_voxel_color(b, off) : make_uchar4(0, 0, 0, 0);
  }
  if (!ok) return false;
  // align_voxel's lines: the value x, then y, then z; the gradient from the same eight values
  const float a0 = lerp1(v[0], v[1], fx), a1 = lerp1(v[2], v[3], fx), a2 = lerp1(v[4], v[5], fx), a3 = lerp1(v[6], v[7], fx);
  const float b0 = lerp1(a0, a1, fy), b1 = lerp1(a2, a3, fy);
  s.tsdf = lerp1(b0, b1, fz);
  s.weight = wmin;
  if (GRAD) {
    const float d0 = v[1] - v[0], d1 = v[3] - v[2], d2 = v[5] - v[4], d3 = v[7] - v[6];
    s.gx = lerp1(lerp1(d0, d1, fy), lerp1(d2, d3, fy), fz);
    s.gy = lerp1(a1 - a0, a3 - a2, fz);
    s.gz = b1 - b0;
  }
  if (COLOR) {
    // v_interp_color's arithmetic and corner order: its corner j has x from bit 2, y from bit 1, z from bit 0
    const float a = fx, bb = fy, c = fz, ia = 1 - a, ib = 1 - bb, ic = 1 - c;
    float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uchar4 cj = col[(j >> 2) | (j & 2) | ((j & 1) << 2)];
      const float wa = (j >> 2) ? a : ia, wb = ((j >> 1) & 1) ? bb : ib, wc = (j & 1) ? c : ic;
      const float t0 = (float)cj.x * wa * wb * wc, t1 = (float)cj.y * wa * wb * wc, t2 = (float)cj.z * wa * wb * wc;
      acc[0] = (j == 0) ? t0 : acc[0] + t0; acc[1] = (j == 0) ? t1 : acc[1] + t1; acc[2] = (j == 0) ? t2 : acc[2] + t2;
    }
    s.color = make_uchar4((unsigned char)acc[0], (unsigned char)acc[1], (unsigned char)acc[2], 0);
  }
  return true;
}

// the tsdf of the voxel the point lies in, floor(p): what the reference's getVoxel reads on the march.  0 where nobody observed.
__device__ __forceinline__ float query_nearest(const MapRef& m, double px, double py, double pz, MapBrick& b) {
  if (!(fabs(px) <= KF_QUERY_LIMIT) || !(fabs(py) <= KF_QUERY_LIMIT) || !(fabs(pz) <= KF_QUERY_LIMIT)) return 0.f;
  unsigned off;
  return map_voxel(m, (int)floor(px), (int)floor(py), (int)floor(pz), b, off).x;
}
