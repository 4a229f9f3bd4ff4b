// query.hip -- querying the map where it lies: tsdf, gradient, weight and colour at N points (kf_map_sample), the first surface crossing of N rays
// (kf_map_cast_rays).  The map is the window's bricks and, outside the window, the brick store's (map_lookup.h): no resolve table, no window move, no copy.
// The march is the reference's (src/cuda/raycastingVolume.cu:79-117) restated over the map; the sample has no reference counterpart -- its value and
// gradient are align_voxel's lines (align.hip), its colour v_interp_color's (vwindow.h): map_sample.h.  The contract is written out above kf_map_sample in
// include/hybkf.h, the argument in DESIGN.md 4e-8.  Both kernels only read the context: one lane per point / ray, 256-thread workgroups, grid-stride.
#include "kf_internal.h"
#include "brick_key.h"
#include "brick_find.h"
#include "resample_shared.h"
#include "map_lookup.h"
#include "map_sample.h"

#define KF_QUERY_MAX_STEPS (1u << 24)  // (float)k is exact up to here

template <bool COLOR>
__global__ void __launch_bounds__(256) k_map_sample(MapRef m, unsigned n, const double* __restrict__ pos, float* __restrict__ out_tsdf, float* __restrict__ out_weight,
                                                    float* __restrict__ out_grad, unsigned char* __restrict__ out_color) {
  MapBrick b = map_brick_none();
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) {
    QuerySample s;
    const bool ok = query_sample<true, COLOR>(m, pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], b, s);
    if (out_tsdf) out_tsdf[i] = ok ? s.tsdf : 0.f;
    if (out_weight) out_weight[i] = ok ? s.weight : 0.f;
    if (out_grad) { out_grad[3 * i] = ok ? s.gx : 0.f; out_grad[3 * i + 1] = ok ? s.gy : 0.f; out_grad[3 * i + 2] = ok ? s.gz : 0.f; }
    if (out_color) {
      const uchar4 c = (COLOR && ok) ? s.color : make_uchar4(0, 0, 0, 0);
      out_color[4 * i] = c.x; out_color[4 * i + 1] = c.y; out_color[4 * i + 2] = c.z; out_color[4 * i + 3] = 0;
    }
  }
}

// One lane per ray.  Sample k at t_k = t_min + (float)k * step, per axis origin + (double)(t_k * dir): the product in fp32, the sum in fp64.  A sample in a
// brick nobody holds is answered by the lane's cached "absent" with no load.  The crossing: the last nearest-voxel tsdf > 0 and this one < 0.
template <bool COLOR>
__global__ void __launch_bounds__(256) k_map_cast(MapRef m, unsigned n, const double* __restrict__ origin, const float* __restrict__ dir, const float* __restrict__ tmin,
                                                  const float* __restrict__ tmax, float step, unsigned max_steps, unsigned char* __restrict__ out_status,
                                                  float* __restrict__ out_t, float* __restrict__ out_normal, unsigned char* __restrict__ out_color,
                                                  float* __restrict__ out_weight) {
  MapBrick b = map_brick_none();
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) {
    const double ox = origin[3 * i], oy = origin[3 * i + 1], oz = origin[3 * i + 2];
    const float dx = dir[3 * i], dy = dir[3 * i + 1], dz = dir[3 * i + 2];
    const float t0 = tmin[i], t1 = tmax[i];
    unsigned status = KF_RAY_MISS;
    float hit_t = 0.f, nx = 0.f, ny = 0.f, nz = 0.f, hit_w = 0.f;
    uchar4 hit_c = make_uchar4(0, 0, 0, 0);
    float last = 0.f;
    for (unsigned k = 0; k < max_steps; ++k) {
      const float tk = t0 + (float)k * step;
      if (!(tk < t1)) break;
      const double px = ox + (double)(tk * dx), py = oy + (double)(tk * dy), pz = oz + (double)(tk * dz);
      const float sdf = query_nearest(m, px, py, pz, b);
      if (last > 0.f && sdf < 0.f) {
        status = KF_RAY_BROKEN;
        const float tl = t0 + (float)(k - 1u) * step;
        QuerySample s0, s1, sh;
        if (!query_sample<false, false>(m, px, py, pz, b, s1)) break;
        if (!query_sample<false, false>(m, ox + (double)(tl * dx), oy + (double)(tl * dy), oz + (double)(tl * dz), b, s0)) break;
        const float alpha = tk - step * s1.tsdf / (s1.tsdf - s0.tsdf);
        if (!query_sample<true, COLOR>(m, ox + (double)(alpha * dx), oy + (double)(alpha * dy), oz + (double)(alpha * dz), b, sh)) break;
        const float len = sqrtf((sh.gx * sh.gx + sh.gy * sh.gy) + sh.gz * sh.gz);    // (correctly rounded, like `/`: the compiler's default for HIP)
        if (!(len >= 1e-8f)) break;
        status = KF_RAY_HIT;
        hit_t = alpha; nx = sh.gx / len; ny = sh.gy / len; nz = sh.gz / len; hit_w = sh.weight;
        if (COLOR) hit_c = sh.color;
        break;
      }
      last = sdf;
    }
    if (out_status) out_status[i] = (unsigned char)status;
    if (out_t) out_t[i] = hit_t;
    if (out_normal) { out_normal[3 * i] = nx; out_normal[3 * i + 1] = ny; out_normal[3 * i + 2] = nz; }
    if (out_color) { out_color[4 * i] = hit_c.x; out_color[4 * i + 1] = hit_c.y; out_color[4 * i + 2] = hit_c.z; out_color[4 * i + 3] = 0; }
    if (out_weight) out_weight[i] = hit_w;
  }
}

static inline unsigned query_grid(uint32_t n) { const unsigned g = (n + 255u) / 256u; return g > 4096u ? 4096u : g; }

extern "C" int kf_map_sample_device(kf_ctx* c, uint32_t n, const double* dev_pos, float* dev_tsdf, float* dev_weight, float* dev_grad, uint8_t* dev_color) {
  if (!c || !dev_pos) return KF_ERR_ARG;
  if (!kf_whole_volume(c)) return KF_ERR_STATE;
  if (n == 0) return 0;
  KF_CHECK(hipSetDevice(c->cfg.device));
  const MapRef m = query_map(c);
  if (c->vol.color && dev_color) hipLaunchKernelGGL(k_map_sample<true>, dim3(query_grid(n)), dim3(256), 0, c->stream, m, n, dev_pos, dev_tsdf, dev_weight, dev_grad, dev_color);
  else hipLaunchKernelGGL(k_map_sample<false>, dim3(query_grid(n)), dim3(256), 0, c->stream, m, n, dev_pos, dev_tsdf, dev_weight, dev_grad, dev_color);
  return (int)hipGetLastError();
}

static inline bool query_cast_args_ok(float step, uint32_t max_steps) { return isfinite(step) && step > 0.f && max_steps >= 1u && max_steps <= KF_QUERY_MAX_STEPS; }

extern "C" int kf_map_cast_rays_device(kf_ctx* c, uint32_t n, const double* dev_origin, const float* dev_dir, const float* dev_tmin, const float* dev_tmax, float step,
                                       uint32_t max_steps, uint8_t* dev_status, float* dev_t, float* dev_normal, uint8_t* dev_color, float* dev_weight) {
  if (!c || !dev_origin || !dev_dir || !dev_tmin || !dev_tmax || !query_cast_args_ok(step, max_steps)) return KF_ERR_ARG;
  if (!kf_whole_volume(c)) return KF_ERR_STATE;
  if (n == 0) return 0;
  KF_CHECK(hipSetDevice(c->cfg.device));
  const MapRef m = query_map(c);
  if (c->vol.color && dev_color)
    hipLaunchKernelGGL(k_map_cast<true>, dim3(query_grid(n)), dim3(256), 0, c->stream, m, n, dev_origin, dev_dir, dev_tmin, dev_tmax, step, max_steps, dev_status, dev_t,
                       dev_normal, dev_color, dev_weight);
  else
    hipLaunchKernelGGL(k_map_cast<false>, dim3(query_grid(n)), dim3(256), 0, c->stream, m, n, dev_origin, dev_dir, dev_tmin, dev_tmax, step, max_steps, dev_status, dev_t,
                       dev_normal, dev_color, dev_weight);
  return (int)hipGetLastError();
}

extern "C" int kf_map_sample(kf_ctx* c, uint32_t n, const double* pos, float* tsdf, float* weight, float* grad, uint8_t* color) {
  if (!c || !pos) return KF_ERR_ARG;
  if (!kf_whole_volume(c)) return KF_ERR_STATE;
  if (n == 0) return 0;
  KF_CHECK(hipSetDevice(c->cfg.device));
  const size_t N = n, b_pos = 24 * N, b_f = 4 * N, b_g = 12 * N, b_c = 4 * N;
  KfCarveTemp tmp;
  if (!tmp.get(KfCarveTemp::pad(b_pos) + 2 * KfCarveTemp::pad(b_f) + KfCarveTemp::pad(b_g) + KfCarveTemp::pad(b_c))) return KF_ERR_ALLOC;
  const double* d_pos = tmp.up(c, pos, b_pos);
  float *d_t = tmp.down(tsdf, b_f), *d_w = tmp.down(weight, b_f), *d_g = tmp.down(grad, b_g);
  uint8_t* d_c = tmp.down(color, b_c);
  return tmp.finish(c, tmp.st ? tmp.st : kf_map_sample_device(c, n, d_pos, d_t, d_w, d_g, d_c));
}

extern "C" int kf_map_cast_rays(kf_ctx* c, uint32_t n, const double* origin, const float* dir, const float* tmin, const float* tmax, float step, uint32_t max_steps,
                                uint8_t* status, float* t, float* normal, uint8_t* color, float* weight) {
  if (!c || !origin || !dir || !tmin || !tmax || !query_cast_args_ok(step, max_steps)) return KF_ERR_ARG;
  if (!kf_whole_volume(c)) return KF_ERR_STATE;
  if (n == 0) return 0;
  KF_CHECK(hipSetDevice(c->cfg.device));
  const size_t N = n, b_o = 24 * N, b_d = 12 * N, b_f = 4 * N, b_s = N, b_c = 4 * N;
  KfCarveTemp tmp;
  if (!tmp.get(KfCarveTemp::pad(b_o) + 2 * KfCarveTemp::pad(b_d) + 4 * KfCarveTemp::pad(b_f) + KfCarveTemp::pad(b_s) + KfCarveTemp::pad(b_c))) return KF_ERR_ALLOC;
  const double* d_o = tmp.up(c, origin, b_o);
  const float *d_d = tmp.up(c, dir, b_d), *d_t0 = tmp.up(c, tmin, b_f), *d_t1 = tmp.up(c, tmax, b_f);
  uint8_t* d_s = tmp.down(status, b_s);
  float *d_t = tmp.down(t, b_f), *d_n = tmp.down(normal, b_d);
  uint8_t* d_c = tmp.down(color, b_c);
  float* d_w = tmp.down(weight, b_f);
  return tmp.finish(c, tmp.st ? tmp.st : kf_map_cast_rays_device(c, n, d_o, d_d, d_t0, d_t1, step, max_steps, d_s, d_t, d_n, d_c, d_w));
}
