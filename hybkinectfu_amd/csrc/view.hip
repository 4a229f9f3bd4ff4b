// view.hip -- viewer frames: the context's display image and the tracking camera's view of the model (reference: DataViewer::viewNormal /
// viewColors on the model normals and the raycast colours, src/HybKinectfu.cpp:152-157, src/DataViewer.cpp:13-44 -- there a blocking copy of the
// float4 maps and a loop on one host thread per picture).  The free viewpoint that marches the volume is kf_render_view (raycast.hip); both write
// the pixel function of view_pixel.h into the same context-owned image.
#include "kf_internal.h"
#include "view_pixel.h"

// The image is one allocation that only grows.  Growing frees the old one, which waits for the work that still reads or writes it.
int kf_view_reserve(kf_ctx* c, uint32_t cols, uint32_t rows, unsigned** img) {
  const size_t px = (size_t)cols * rows;
  if (px > c->view_cap_px) {
    if (c->view_img) { hipFree(c->view_img); c->view_img = nullptr; c->view_cap_px = 0; c->view_cols = c->view_rows = 0; }
    if (hipMalloc((void**)&c->view_img, px * sizeof(unsigned)) != hipSuccess) { c->view_img = nullptr; return KF_ERR_ALLOC; }
    c->view_cap_px = px;
  }
  c->view_cols = cols; c->view_rows = rows;
  *img = c->view_img;
  return 0;
}

// one pixel per lane over level 0 of the model maps; the eye is the device-resident pose's translation
template <int MODE>
__global__ void __launch_bounds__(256) k_view_maps(const float4* __restrict__ v, const float4* __restrict__ n, const uchar4* __restrict__ rgb,
                                                   const float* __restrict__ pose, unsigned* __restrict__ img, int npx) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= npx) return;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 vi = v[i];
  const float4 ni = MODE == KF_VIEW_COLOR ? z : n[i];
  const uchar4 ci = MODE == KF_VIEW_COLOR ? rgb[i] : make_uchar4(0, 0, 0, 0);
  img[i] = kf_view_pixel<MODE>(vi, ni, ci, kf3(pose[3], pose[7], pose[11]));
}

extern "C" int kf_view_model_maps(kf_ctx* c, int mode) {
  if (!c) return KF_ERR_ARG;
  if (mode != KF_VIEW_NORMALS && mode != KF_VIEW_SHADED && mode != KF_VIEW_COLOR) return KF_ERR_ARG;
  if (mode == KF_VIEW_COLOR && !c->raycast_rgb) return KF_ERR_STATE;
  unsigned* img = nullptr;
  { const int st = kf_view_reserve(c, (uint32_t)c->cols, (uint32_t)c->rows, &img); if (st) return st; }
  const int npx = c->cols * c->rows;
  const dim3 grid(kf_div_up(npx, 256)), block(256);
  const float4* v = c->model_v[0]; const float4* n = c->model_n[0]; const float* pose = c->track->pose;
  if (mode == KF_VIEW_NORMALS) hipLaunchKernelGGL(k_view_maps<KF_VIEW_NORMALS>, grid, block, 0, c->stream, v, n, (const uchar4*)c->raycast_rgb, pose, img, npx);
  else if (mode == KF_VIEW_SHADED) hipLaunchKernelGGL(k_view_maps<KF_VIEW_SHADED>, grid, block, 0, c->stream, v, n, (const uchar4*)c->raycast_rgb, pose, img, npx);
  else hipLaunchKernelGGL(k_view_maps<KF_VIEW_COLOR>, grid, block, 0, c->stream, v, n, (const uchar4*)c->raycast_rgb, pose, img, npx);
  return (int)hipGetLastError();
}

extern "C" int kf_view_size(kf_ctx* c, uint32_t* cols, uint32_t* rows) {
  if (!c) return KF_ERR_ARG;
  if (!c->view_cols) return KF_ERR_STATE;
  if (cols) *cols = c->view_cols;
  if (rows) *rows = c->view_rows;
  return 0;
}

extern "C" const uint8_t* kf_view_device(kf_ctx* c) { return (c && c->view_cols) ? (const uint8_t*)c->view_img : nullptr; }

extern "C" int kf_read_view(kf_ctx* c, uint8_t* dst, size_t dst_bytes) {
  if (!c || !dst) return KF_ERR_ARG;
  if (!c->view_cols) return KF_ERR_STATE;
  const size_t bytes = (size_t)c->view_cols * c->view_rows * 4;
  if (dst_bytes < bytes) return KF_ERR_ARG;
  KF_CHECK(hipMemcpyAsync(dst, c->view_img, bytes, hipMemcpyDeviceToHost, c->stream));
  KF_CHECK(hipStreamSynchronize(c->stream));
  return 0;
}
