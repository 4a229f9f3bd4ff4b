// hybkf_host.cpp -- implementation of the host classes in hybkf_host.hpp over the C ABI (libhybkf.so).
// Reference files followed: src/HybKinectfu.cpp, src/CameraPoseFinderICP.cpp, src/CameraPoseFinderSDF.cpp,
// src/utils/eigen_utils.cpp, src/MeshGeneratorMarchingcube.cpp, src/utils/mesh/meshData.{h,cpp}, src/utils/mesh/MeshIO.cpp.
#include "hybkf_host.hpp"
#include "map_file.hpp"
#include "erase_box_voxels.hpp"
#include "map_query_voxels.hpp"
#include "edt_box_voxels.hpp"
#include "mesh_parts.hpp"
#include <math.h>
#include <string.h>
#include <stdio.h>
#include <algorithm>
#include <exception>
#include <fstream>
#include <new>
#include <unordered_map>
#include <unordered_set>

// ---- AppParams --------------------------------------------------------------------------------------------------------
void AppParams::setDefaults(unsigned res, float size) {
  _switch_params = {false, false, false, true, true, false, false};
  _depth_camera_params = {640, 480, 319.5f, 239.5f, 525.0f, 525.0f};
  _rgb_camera_params = _depth_camera_params;
  _depth_prepocess_params = {4.0f, 0.3f, 0.03f, 2.0f};                  // max, min, sigma depth, sigma pixel
  _icp_params = {3, 0.1f, 0.1f, 0.3f, 0.3f};
  _sdf_tracker_params = {6, 0.3f, 0.3f};
  _volume_params = {res, size, 128.0f, 0.0f, 0u, 0u, false};
  _integrate_params = {0.05f, 2.0f};
  _raycast_params.fRayIncrement = 0.7f * _integrate_params.fSdfTruncation;  // AppParamsProducer.cpp:113-117
  _marchingcube_params.uMaxTriangles = 6500000;
}

// ---- Mat44 (src/cuda/Mat.h) ---------------------------------------------------------------------------------------------
Mat44 Mat44::getIdentity() { Mat44 m; memset(m.entries, 0, sizeof(m.entries)); m.entries[0] = m.entries[5] = m.entries[10] = m.entries[15] = 1.f; return m; }
Mat44 Mat44::operator*(const Mat44& o) const {
  Mat44 r;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j)
      r.entries[i * 4 + j] = entries[i * 4] * o.entries[j] + entries[i * 4 + 1] * o.entries[4 + j] + entries[i * 4 + 2] * o.entries[8 + j] + entries[i * 4 + 3] * o.entries[12 + j];
  return r;
}
#define T3(a, b, c) (e[a] * e[b] * e[c])
Mat44 Mat44::getInverse() const {                              // Mat.h:319-440
  const float* e = entries; float inv[16];
  inv[0] = T3(5, 10, 15) - T3(5, 11, 14) - T3(9, 6, 15) + T3(9, 7, 14) + T3(13, 6, 11) - T3(13, 7, 10);
  inv[4] = -T3(4, 10, 15) + T3(4, 11, 14) + T3(8, 6, 15) - T3(8, 7, 14) - T3(12, 6, 11) + T3(12, 7, 10);
  inv[8] = T3(4, 9, 15) - T3(4, 11, 13) - T3(8, 5, 15) + T3(8, 7, 13) + T3(12, 5, 11) - T3(12, 7, 9);
  inv[12] = -T3(4, 9, 14) + T3(4, 10, 13) + T3(8, 5, 14) - T3(8, 6, 13) - T3(12, 5, 10) + T3(12, 6, 9);
  inv[1] = -T3(1, 10, 15) + T3(1, 11, 14) + T3(9, 2, 15) - T3(9, 3, 14) - T3(13, 2, 11) + T3(13, 3, 10);
  inv[5] = T3(0, 10, 15) - T3(0, 11, 14) - T3(8, 2, 15) + T3(8, 3, 14) + T3(12, 2, 11) - T3(12, 3, 10);
  inv[9] = -T3(0, 9, 15) + T3(0, 11, 13) + T3(8, 1, 15) - T3(8, 3, 13) - T3(12, 1, 11) + T3(12, 3, 9);
  inv[13] = T3(0, 9, 14) - T3(0, 10, 13) - T3(8, 1, 14) + T3(8, 2, 13) + T3(12, 1, 10) - T3(12, 2, 9);
  inv[2] = T3(1, 6, 15) - T3(1, 7, 14) - T3(5, 2, 15) + T3(5, 3, 14) + T3(13, 2, 7) - T3(13, 3, 6);
  inv[6] = -T3(0, 6, 15) + T3(0, 7, 14) + T3(4, 2, 15) - T3(4, 3, 14) - T3(12, 2, 7) + T3(12, 3, 6);
  inv[10] = T3(0, 5, 15) - T3(0, 7, 13) - T3(4, 1, 15) + T3(4, 3, 13) + T3(12, 1, 7) - T3(12, 3, 5);
  inv[14] = -T3(0, 5, 14) + T3(0, 6, 13) + T3(4, 1, 14) - T3(4, 2, 13) - T3(12, 1, 6) + T3(12, 2, 5);
  inv[3] = -T3(1, 6, 11) + T3(1, 7, 10) + T3(5, 2, 11) - T3(5, 3, 10) - T3(9, 2, 7) + T3(9, 3, 6);
  inv[7] = T3(0, 6, 11) - T3(0, 7, 10) - T3(4, 2, 11) + T3(4, 3, 10) + T3(8, 2, 7) - T3(8, 3, 6);
  inv[11] = -T3(0, 5, 11) + T3(0, 7, 9) + T3(4, 1, 11) - T3(4, 3, 9) - T3(8, 1, 7) + T3(8, 3, 5);
  inv[15] = T3(0, 5, 10) - T3(0, 6, 9) - T3(4, 1, 10) + T3(4, 2, 9) + T3(8, 1, 6) - T3(8, 2, 5);
  float det = e[0] * inv[0] + e[1] * inv[4] + e[2] * inv[8] + e[3] * inv[12];
  float detr = 1.0f / det;
  Mat44 r;
  for (int i = 0; i < 16; ++i) r.entries[i] = inv[i] * detr;
  return r;
}
#undef T3
static kf_mat44 to_kf(const Mat44& m) { kf_mat44 k; memcpy(k.m, m.entries, 64); return k; }

// ---- small fp32 dense algebra (Eigen stand-ins for the host loop) --------------------------------------------------------
static void unpack27(const float* in, float A[36], float b[6]) {   // ICP.cpp:119-136
  int s = 0;
  for (int i = 0; i < 6; ++i) for (int j = i; j < 7; ++j) { float v = in[s++]; if (j == 6) b[i] = v; else { A[i * 6 + j] = v; A[j * 6 + i] = v; } }
}
static float det6(const float A[36]) {                            // partial-pivot LU, Eigen's 6x6 determinant() path
  float m[36]; memcpy(m, A, sizeof(m)); float det = 1.f;
  for (int k = 0; k < 6; ++k) {
    int p = k; float best = fabsf(m[k * 6 + k]);
    for (int r = k + 1; r < 6; ++r) { float v = fabsf(m[r * 6 + k]); if (v > best) { best = v; p = r; } }
    if (best == 0.f) return 0.f;
    if (p != k) { for (int c = 0; c < 6; ++c) std::swap(m[k * 6 + c], m[p * 6 + c]); det = -det; }
    float piv = m[k * 6 + k]; det *= piv;
    for (int r = k + 1; r < 6; ++r) { float f = m[r * 6 + k] / piv; for (int c = k + 1; c < 6; ++c) m[r * 6 + c] -= f * m[k * 6 + c]; }
  }
  return det;
}
static void llt_solve6(const float A[36], const float b[6], float x[6]) {
  float L[36]; memset(L, 0, sizeof(L));
  for (int j = 0; j < 6; ++j) {
    float s = A[j * 6 + j]; for (int k = 0; k < j; ++k) s -= L[j * 6 + k] * L[j * 6 + k];
    float d = sqrtf(s); L[j * 6 + j] = d;
    for (int i = j + 1; i < 6; ++i) { float t = A[i * 6 + j]; for (int k = 0; k < j; ++k) t -= L[i * 6 + k] * L[j * 6 + k]; L[i * 6 + j] = t / d; }
  }
  float y[6];
  for (int i = 0; i < 6; ++i) { float t = b[i]; for (int k = 0; k < i; ++k) t -= L[i * 6 + k] * y[k]; y[i] = t / L[i * 6 + i]; }
  for (int i = 5; i >= 0; --i) { float t = y[i]; for (int k = i + 1; k < 6; ++k) t -= L[k * 6 + i] * x[k]; x[i] = t / L[i * 6 + i]; }
}
// R = Rx(x0) Ry(x1) Rz(x2); rotation angle of R (== Eigen AngleAxisf(R).angle()) and |t| against the shake limits
static bool euler_increment(const float x[6], float dist_shake, float angle_shake, Mat44& out) {
  float c0 = cosf(x[0]), s0 = sinf(x[0]), c1 = cosf(x[1]), s1 = sinf(x[1]), c2 = cosf(x[2]), s2 = sinf(x[2]);
  float Rx[9] = {1, 0, 0, 0, c0, -s0, 0, s0, c0}, Ry[9] = {c1, 0, s1, 0, 1, 0, -s1, 0, c1}, Rz[9] = {c2, -s2, 0, s2, c2, 0, 0, 0, 1};
  float Rxy[9], R[9];
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) Rxy[r * 3 + c] = Rx[r * 3] * Ry[c] + Rx[r * 3 + 1] * Ry[3 + c] + Rx[r * 3 + 2] * Ry[6 + c];
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R[r * 3 + c] = Rxy[r * 3] * Rz[c] + Rxy[r * 3 + 1] * Rz[3 + c] + Rxy[r * 3 + 2] * Rz[6 + c];
  float ca = (R[0] + R[4] + R[8] - 1.f) * 0.5f; ca = ca > 1.f ? 1.f : (ca < -1.f ? -1.f : ca);
  float angle = acosf(ca), d = sqrtf(x[3] * x[3] + x[4] * x[4] + x[5] * x[5]);
  if (angle > angle_shake || d > dist_shake) return false;
  out = Mat44::getIdentity();
  for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) out.entries[r * 4 + c] = R[r * 3 + c]; out.entries[r * 4 + 3] = x[3 + r]; }
  return true;
}

// ---- CudaDeviceDataMan ------------------------------------------------------------------------------------------------------
bool CudaDeviceDataMan::init() {
  release();
  const AppParams* p = AppParams::instance();
  kf_config cfg; memset(&cfg, 0, sizeof(cfg));
  cfg.depth_camera = p->_depth_camera_params; cfg.rgb_camera = p->_rgb_camera_params;
  cfg.volume.resolution = p->_volume_params.nResolution; cfg.volume.size_m = p->_volume_params.fVolumeMeterSize; cfg.volume.max_weight = p->_volume_params.fWeightMax;
  cfg.pyramid_levels = p->_icp_params.nPyramidLevels; cfg.max_triangles = p->_marchingcube_params.uMaxTriangles;
  cfg.has_color = p->_switch_params.useRGBData ? 1 : 0; cfg.device = p->device;
  cfg.slab_z_begin = p->slab_z_begin; cfg.slab_z_end = p->slab_z_end; cfg.slab_halo = p->slab_halo;
  _err = kf_create(&cfg, &_ctx);
  return _err == 0;
}
void CudaDeviceDataMan::release() { if (_ctx) { kf_destroy(_ctx); _ctx = nullptr; } }

// ---- CameraPoseFinder (src/CameraPoseFinder.h:15-43) ---------------------------------------------------------------------------
bool CameraPoseFinder::init(const Mat44& reference_transform) {
  if (_inited) return false;
  _pose = reference_transform;
  if (!initPoseFinder()) return false;
  kf_mat44 k = to_kf(_pose);
  if (CudaDeviceDataMan::instance()->check(kf_set_pose(CudaDeviceDataMan::instance()->ctx(), &k))) return false;
  _inited = true;
  return _inited;
}
bool CameraPoseFinder::findCameraPose(const DepthFrameData& d, const ColorFrameData& c) {
  if (!_inited) return false;
  return estimateCameraPose(d, c);
}
void CameraPoseFinder::setCameraPose(const Mat44& t) {
  _pose = t;
  kf_mat44 k = to_kf(_pose);
  CudaDeviceDataMan::instance()->check(kf_set_pose(CudaDeviceDataMan::instance()->ctx(), &k));
}
bool CameraPoseFinder::enqueueCameraPose(const DepthFrameData& d) { return _inited && enqueueEstimate(d); }
bool CameraPoseFinder::enqueueEstimate(const DepthFrameData& d) {   // default for two-virtual plugins (src/CameraPoseFinder.h:38-39)
  ColorFrameData none;
  if (!estimateCameraPose(d, none)) return false;
  setCameraPose(_pose);                                              // publish pose + "tracked" to the device-resident state
  return true;
}
bool CameraPoseFinder::requestPose() {
  return !CudaDeviceDataMan::instance()->check(kf_request_track_result(CudaDeviceDataMan::instance()->ctx()));
}
bool CameraPoseFinder::waitPose() {
  kf_track_result r;
  if (CudaDeviceDataMan::instance()->check(kf_wait_track_result(CudaDeviceDataMan::instance()->ctx(), &r))) return false;
  memcpy(_pose.entries, r.pose.m, 64);
  return r.tracked != 0;
}
bool CameraPoseFinder::syncPose() {
  kf_track_result r;
  if (CudaDeviceDataMan::instance()->check(kf_read_track_result(CudaDeviceDataMan::instance()->ctx(), &r))) return false;
  memcpy(_pose.entries, r.pose.m, 64);
  return r.tracked != 0;
}

// ---- CameraPoseFinderICP (src/CameraPoseFinderICP.cpp) ---------------------------------------------------------------------------
bool CameraPoseFinderICP::initPoseFinder() {                    // :12-49
  unsigned levels = AppParams::instance()->_icp_params.nPyramidLevels;
  _iter_nums.resize(levels);
  if (levels == 1) { _iter_nums[0] = 3; }
  else if (levels == 2) { _iter_nums[0] = 10; _iter_nums[1] = 5; }
  else if (levels == 3) { _iter_nums[0] = 10; _iter_nums[1] = 5; _iter_nums[2] = 4; }
  else return false;
  _camera_params_pyramid.clear();
  _camera_params_pyramid.push_back(AppParams::instance()->_depth_camera_params);
  for (unsigned l = 1; l < levels; l++) {
    CameraParams cur, prev = _camera_params_pyramid[l - 1];
    cur.cols = prev.cols / 2; cur.rows = prev.rows / 2; cur.cx = prev.cx / 2; cur.cy = prev.cy / 2; cur.fx = prev.fx / 2; cur.fy = prev.fy / 2;
    _camera_params_pyramid.push_back(cur);
  }
  return true;
}
bool CameraPoseFinderICP::enqueueEstimate(const DepthFrameData& depth_frame) {
  const IcpParams& ip = AppParams::instance()->_icp_params;
  kf_icp_params k = {ip.nPyramidLevels, ip.fNormSinThres, ip.fDistThres, ip.fDistShake, ip.fAngleShake};
  return 0 == CudaDeviceDataMan::instance()->check(kf_icp_track(CudaDeviceDataMan::instance()->ctx(), depth_frame.frameId(), &k,
                                                                &AppParams::instance()->_depth_camera_params));
}
bool CameraPoseFinderICP::estimateCameraPose(const DepthFrameData& depth_frame, const ColorFrameData&) {   // :50-94
  if (!_host_loop) return enqueueEstimate(depth_frame) && syncPose();
  if (depth_frame.frameId() == 0) return true;
  kf_ctx* ctx = CudaDeviceDataMan::instance()->ctx();
  kf_downsample_new_vertices(ctx); kf_downsample_new_normals(ctx); kf_downsample_model_vertices(ctx); kf_downsample_model_normals(ctx);
  Mat44 cur_transform = _pose, last_transform_inv = _pose.getInverse();
  float delta_dof[6];
  for (int l = (int)_iter_nums.size() - 1; l >= 0; l--) {
    int it_nums = _iter_nums[l];
    while (it_nums--) {
      if (!minimizePointToPlaneErrFunc(l, delta_dof, cur_transform, last_transform_inv)) return false;
      Mat44 t;
      if (!vector6ToTransformMatrix(delta_dof, t)) return false;   // "camera shaking detected"
      cur_transform = t * cur_transform;
    }
  }
  setCameraPose(cur_transform);
  return true;
}
bool CameraPoseFinderICP::vector6ToTransformMatrix(const float x[6], Mat44& output) {   // :95-111
  return euler_increment(x, AppParams::instance()->_icp_params.fDistShake, AppParams::instance()->_icp_params.fAngleShake, output);
}
bool CameraPoseFinderICP::minimizePointToPlaneErrFunc(unsigned level, float six_dof[6], const Mat44& cur, const Mat44& last_inv) {   // :113-145
  kf_ctx* ctx = CudaDeviceDataMan::instance()->ctx();
  kf_mat44 kc = to_kf(cur), kl = to_kf(last_inv);
  if (kf_cal_point_to_plane_solver_params(ctx, level, &kc, &kl, &_camera_params_pyramid[level], AppParams::instance()->_icp_params.fDistThres,
                                          AppParams::instance()->_icp_params.fNormSinThres)) return false;
  float buf[27], A[36], b[6];
  if (kf_read_solver_params(ctx, buf)) return false;
  unpack27(buf, A, b);
  if (det6(A) < 1E-10) return false;
  llt_solve6(A, b, six_dof);
  return true;
}

// ---- CameraPoseFinderSDF (src/CameraPoseFinderSDF.cpp, src/utils/eigen_utils.cpp) ---------------------------------------------------
bool CameraPoseFinderSDF::initPoseFinder() { return true; }
bool CameraPoseFinderSDF::vector6ToTransformMatrix(const float x[6], Mat44& output) {
  return euler_increment(x, AppParams::instance()->_sdf_tracker_params.fDistShake, AppParams::instance()->_sdf_tracker_params.fAngleShake, output);
}
bool CameraPoseFinderSDF::enqueueEstimate(const DepthFrameData& depth_frame) {
  const SDFTrackerParams& sp = AppParams::instance()->_sdf_tracker_params;
  kf_sdf_tracker_params k = {sp.maxIterNums, sp.fDistShake, sp.fAngleShake};
  return 0 == CudaDeviceDataMan::instance()->check(kf_sdf_track(CudaDeviceDataMan::instance()->ctx(), depth_frame.frameId(), &k,
                                                                &AppParams::instance()->_depth_camera_params));
}
static void exp_map(const double v[6], double R[9], double dt[3]) {   // eigen_utils.cpp:60-127
  double u0 = v[0], u1 = v[1], u2 = v[2];
  double theta = sqrt(u0 * u0 + u1 * u1 + u2 * u2), si = sin(theta), co = cos(theta);
  double sinc = fabs(theta) < 1.0e-8 ? 1.0 : si / theta;
  double mcosc = fabs(theta) < 2.5e-4 ? 0.5 : (1.0 - co) / theta / theta;
  double msinc = fabs(theta) < 2.5e-4 ? (1. / 6.0) : (1.0 - si / theta) / theta / theta;
  R[0] = co + mcosc * u0 * u0; R[1] = -sinc * u2 + mcosc * u0 * u1; R[2] = sinc * u1 + mcosc * u0 * u2;
  R[3] = sinc * u2 + mcosc * u1 * u0; R[4] = co + mcosc * u1 * u1; R[5] = -sinc * u0 + mcosc * u1 * u2;
  R[6] = -sinc * u1 + mcosc * u2 * u0; R[7] = sinc * u0 + mcosc * u2 * u1; R[8] = co + mcosc * u2 * u2;
  dt[0] = v[3] * (sinc + u0 * u0 * msinc) + v[4] * (u0 * u1 * msinc - u2 * mcosc) + v[5] * (u0 * u2 * msinc + u1 * mcosc);
  dt[1] = v[3] * (u0 * u1 * msinc + u2 * mcosc) + v[4] * (sinc + u1 * u1 * msinc) + v[5] * (u1 * u2 * msinc - u0 * mcosc);
  dt[2] = v[3] * (u0 * u2 * msinc - u1 * mcosc) + v[4] * (u1 * u2 * msinc + u0 * mcosc) + v[5] * (sinc + u2 * u2 * msinc);
}
bool CameraPoseFinderSDF::estimateCameraPose(const DepthFrameData& depth_frame, const ColorFrameData&) {   // :44-106
  if (!_host_loop) return enqueueEstimate(depth_frame) && syncPose();
  if (depth_frame.frameId() == 0) return true;
  kf_ctx* ctx = CudaDeviceDataMan::instance()->ctx();
  unsigned iter = 0; const float e = 0.001f;
  Mat44 cur = _pose;
  while (iter < AppParams::instance()->_sdf_tracker_params.maxIterNums) {
    kf_mat44 kc = to_kf(cur);
    float buf[27], A[36], b[6], x[6];
    if (kf_cal_sdf_solver_params(ctx, &AppParams::instance()->_depth_camera_params, &kc) || kf_read_solver_params(ctx, buf)) return false;
    unpack27(buf, A, b);
    llt_solve6(A, b, x);
    Mat44 t;
    if (!vector6ToTransformMatrix(x, t)) return false;
    float nx = sqrtf(x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3] + x[4] * x[4] + x[5] * x[5]);
    if (nx < e) break;
    double xd[6], R[9], dt[3];
    for (int k = 0; k < 6; ++k) xd[k] = (double)x[k];
    exp_map(xd, R, dt);
    Mat44 n = Mat44::getIdentity();
    for (int r = 0; r < 3; ++r) {
      float rt = 0.f;
      for (int c = 0; c < 3; ++c) n.entries[r * 4 + c] = (float)R[0 * 3 + r] * cur.entries[c] + (float)R[1 * 3 + r] * cur.entries[4 + c] + (float)R[2 * 3 + r] * cur.entries[8 + c];
      rt = (float)R[0 * 3 + r] * (float)dt[0] + (float)R[1 * 3 + r] * (float)dt[1] + (float)R[2 * 3 + r] * (float)dt[2];
      n.entries[r * 4 + 3] = cur.entries[r * 4 + 3] - rt;
    }
    cur = n;
    iter++;
  }
  setCameraPose(cur);
  return true;
}

// ---- HybKinectfu (src/HybKinectfu.cpp) ---------------------------------------------------------------------------------------------
HybKinectfu::HybKinectfu() : _camera_pose_finder(nullptr), _inited(false) {}
HybKinectfu::~HybKinectfu() { delete _camera_pose_recorder; _camera_pose_recorder = nullptr; delete _camera_pose_finder; _camera_pose_finder = nullptr; }

bool HybKinectfu::init() {                                     // :28-61
  if (_inited) return false;
  if (!CudaDeviceDataMan::instance()->ctx() && !CudaDeviceDataMan::instance()->init()) return false;
  if (AppParams::instance()->_switch_params.useTrajFromFile) _camera_pose_finder = new CameraPoseFinderFromFile();
  else if (AppParams::instance()->_switch_params.useSdfTracker) _camera_pose_finder = new CameraPoseFinderSDF();
  else _camera_pose_finder = new CameraPoseFinderICP();
  if (AppParams::instance()->_switch_params.recordTrajectory)
    _camera_pose_recorder = new TrajectoryRecorder(AppParams::instance()->_io_params.trajWriteFilename);
  Mat44 camera_pose0 = Mat44::getIdentity();
  camera_pose0.setTranslation((float)(AppParams::instance()->_volume_params.fVolumeMeterSize / 2.0),
                              (float)(AppParams::instance()->_volume_params.fVolumeMeterSize / 2.0),
                              -AppParams::instance()->_depth_prepocess_params.fMinTrunc);
  if (!_camera_pose_finder->init(camera_pose0)) return false;
  _inited = true;
  if (AppParams::instance()->_volume_params.nStreamMeshTriangles > 0 && !setStreamMesh(AppParams::instance()->_volume_params.nStreamMeshTriangles)) _inited = false;
  if (_inited && AppParams::instance()->_volume_params.nBrickStoreBricks > 0 && !setBrickStore(AppParams::instance()->_volume_params.nBrickStoreBricks)) _inited = false;
  return _inited;
}

void HybKinectfu::copyFrameToGPU(const DepthFrameData& d, const ColorFrameData& c) {   // :63-96 (the u16 -> f32 conversion runs on the device)
  CudaDeviceDataMan* dm = CudaDeviceDataMan::instance();
  if (d.on_device) dm->check(kf_set_depth_mm_device(dm->ctx(), d.mm, d.cols, d.rows));
  else dm->check(kf_upload_depth_mm(dm->ctx(), d.mm, d.cols, d.rows));
  if (AppParams::instance()->_switch_params.useRGBData && c.bgr) dm->check(kf_upload_rgb(dm->ctx(), c.bgr, c.cols, c.rows));
}

bool HybKinectfu::enqueueFrame(const DepthFrameData& depth_frame, const ColorFrameData& rgb_frame) {
  if (!_inited) return false;
  const AppParams* p = AppParams::instance();
  CudaDeviceDataMan* dm = CudaDeviceDataMan::instance();
  kf_ctx* ctx = dm->ctx();
  // a finder that computes its pose on the host (file-driven, or a plugin with the reference's two virtuals) has no streaming
  // form: the frame takes the reference's own sequence, which also handles a lost frame (no integrate, raycast with the old pose)
  if (!_camera_pose_finder->deviceResident()) return processNewFrame(depth_frame, rgb_frame);
  _frame_id = depth_frame.frameId();
  copyFrameToGPU(depth_frame, rgb_frame);
  if (dm->check(kf_preprocess(ctx, p->_depth_prepocess_params.fMinTrunc, p->_depth_prepocess_params.fMaxTrunc, p->_depth_prepocess_params.fSigmaPixel,
                              p->_depth_prepocess_params.fSigmaDepth, &p->_depth_camera_params))) return false;      // :106-110
  if (!_camera_pose_finder->enqueueCameraPose(depth_frame)) return false;                                            // :116
  _pending = true;
  kf_integrate_params ip = {p->_integrate_params.fSdfTruncation, p->_integrate_params.fMaxIntegrateDist};
  if (dm->check(kf_integrate_volume(ctx, p->_switch_params.useRGBData, p->_switch_params.colorAngleWeight, nullptr, &ip,
                                    &p->_depth_camera_params, &p->_rgb_camera_params))) return false;                // :125-140, predicated on device
  kf_raycast_params rp = {p->_raycast_params.fRayIncrement};
  if (dm->check(kf_raycast_volume(ctx, p->_switch_params.useRGBData, nullptr, &rp, &p->_depth_camera_params,
                                  p->_depth_prepocess_params.fMinTrunc, p->_depth_prepocess_params.fMaxTrunc))) return false;   // :149-154
  return true;
}

bool HybKinectfu::processNewFrame(const DepthFrameData& depth_frame, const ColorFrameData& rgb_frame) {   // :98-160
  if (!_inited) return false;
  const AppParams* p = AppParams::instance();
  CudaDeviceDataMan* dm = CudaDeviceDataMan::instance();
  kf_ctx* ctx = dm->ctx();
  _frame_id = depth_frame.frameId();
  copyFrameToGPU(depth_frame, rgb_frame);
  if (dm->check(kf_preprocess(ctx, p->_depth_prepocess_params.fMinTrunc, p->_depth_prepocess_params.fMaxTrunc, p->_depth_prepocess_params.fSigmaPixel,
                              p->_depth_prepocess_params.fSigmaDepth, &p->_depth_camera_params))) return false;
  if (_camera_pose_finder->deviceResident()) {
    // Same results as the sequence below, without a bubble: the verdict is requested right behind the tracker, integrate and
    // raycast are enqueued with the device-resident pose (integrate is predicated on the verdict inside the kernel, :123; a lost
    // frame leaves the pose untouched, so the raycast sees what getCameraPose() would have returned), and only then does the
    // host wait -- for the tracker's result, not for the rest of the frame.
    if (!_camera_pose_finder->enqueueCameraPose(depth_frame) || !_camera_pose_finder->requestPose()) return false;
    kf_integrate_params ip = {p->_integrate_params.fSdfTruncation, p->_integrate_params.fMaxIntegrateDist};
    if (dm->check(kf_integrate_volume(ctx, p->_switch_params.useRGBData, p->_switch_params.colorAngleWeight, nullptr, &ip,
                                      &p->_depth_camera_params, &p->_rgb_camera_params))) return false;
    kf_raycast_params rp = {p->_raycast_params.fRayIncrement};
    if (dm->check(kf_raycast_volume(ctx, p->_switch_params.useRGBData, nullptr, &rp, &p->_depth_camera_params,
                                    p->_depth_prepocess_params.fMinTrunc, p->_depth_prepocess_params.fMaxTrunc))) return false;
    _last_tracked = _camera_pose_finder->waitPose(); _pending = false;
    if (_last_tracked && _camera_pose_recorder) _camera_pose_recorder->recordCameraPose(worldPose(_camera_pose_finder->getCameraPose()), depth_frame.timeStamp());
    if (_last_tracked && p->_volume_params.fRecentreDist > 0.f) return recentre();
    return true;
  }
  bool camera_tracking_success = _camera_pose_finder->findCameraPose(depth_frame, rgb_frame);
  _last_tracked = camera_tracking_success; _pending = false;
  Mat44 cur_camera_pose = _camera_pose_finder->getCameraPose();
  kf_mat44 kp = to_kf(cur_camera_pose);
  if (camera_tracking_success) {
    if (_camera_pose_recorder) _camera_pose_recorder->recordCameraPose(worldPose(cur_camera_pose), depth_frame.timeStamp());     // :129-132
    kf_integrate_params ip = {p->_integrate_params.fSdfTruncation, p->_integrate_params.fMaxIntegrateDist};
    if (dm->check(kf_integrate_volume(ctx, p->_switch_params.useRGBData, p->_switch_params.colorAngleWeight, &kp, &ip,
                                      &p->_depth_camera_params, &p->_rgb_camera_params))) return false;
  }                                                            // else: "camera lost" -- the reference blocks on cv::waitKey(); we never block
  kf_raycast_params rp = {p->_raycast_params.fRayIncrement};
  if (dm->check(kf_raycast_volume(ctx, p->_switch_params.useRGBData, &kp, &rp, &p->_depth_camera_params,
                                  p->_depth_prepocess_params.fMinTrunc, p->_depth_prepocess_params.fMaxTrunc))) return false;
  if (camera_tracking_success && p->_volume_params.fRecentreDist > 0.f) return recentre();
  return true;
}
// ---- the moving volume ------------------------------------------------------------------------------------------------------------------
static float volume_cell() {                                   // KfVolume::cell: the fp32 quotient (tsdfVolume.h:44-46)
  const AppParams* p = AppParams::instance();
  return p->_volume_params.fVolumeMeterSize / (float)p->_volume_params.nResolution;
}
void HybKinectfu::volumeOrigin(int out[3]) {
  int32_t o[3] = {0, 0, 0};
  CudaDeviceDataMan* dm = CudaDeviceDataMan::instance();
  if (dm->ctx()) dm->check(kf_volume_origin(dm->ctx(), o));
  for (int k = 0; k < 3; ++k) out[k] = (int)o[k];
}
Mat44 HybKinectfu::worldPose(const Mat44& pose) {
  int o[3]; volumeOrigin(o);
  const int32_t o32[3] = {o[0], o[1], o[2]};
  Mat44 w = pose;
  hkf_world_pose(w.entries, o32, volume_cell());
  return w;
}
bool HybKinectfu::shiftVolume(int dx, int dy, int dz) {
  if (!_inited) return false;
  const AppParams* p = AppParams::instance();
  CudaDeviceDataMan* dm = CudaDeviceDataMan::instance();
  if (dm->check(kf_shift_volume(dm->ctx(), dx, dy, dz))) return false;
  if (dx == 0 && dy == 0 && dz == 0) return true;
  const float cell = volume_cell();
  Mat44 moved = _camera_pose_finder->getCameraPose();           // the same expression as k_shift_pose
  moved.entries[3] = moved.entries[3] - (float)dx * cell;
  moved.entries[7] = moved.entries[7] - (float)dy * cell;
  moved.entries[11] = moved.entries[11] - (float)dz * cell;
  const bool resident = _camera_pose_finder->deviceResident();
  if (resident) _camera_pose_finder->adoptCameraPose(moved); else _camera_pose_finder->setCameraPose(moved);
  const kf_mat44 kp = to_kf(moved);
  kf_raycast_params rp = {p->_raycast_params.fRayIncrement};
  return 0 == dm->check(kf_raycast_volume(dm->ctx(), p->_switch_params.useRGBData, resident ? nullptr : &kp, &rp, &p->_depth_camera_params,
                                          p->_depth_prepocess_params.fMinTrunc, p->_depth_prepocess_params.fMaxTrunc));
}
static float mesh_threshold() {                                // MeshGeneratorMarchingcube.cpp:23-29
  const AppParams* p = AppParams::instance();
  return 300 * p->_volume_params.fVolumeMeterSize / p->_volume_params.nResolution;
}
bool HybKinectfu::setStreamMesh(unsigned max_triangles) {
  if (!_inited) return false;
  AppParams* p = AppParams::instance();
  CudaDeviceDataMan* dm = CudaDeviceDataMan::instance();
  p->_volume_params.nStreamMeshTriangles = max_triangles;
  if (dm->check(kf_world_soup_reserve(dm->ctx(), max_triangles))) { p->_volume_params.nStreamMeshTriangles = 0; return false; }
  if (max_triangles == 0) return true;
  if (dm->check(kf_set_stream_out(dm->ctx(), 1, p->_switch_params.useRGBData, mesh_threshold()))) { p->_volume_params.nStreamMeshTriangles = 0; return false; }
  return true;
}
unsigned HybKinectfu::worldSoupCount() {
  uint32_t n = 0; CudaDeviceDataMan* dm = CudaDeviceDataMan::instance();
  if (dm->ctx()) dm->check(kf_world_soup_count(dm->ctx(), &n, nullptr));
  return n;
}
bool HybKinectfu::setBrickStore(unsigned max_bricks) {
  if (!_inited) return false;
  AppParams* p = AppParams::instance();
  CudaDeviceDataMan* dm = CudaDeviceDataMan::instance();
  p->_volume_params.nBrickStoreBricks = max_bricks;
  if (dm->check(kf_brick_store_reserve(dm->ctx(), max_bricks))) { p->_volume_params.nBrickStoreBricks = 0; return false; }
  return true;
}
bool HybKinectfu::brickStoreCounts(unsigned& held, uint64_t& dropped, uint64_t& restored) {
  held = 0; dropped = 0; restored = 0;
  CudaDeviceDataMan* dm = CudaDeviceDataMan::instance();
  if (!dm->ctx()) return false;
  uint32_t h = 0;
  if (dm->check(kf_brick_store_count(dm->ctx(), &h, &dropped, &restored))) return false;
  held = h;
  return true;
}
// ---- the map on disk (map_file.hpp) ---------------------------------------------------------------------------------------------------------
static const uint32_t kMapChunkBricks = 256;                   // bricks per kf_read_brick_store / kf_write_brick_store call: 1.4 MiB of host memory
bool HybKinectfu::saveMap(const std::string& path) {
  if (!_inited) return false;
  const AppParams* p = AppParams::instance();
  CudaDeviceDataMan* dm = CudaDeviceDataMan::instance();
  kf_ctx* ctx = dm->ctx();
  uint32_t held = 0; uint64_t dropped_before = 0, dropped = 0;
  if (dm->check(kf_brick_store_count(ctx, nullptr, &dropped_before, nullptr))) return false;
  if (dm->check(kf_brick_store_capture(ctx))) return false;    // KF_ERR_STATE without a store
  if (dm->check(kf_brick_store_count(ctx, &held, &dropped, nullptr))) return false;
  if (dropped != dropped_before) {
    fprintf(stderr, "saveMap: the brick store is full: %llu bricks of the window did not fit; nothing written\n", (unsigned long long)(dropped - dropped_before));
    return false;
  }
  if (dropped) fprintf(stderr, "saveMap: the brick store has dropped %llu bricks for want of room: the map has holes there\n", (unsigned long long)dropped);
  HkfMapHeader h;
  memset(&h, 0, sizeof(h));
  h.resolution = p->_volume_params.nResolution; h.has_color = p->_switch_params.useRGBData ? 1u : 0u;
  h.size_m = p->_volume_params.fVolumeMeterSize; h.max_weight = p->_volume_params.fWeightMax;
  int o[3]; volumeOrigin(o);
  for (int k = 0; k < 3; ++k) h.origin_vox[k] = o[k];
  h.frame_id = _frame_id;
  Mat44 pose = getCameraPose();                                 // (waits for a pending verdict)
  if (_camera_pose_finder->deviceResident()) {                  // the device holds the pose: a window placed behind the host's back has moved it there only
    kf_track_result r;
    if (dm->check(kf_read_track_result(ctx, &r))) return false;
    memcpy(pose.entries, r.pose.m, 64);
  }
  memcpy(h.pose, pose.entries, 64);
  h.n_bricks = held; h.dropped = dropped;
  const bool color = h.has_color != 0;
  const int st = hkf_map_write(path.c_str(), h, kMapChunkBricks, [&](uint32_t first, uint32_t count, int32_t* keys, float* tsdf, float* weight, uint8_t* col) {
    return 0 == dm->check(kf_read_brick_store(ctx, first, count, keys, tsdf, weight, color ? col : nullptr));
  });
  if (st != HKF_MAP_OK) fprintf(stderr, "saveMap: writing %s failed (%d)\n", path.c_str(), st);
  return st == HKF_MAP_OK;
}
bool HybKinectfu::loadMap(const std::string& path) {
  if (!_inited) return false;
  AppParams* p = AppParams::instance();
  CudaDeviceDataMan* dm = CudaDeviceDataMan::instance();
  kf_ctx* ctx = dm->ctx();
  HkfMapHeader h;
  bool store_ok = true, touched = false;
  lastTracked();                                                // a frame still in flight settles first: afterwards the loaded pose is the one that counts
  const HkfMapAccept accept = [&](const HkfMapHeader& f) {      // the whole file has passed the reader's checks; nothing is touched before this returns true
    if (f.resolution != p->_volume_params.nResolution || memcmp(&f.size_m, &p->_volume_params.fVolumeMeterSize, 4) != 0 ||
        memcmp(&f.max_weight, &p->_volume_params.fWeightMax, 4) != 0 || (f.has_color != 0) != p->_switch_params.useRGBData) return false;
    h = f;
    touched = true;                                            // from here on a failure leaves an EMPTY map: see below
    if (dm->check(kf_reset_volume(ctx))) { store_ok = false; return false; }
    const uint64_t want = f.n_bricks > p->_volume_params.nBrickStoreBricks ? f.n_bricks : p->_volume_params.nBrickStoreBricks;
    store_ok = setBrickStore((unsigned)(want ? want : 1u));   // (a store of one brick for an empty map: kf_place_window needs a store)
    return store_ok;
  };
  const int st = hkf_map_read(path.c_str(), kMapChunkBricks, accept, [&](uint32_t count, const int32_t* keys, const float* tsdf, const float* weight, const uint8_t* col) {
    return 0 == dm->check(kf_write_brick_store(ctx, count, keys, tsdf, weight, col));
  });
  if (st != HKF_MAP_OK) {
    fprintf(stderr, "loadMap: %s refused (%d)%s\n", path.c_str(), st, st == HKF_MAP_ERR_REFUSED && store_ok ? ": its volume is not this instance's" : "");
    // The file was checked as a whole before anything was touched, so a failure past that point is a read error or a device error.  It must not leave a
    // partly filled store under an empty window: volume and store are reset once more.  The host's pose and frame id are still the old session's.
    if (touched) dm->check(kf_reset_volume(ctx));
    return false;
  }
  if (dm->check(kf_place_window(ctx, h.origin_vox[0], h.origin_vox[1], h.origin_vox[2]))) { dm->check(kf_reset_volume(ctx)); return false; }
  Mat44 pose; memcpy(pose.entries, h.pose, 64);
  _camera_pose_finder->setCameraPose(pose);                    // host copy and device-resident pose (kf_set_pose: "tracked")
  _frame_id = h.frame_id; _last_tracked = true; _pending = false;
  const bool resident = _camera_pose_finder->deviceResident();
  const kf_mat44 kp = to_kf(pose);
  kf_raycast_params rp = {p->_raycast_params.fRayIncrement};  // shiftVolume's raycast: the model maps show the loaded window before the next frame is tracked
  return 0 == dm->check(kf_raycast_volume(ctx, p->_switch_params.useRGBData, resident ? nullptr : &kp, &rp, &p->_depth_camera_params,
                                          p->_depth_prepocess_params.fMinTrunc, p->_depth_prepocess_params.fMaxTrunc));
}
// the file's status and header against this instance's volume: resolution, size, max weight and colour flag
static bool merge_file_is_ours(const std::string& path, int is, const HkfMapHeader& h) {
  const AppParams* p = AppParams::instance();
  if (is != HKF_MAP_OK || h.resolution != p->_volume_params.nResolution || memcmp(&h.size_m, &p->_volume_params.fVolumeMeterSize, 4) != 0 ||
      memcmp(&h.max_weight, &p->_volume_params.fWeightMax, 4) != 0 || (h.has_color != 0) != p->_switch_params.useRGBData) {
    fprintf(stderr, "mergeMap: %s refused (%d)%s\n", path.c_str(), is, is == HKF_MAP_OK ? ": its volume is not this instance's" : "");
    return false;
  }
  return true;
}
bool HybKinectfu::mergeMakeRoom(bool color, uint64_t incoming) {
  AppParams* p = AppParams::instance();
  CudaDeviceDataMan* dm = CudaDeviceDataMan::instance();
  kf_ctx* ctx = dm->ctx();
  // a store that was never reserved: room for whatever the capture may bring (every brick of the window); the incoming bricks are added below
  if (p->_volume_params.nBrickStoreBricks == 0) {
    const uint64_t nb = p->_volume_params.nResolution / 8u;
    if (!setBrickStore((unsigned)(nb * nb * nb))) return false;
  }
  // the window into the store: afterwards the store alone is this session's map
  uint32_t held = 0; uint64_t dropped_before = 0, dropped = 0;
  if (dm->check(kf_brick_store_count(ctx, nullptr, &dropped_before, nullptr))) return false;
  if (dm->check(kf_brick_store_capture(ctx))) return false;
  if (dm->check(kf_brick_store_count(ctx, &held, &dropped, nullptr))) return false;
  if (dropped != dropped_before) {
    fprintf(stderr, "mergeMap: the brick store is full: %llu bricks of the window did not fit; nothing merged\n", (unsigned long long)(dropped - dropped_before));
    return false;
  }
  // room for every incoming brick (all of them new, at worst): the store read out, reserved larger, written back -- the bricks verbatim, true weights
  const uint64_t want = (uint64_t)held + incoming;
  if (want > 0xFFFFFFFFull) return false;
  if (want > p->_volume_params.nBrickStoreBricks) {
    std::vector<int32_t> keys((size_t)held * 3);
    std::vector<float> t((size_t)held * HKF_MAP_BRICK_VOX), w((size_t)held * HKF_MAP_BRICK_VOX);
    std::vector<uint8_t> col(color ? (size_t)held * HKF_MAP_BRICK_VOX * 3 : 0);
    if (held && dm->check(kf_read_brick_store(ctx, 0, held, keys.data(), t.data(), w.data(), color ? col.data() : nullptr))) return false;
    if (!setBrickStore((unsigned)want)) return false;
    if (held && dm->check(kf_write_brick_store(ctx, held, keys.data(), t.data(), w.data(), color ? col.data() : nullptr))) return false;
  }
  return true;
}
bool HybKinectfu::mergeShow() {
  AppParams* p = AppParams::instance();
  CudaDeviceDataMan* dm = CudaDeviceDataMan::instance();
  kf_ctx* ctx = dm->ctx();
  if (dm->check(kf_refill_window(ctx))) return false;
  const Mat44 pose = _camera_pose_finder->getCameraPose();
  const bool resident = _camera_pose_finder->deviceResident();
  const kf_mat44 kp = to_kf(pose);
  kf_raycast_params rp = {p->_raycast_params.fRayIncrement};
  return 0 == dm->check(kf_raycast_volume(ctx, p->_switch_params.useRGBData, resident ? nullptr : &kp, &rp, &p->_depth_camera_params,
                                          p->_depth_prepocess_params.fMinTrunc, p->_depth_prepocess_params.fMaxTrunc));
}
bool HybKinectfu::mergeMap(const std::string& path, const int offsetBricks[3]) {
  if (!_inited) return false;
  CudaDeviceDataMan* dm = CudaDeviceDataMan::instance();
  kf_ctx* ctx = dm->ctx();
  const int32_t off[3] = {offsetBricks ? offsetBricks[0] : 0, offsetBricks ? offsetBricks[1] : 0, offsetBricks ? offsetBricks[2] : 0};
  lastTracked();                                                // a frame still in flight settles first: the raycast below uses this session's pose
  // 1. the whole file checked, every translated key in range, the volume this instance's: nothing is touched before
  HkfMapHeader h;
  const int is = hkf_map_info_offset(path.c_str(), off, &h);
  if (!merge_file_is_ours(path, is, h)) return false;
  // 2. the window captured; 3. room for every brick of the file
  if (!mergeMakeRoom(h.has_color != 0, h.n_bricks)) return false;
  // 4. the file's bricks, translated, merged chunk by chunk (a file's keys are unique, so every call's are)
  std::vector<int32_t> moved((size_t)kMapChunkBricks * 3);
  const int st = hkf_map_read(path.c_str(), kMapChunkBricks, HkfMapAccept(), [&](uint32_t count, const int32_t* keys, const float* tsdf, const float* weight, const uint8_t* c) {
    if (!hkf_map_offset_keys(count, keys, off, moved.data())) return false;
    return 0 == dm->check(kf_merge_brick_store(ctx, count, moved.data(), tsdf, weight, c, nullptr));
  });
  if (st != HKF_MAP_OK) fprintf(stderr, "mergeMap: reading %s failed (%d): the store holds the bricks merged so far\n", path.c_str(), st);
  // 5. the window shows the merged store (also after a failed read: window and store must not disagree); 6. shiftVolume's raycast, this session's pose
  if (!mergeShow()) return false;
  return st == HKF_MAP_OK;
}
// the whole file in host memory (a destination brick draws on up to 27 of its bricks: no chunks); `color`: the colour bytes too.  Touches no device state.
static bool read_whole_map(const char* who, const std::string& path, const HkfMapHeader& h, bool color, std::vector<int32_t>& keys, std::vector<float>& t,
                           std::vector<float>& w, std::vector<uint8_t>& col) {
  try {
    keys.reserve((size_t)h.n_bricks * 3); t.reserve((size_t)h.n_bricks * HKF_MAP_BRICK_VOX); w.reserve((size_t)h.n_bricks * HKF_MAP_BRICK_VOX);
    if (color) col.reserve((size_t)h.n_bricks * HKF_MAP_BRICK_VOX * 3);
    const int st = hkf_map_read(path.c_str(), kMapChunkBricks, HkfMapAccept(), [&](uint32_t count, const int32_t* k, const float* tsdf, const float* weight, const uint8_t* c) {
      keys.insert(keys.end(), k, k + (size_t)count * 3);
      t.insert(t.end(), tsdf, tsdf + (size_t)count * HKF_MAP_BRICK_VOX);
      w.insert(w.end(), weight, weight + (size_t)count * HKF_MAP_BRICK_VOX);
      if (color && c) col.insert(col.end(), c, c + (size_t)count * HKF_MAP_BRICK_VOX * 3);
      return true;
    });
    if (st != HKF_MAP_OK || keys.size() != (size_t)h.n_bricks * 3 || (color && col.size() != t.size() * 3)) {
      fprintf(stderr, "%s: reading %s failed (%d); nothing touched\n", who, path.c_str(), st);
      return false;
    }
  } catch (const std::bad_alloc&) { return false; }
  return true;
}
// a matrix in metres, as poses are, as the C ABI's [R | t] in voxels: the cell is the fp32 quotient the volume uses
static void rigid_in_voxels(const Mat44& m, double xf[12]) {
  const AppParams* p = AppParams::instance();
  const float cell = p->_volume_params.fVolumeMeterSize / (float)p->_volume_params.nResolution;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) xf[4 * i + j] = (double)m.entries[4 * i + j];
    xf[4 * i + 3] = (double)m.entries[4 * i + 3] / (double)cell;
  }
}
bool HybKinectfu::mergeMap(const std::string& path, const Mat44& srcToDst) {
  if (!_inited) return false;
  AppParams* p = AppParams::instance();
  CudaDeviceDataMan* dm = CudaDeviceDataMan::instance();
  kf_ctx* ctx = dm->ctx();
  lastTracked();
  // 1. the file checked, the volume this instance's; the transform in voxels: the cell is the fp32 quotient the volume uses
  HkfMapHeader h;
  const int is = hkf_map_info(path.c_str(), &h);
  if (!merge_file_is_ours(path, is, h)) return false;
  double xf[12];
  rigid_in_voxels(srcToDst, xf);
  const bool color = h.has_color != 0;
  if (h.n_bricks > 0xFFFFFFFFull) return false;
  // 2. the whole file in host memory, and its candidate bricks: still nothing touched
  std::vector<int32_t> keys;
  std::vector<float> t, w;
  std::vector<uint8_t> col;
  int64_t candidates = -1;
  if (!read_whole_map("mergeMap", path, h, color, keys, t, w, col)) return false;
  candidates = kf_rigid_brick_keys((uint32_t)h.n_bricks, keys.data(), xf, nullptr, 0);
  if (candidates < 0) {
    fprintf(stderr, "mergeMap: %s refused: the matrix is no rigid transform, or it moves a brick out of the key range\n", path.c_str());
    return false;
  }
  // 3. the window captured, room for every candidate brick; 4. one merge; 5. the window shows the merged store; 6. the raycast
  if (!mergeMakeRoom(color, (uint64_t)candidates)) return false;
  const int ms = dm->check(kf_merge_brick_store_rigid(ctx, (uint32_t)h.n_bricks, keys.data(), t.data(), w.data(), color ? col.data() : nullptr, xf));
  if (!mergeShow()) return false;
  return ms == 0;
}
bool HybKinectfu::alignMap(const std::string& path, const Mat44& guess, Mat44& found, kf_align_report* report) {
  if (!_inited) return false;
  AppParams* p = AppParams::instance();
  CudaDeviceDataMan* dm = CudaDeviceDataMan::instance();
  kf_ctx* ctx = dm->ctx();
  lastTracked();
  // 1. mergeMap's checks: the file, the volume this instance's, the guess a rigid transform that keeps every brick in the key range; nothing touched before
  HkfMapHeader h;
  const int is = hkf_map_info(path.c_str(), &h);
  if (!merge_file_is_ours(path, is, h)) return false;
  double xf[12];
  rigid_in_voxels(guess, xf);
  if (h.n_bricks > 0xFFFFFFFFull) return false;
  std::vector<int32_t> keys;
  std::vector<float> t, w;
  std::vector<uint8_t> col;
  if (!read_whole_map("alignMap", path, h, false, keys, t, w, col)) return false;
  if (kf_rigid_brick_keys((uint32_t)h.n_bricks, keys.data(), xf, nullptr, 0) < 0) {
    fprintf(stderr, "alignMap: %s refused: the guess is no rigid transform, or it moves a brick out of the key range\n", path.c_str());
    return false;
  }
  // 2. the window captured: the store alone is this session's map (a store that was never reserved is reserved, as mergeMap does); no room is made
  if (!mergeMakeRoom(p->_switch_params.useRGBData, 0)) return false;
  // 3. rotations about the middle of the map; 4. one call.  eps 0: the steps go down to what the rule resolves
  int32_t lo[3], hi[3];
  if (dm->check(kf_brick_store_bounds(ctx, lo, hi))) return false;
  kf_align_params ap = {30u, 1000u, 0.0, 0.0, {4.0 * ((double)lo[0] + hi[0]), 4.0 * ((double)lo[1] + hi[1]), 4.0 * ((double)lo[2] + hi[2])}};
  kf_align_report rep;
  if (dm->check(kf_align_brick_store(ctx, (uint32_t)h.n_bricks, keys.data(), t.data(), w.data(), xf, &ap, &rep))) return false;
  if (report) *report = rep;
  const float cell = p->_volume_params.fVolumeMeterSize / (float)p->_volume_params.nResolution;
  found = Mat44();
  for (int i = 0; i < 16; ++i) found.entries[i] = (i % 5 == 0) ? 1.f : 0.f;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) found.entries[4 * i + j] = (float)xf[4 * i + j];
    found.entries[4 * i + 3] = (float)(xf[4 * i + 3] * (double)cell);
  }
  if (rep.verdict != KF_ALIGN_CONVERGED) fprintf(stderr, "alignMap: %s: no convergence (verdict %u after %u steps, %.0f pairs)\n", path.c_str(), rep.verdict, rep.iterations, rep.sums[28]);
  return rep.verdict == KF_ALIGN_CONVERGED;
}
bool HybKinectfu::eraseMapBox(const float lo_m[3], const float hi_m[3], bool keepInside, unsigned* bricksRemoved, uint64_t* voxelsCleared) {
  if (bricksRemoved) *bricksRemoved = 0;
  if (voxelsCleared) *voxelsCleared = 0;
  if (!_inited || !lo_m || !hi_m) return false;
  for (int k = 0; k < 3; ++k) if (lo_m[k] != lo_m[k] || hi_m[k] != hi_m[k]) return false;   // NaN
  AppParams* p = AppParams::instance();
  CudaDeviceDataMan* dm = CudaDeviceDataMan::instance();
  const float cell = p->_volume_params.fVolumeMeterSize / (float)p->_volume_params.nResolution;
  int32_t lo[3], hi[3];
  hkf_erase_box_voxels(lo_m, hi_m, cell, lo, hi);
  lastTracked();                                                // a frame still in flight settles first: the raycast below uses this session's pose
  if (!mergeMakeRoom(p->_switch_params.useRGBData, 0)) return false;      // the window captured: the store alone is this session's map
  uint32_t removed = 0; uint64_t cleared = 0;
  const int es = dm->check(kf_brick_store_erase_box(dm->ctx(), lo, hi, keepInside ? KF_ERASE_OUTSIDE : KF_ERASE_INSIDE, &removed, &cleared));
  if (!mergeShow()) return false;                               // (also after a failed erase: window and store must not disagree)
  if (bricksRemoved) *bricksRemoved = removed;
  if (voxelsCleared) *voxelsCleared = cleared;
  return es == 0;
}
bool HybKinectfu::eraseMapWeak(float minWeight, unsigned* bricksRemoved) {
  if (bricksRemoved) *bricksRemoved = 0;
  if (!_inited || minWeight != minWeight) return false;          // (NaN: kf_brick_store_erase_weak would refuse it after the capture)
  AppParams* p = AppParams::instance();
  CudaDeviceDataMan* dm = CudaDeviceDataMan::instance();
  lastTracked();
  if (!mergeMakeRoom(p->_switch_params.useRGBData, 0)) return false;
  uint32_t removed = 0;
  const int es = dm->check(kf_brick_store_erase_weak(dm->ctx(), minWeight, &removed));
  if (!mergeShow()) return false;
  if (bricksRemoved) *bricksRemoved = removed;
  return es == 0;
}
bool HybKinectfu::relocalise(const DepthFrameData& depth_frame, const RelocParams& rp_in, RelocReport* report) {
  RelocReport rep;
  memset(&rep, 0, sizeof(rep));
  if (report) *report = rep;
  if (!_inited || !depth_frame.mm) return false;
  const AppParams* p = AppParams::instance();
  CudaDeviceDataMan* dm = CudaDeviceDataMan::instance();
  kf_ctx* ctx = dm->ctx();
  RelocParams par = rp_in;
  const RelocParams def = hkf_reloc_defaults();
  const uint32_t levels = p->_icp_params.nPyramidLevels ? p->_icp_params.nPyramidLevels : 1u;
  const uint32_t level = par.level < 0 ? levels - 1u : (uint32_t)par.level;
  if (level >= levels) return false;
  if (par.top == 0) par.top = def.top;
  if (par.max_points == 0) par.max_points = def.max_points;
  for (int k = 0; k < 6; ++k) if (par.n[k] < 0) par.n[k] = def.n[k];
  if (par.top > 4096u || reloc_lattice_count(par.n) < 0) return false;
  lastTracked();                                                // a frame still in flight settles first
  copyFrameToGPU(depth_frame, ColorFrameData());
  if (dm->check(kf_preprocess(ctx, p->_depth_prepocess_params.fMinTrunc, p->_depth_prepocess_params.fMaxTrunc, p->_depth_prepocess_params.fSigmaPixel,
                              p->_depth_prepocess_params.fSigmaDepth, &p->_depth_camera_params))) return false;
  if (level > 0 && dm->check(kf_downsample_new_vertices(ctx))) return false;   // (the pyramid is the tracker's work: without it the level holds the last frame's)
  // the points: the level's vertex map, valid vertices, voxels
  const uint32_t cols = p->_depth_camera_params.cols >> level, rows = p->_depth_camera_params.rows >> level;
  const float cell = volume_cell();
  std::vector<float> verts, pts;
  std::vector<double> poses, centres, refined;
  std::vector<kf_pose_score> scores;
  std::vector<uint32_t> best;
  std::vector<kf_align_report> reps;
  try { verts.resize((size_t)cols * rows * 4); pts.resize((size_t)par.max_points * 3); } catch (const std::bad_alloc&) { return false; }
  if (dm->check(kf_download_map(ctx, KF_MAP_NEW_VERTICES, level, verts.data(), verts.size() * sizeof(float)))) return false;
  float median = 0.f;
  const uint32_t n_pts = reloc_points(verts.data(), cols * rows, cell, par.max_points, pts.data(), &median);
  rep.points = n_pts; rep.median_depth = median;
  if (report) *report = rep;
  if (n_pts == 0 || !(median > 0.f)) return false;             // no measurement in the frame
  const float trans_m = par.trans_step > 0.f ? par.trans_step : p->_integrate_params.fSdfTruncation;
  const float rot = par.rot_step > 0.f ? par.rot_step : atanf(p->_integrate_params.fSdfTruncation / median);
  rep.trans_step = trans_m; rep.rot_step = rot;
  // the centre pose, world voxels, fp64
  const Mat44 cw = par.has_guess ? [&] { Mat44 g; memcpy(g.entries, par.guess, 64); return g; }() : worldPose(_camera_pose_finder->getCameraPose());
  double centre[12];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) centre[4 * i + j] = (double)cw.entries[4 * i + j];
    centre[4 * i + 3] = (double)cw.entries[4 * i + 3] / (double)cell;
  }
  for (int i = 0; i < 12; ++i) if (!isfinite(centre[i])) return false;
  const int64_t K = reloc_lattice_count(par.n);
  try {
    poses.resize((size_t)K * 12); scores.resize((size_t)K); best.resize(par.top); centres.resize((size_t)par.top * 3); refined.resize((size_t)par.top * 12);
    reps.resize(par.top);
  } catch (const std::bad_alloc&) { return false; }
  reloc_lattice(centre, par.n, (double)trans_m / (double)cell, (double)rot, poses.data(), K);
  rep.candidates = (uint32_t)K;
  if (report) *report = rep;
  if (dm->check(kf_map_score_poses(ctx, n_pts, pts.data(), (uint32_t)K, poses.data(), par.band, scores.data()))) return false;
  const uint32_t eligible = reloc_rank(scores.data(), (uint32_t)K, par.min_obs, par.top, best.data());
  const uint32_t M = eligible < par.top ? eligible : par.top;
  if (M == 0) return false;                                     // no candidate sees enough of the map
  rep.best_index = best[0]; rep.best_score = scores[best[0]];
  memcpy(rep.best_pose, &poses[(size_t)best[0] * 12], sizeof(rep.best_pose));
  if (report) *report = rep;
  // each candidate's centre: R * mean(points) + t
  double mean[3] = {0.0, 0.0, 0.0};
  for (uint32_t i = 0; i < n_pts; ++i) for (int k = 0; k < 3; ++k) mean[k] += (double)pts[3 * (size_t)i + k];
  for (int k = 0; k < 3; ++k) mean[k] /= (double)n_pts;
  for (uint32_t a = 0; a < M; ++a) {
    const double* P = &poses[(size_t)best[a] * 12];
    memcpy(&refined[(size_t)a * 12], P, 12 * sizeof(double));
    for (int j = 0; j < 3; ++j) centres[3 * (size_t)a + j] = ((P[4 * j] * mean[0] + P[4 * j + 1] * mean[1]) + P[4 * j + 2] * mean[2]) + P[4 * j + 3];
  }
  kf_refine_params fp = {par.max_iter, par.min_pairs, par.eps_rot, par.eps_trans, par.gate};
  if (dm->check(kf_map_refine_poses(ctx, n_pts, pts.data(), M, refined.data(), centres.data(), &fp, reps.data()))) return false;
  if (dm->check(kf_map_score_poses(ctx, n_pts, pts.data(), M, refined.data(), par.band, scores.data()))) return false;
  uint32_t win = 0;
  if (reloc_rank(scores.data(), M, par.min_obs, 1u, &win) == 0) return false;
  const double* F = &refined[(size_t)win * 12];
  memcpy(rep.refined_pose, F, sizeof(rep.refined_pose));
  rep.refined_score = scores[win]; rep.verdict = reps[win].verdict; rep.iterations = reps[win].iterations;
  const bool accept = (double)scores[win].n_in >= (double)par.accept_inliers * (double)n_pts && scores[win].n_obs >= par.min_obs &&
                      reps[win].verdict != KF_ALIGN_FEW_PAIRS && reps[win].verdict != KF_ALIGN_SINGULAR;
  if (report) *report = rep;
  if (!accept) return false;
  // the found pose in world metres (fp32), its frame, and the pose in that frame
  Mat44 wp = Mat44::getIdentity(), local;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) wp.entries[4 * i + j] = (float)F[4 * i + j];
    wp.entries[4 * i + 3] = (float)(F[4 * i + 3] * (double)cell);
  }
  int32_t frame[3];
  hkf_view_frame(wp.entries, p->_volume_params.fVolumeMeterSize, p->_volume_params.nResolution, frame, local.entries);
  int o[3]; volumeOrigin(o);
  const bool move = p->_volume_params.nBrickStoreBricks > 0 && (frame[0] != o[0] || frame[1] != o[1] || frame[2] != o[2]);
  if (move) {                                                   // loadMap's tail: the window stands where the pose looks
    if (dm->check(kf_brick_store_capture(ctx)) || dm->check(kf_place_window(ctx, frame[0], frame[1], frame[2]))) return false;   // (refused: window, origin and pose untouched)
  } else {                                                      // the pose in the window as it stands: window metres, fp32
    local = wp;
    for (int i = 0; i < 3; ++i) local.entries[4 * i + 3] = (float)((F[4 * i + 3] - (double)o[i]) * (double)cell);
  }
  _camera_pose_finder->setCameraPose(local);                    // host copy and device-resident pose (kf_set_pose: "tracked")
  _frame_id = depth_frame.frameId(); _last_tracked = true; _pending = false;
  rep.accepted = 1;
  if (report) *report = rep;
  const bool resident = _camera_pose_finder->deviceResident();
  const kf_mat44 kp = to_kf(local);
  kf_raycast_params rc = {p->_raycast_params.fRayIncrement};
  return 0 == dm->check(kf_raycast_volume(ctx, p->_switch_params.useRGBData, resident ? nullptr : &kp, &rc, &p->_depth_camera_params,
                                          p->_depth_prepocess_params.fMinTrunc, p->_depth_prepocess_params.fMaxTrunc));
}
bool HybKinectfu::sampleMap(const double* world_m, size_t n, float* distance_m, float* weight, float* gradient, uint8_t* color) {
  if (!_inited || !world_m || n > 0xFFFFFFFFull) return false;
  if (n == 0) return true;
  AppParams* p = AppParams::instance();
  CudaDeviceDataMan* dm = CudaDeviceDataMan::instance();
  const float cell = p->_volume_params.fVolumeMeterSize / (float)p->_volume_params.nResolution;
  const float trunc = p->_integrate_params.fSdfTruncation;
  std::vector<double> vox(3 * n);
  hkf_query_voxels(world_m, 3 * n, cell, vox.data());
  if (dm->check(kf_map_sample(dm->ctx(), (uint32_t)n, vox.data(), distance_m, weight, gradient, color))) return false;
  if (distance_m) for (size_t i = 0; i < n; ++i) distance_m[i] = distance_m[i] * trunc;
  if (gradient) for (size_t i = 0; i < 3 * n; ++i) gradient[i] = gradient[i] * trunc / cell;
  return true;
}
bool HybKinectfu::castMapRays(const double* origin_m, const float* dir, const float* t_min_m, const float* t_max_m, size_t n, uint8_t* status, float* t_m, float* normal,
                              uint8_t* color, float* weight) {
  if (!_inited || !origin_m || !dir || !t_min_m || !t_max_m || n > 0xFFFFFFFFull) return false;
  if (n == 0) return true;
  AppParams* p = AppParams::instance();
  CudaDeviceDataMan* dm = CudaDeviceDataMan::instance();
  const float cell = p->_volume_params.fVolumeMeterSize / (float)p->_volume_params.nResolution;
  std::vector<double> vox(3 * n);
  hkf_query_voxels(origin_m, 3 * n, cell, vox.data());
  std::vector<float> t0(n), t1(n);
  for (size_t i = 0; i < n; ++i) { t0[i] = t_min_m[i] / cell; t1[i] = t_max_m[i] / cell; }
  const float step = p->_raycast_params.fRayIncrement / cell;
  if (dm->check(kf_map_cast_rays(dm->ctx(), (uint32_t)n, vox.data(), dir, t0.data(), t1.data(), step, 1u << 24, status, t_m, normal, color, weight))) return false;
  if (t_m) for (size_t i = 0; i < n; ++i) t_m[i] = t_m[i] * cell;
  return true;
}
bool HybKinectfu::distanceFieldVoxels(const int32_t lo_vox[3], const uint32_t dims[3], uint32_t radius, float level, uint32_t siteMask, uint16_t* dist2, uint8_t* cls) {
  uint64_t count = 0;
  if (!_inited || !lo_vox || !dims || !hkf_edt_voxel_count(dims, &count)) return false;        // (also a box of more than HKF_EDT_MAX_VOXELS voxels)
  CudaDeviceDataMan* dm = CudaDeviceDataMan::instance();
  const uint32_t tx = hkf_edt_tile_count(dims[0]), ty = hkf_edt_tile_count(dims[1]), tz = hkf_edt_tile_count(dims[2]);
  if (tx == 1u && ty == 1u && tz == 1u) return dm->check(kf_map_distance_field(dm->ctx(), lo_vox, dims, radius, level, siteMask, dist2, cls)) == 0;
  std::vector<uint16_t> td;
  std::vector<uint8_t> tc;
  try {
    td.resize(dist2 ? (size_t)HKF_EDT_TILE * HKF_EDT_TILE * HKF_EDT_TILE : 0);
    tc.resize(cls ? (size_t)HKF_EDT_TILE * HKF_EDT_TILE * HKF_EDT_TILE : 0);
  } catch (const std::exception&) { return false; }
  for (uint32_t iz = 0; iz < tz; ++iz) for (uint32_t iy = 0; iy < ty; ++iy) for (uint32_t ix = 0; ix < tx; ++ix) {
    uint32_t off[3], len[3];
    hkf_edt_tile(dims[0], ix, &off[0], &len[0]); hkf_edt_tile(dims[1], iy, &off[1], &len[1]); hkf_edt_tile(dims[2], iz, &off[2], &len[2]);
    const int64_t lo64[3] = {(int64_t)lo_vox[0] + off[0], (int64_t)lo_vox[1] + off[1], (int64_t)lo_vox[2] + off[2]};
    if (lo64[0] > INT32_MAX || lo64[1] > INT32_MAX || lo64[2] > INT32_MAX) return false;     // (such a box lies outside the key range)
    const int32_t lo[3] = {(int32_t)lo64[0], (int32_t)lo64[1], (int32_t)lo64[2]};
    if (dm->check(kf_map_distance_field(dm->ctx(), lo, len, radius, level, siteMask, dist2 ? td.data() : nullptr, cls ? tc.data() : nullptr))) return false;
    for (uint32_t z = 0; z < len[2]; ++z) for (uint32_t y = 0; y < len[1]; ++y) {
      const size_t src = ((size_t)z * len[1] + y) * len[0], dst = (((size_t)off[2] + z) * dims[1] + off[1] + y) * dims[0] + off[0];
      if (dist2) memcpy(dist2 + dst, td.data() + src, 2 * (size_t)len[0]);
      if (cls) memcpy(cls + dst, tc.data() + src, len[0]);
    }
  }
  return true;
}
bool HybKinectfu::distanceField(const float lo_m[3], const float hi_m[3], float maxDist_m, float level, uint32_t siteMask, std::vector<float>& distance_m,
                                std::vector<uint8_t>& cls, uint32_t dims[3], uint32_t* radiusVox, int32_t* loVox) {
  if (!_inited || !lo_m || !hi_m || !dims) return false;
  AppParams* p = AppParams::instance();
  const float cell = p->_volume_params.fVolumeMeterSize / (float)p->_volume_params.nResolution;
  int32_t lo[3];
  if (!hkf_edt_box_voxels(lo_m, hi_m, cell, lo, dims)) return false;
  const uint32_t radius = hkf_edt_radius(maxDist_m, cell);
  if (radiusVox) *radiusVox = radius;
  if (loVox) memcpy(loVox, lo, sizeof(lo));
  uint64_t count = 0;
  if (!hkf_edt_voxel_count(dims, &count)) return false;          // too large a box: refused before anything is sized
  const size_t n = (size_t)count;
  std::vector<uint16_t> d2;
  try { d2.resize(n); distance_m.resize(n); cls.resize(n); } catch (const std::exception&) { return false; }   // (bad_alloc, length_error)
  if (!distanceFieldVoxels(lo, dims, radius, level, siteMask, d2.data(), cls.data())) return false;
  for (size_t i = 0; i < n; ++i) distance_m[i] = d2[i] == KF_EDT_FAR ? INFINITY : sqrtf((float)d2[i]) * cell;
  return true;
}
bool HybKinectfu::loadMapCoarser(const std::string& path) {
  if (!_inited) return false;
  AppParams* p = AppParams::instance();
  CudaDeviceDataMan* dm = CudaDeviceDataMan::instance();
  kf_ctx* ctx = dm->ctx();
  lastTracked();                                                // as loadMap: a frame still in flight settles first
  // 1. the file checked as a whole; the volume this instance's but for a resolution 2^L times as fine, L in [1, 3]: nothing is touched before
  HkfMapHeader h;
  memset(&h, 0, sizeof(h));
  const int is = hkf_map_info(path.c_str(), &h);
  const uint32_t res = p->_volume_params.nResolution;
  if (is == HKF_MAP_OK && h.resolution == res) return loadMap(path);
  unsigned levels = 0;
  for (unsigned l = 1; l <= 3; ++l) if (h.resolution == (uint64_t)res << l) levels = l;
  if (is != HKF_MAP_OK || levels == 0 || memcmp(&h.size_m, &p->_volume_params.fVolumeMeterSize, 4) != 0 ||
      memcmp(&h.max_weight, &p->_volume_params.fWeightMax, 4) != 0 || (h.has_color != 0) != p->_switch_params.useRGBData || h.n_bricks > 0xFFFFFFFFull) {
    fprintf(stderr, "loadMapCoarser: %s refused (%d)%s\n", path.c_str(), is, is == HKF_MAP_OK ? ": its volume is not this instance's at 2, 4 or 8 times the resolution" : "");
    return false;
  }
  const bool color = h.has_color != 0;
  std::vector<int32_t> keys;
  std::vector<float> t, w;
  std::vector<uint8_t> col;
  if (!read_whole_map("loadMapCoarser", path, h, color, keys, t, w, col)) return false;
  // 2. from here on a failure leaves an EMPTY map, as loadMap's does.  Level by level through the store: reserved (which clears it) for the level's coarse
  // keys, the finer map merged halved into it, and for the next level read out again
  bool ok = 0 == dm->check(kf_reset_volume(ctx));
  for (unsigned l = 0; ok && l < levels; ++l) {
    const uint32_t n = (uint32_t)(keys.size() / 3);
    const int64_t coarse = kf_halved_brick_keys(n, keys.data(), nullptr, 0);
    ok = coarse >= 0;
    if (!ok) break;
    const uint64_t want = (uint64_t)coarse > p->_volume_params.nBrickStoreBricks ? (uint64_t)coarse : p->_volume_params.nBrickStoreBricks;
    ok = setBrickStore((unsigned)(want ? want : 1u)) &&        // (a store of one brick for an empty map: kf_place_window needs a store)
         0 == dm->check(kf_merge_brick_store_halved(ctx, n, keys.data(), t.data(), w.data(), color ? col.data() : nullptr));
    if (!ok || l + 1 == levels) break;
    uint32_t held = 0;
    ok = 0 == dm->check(kf_brick_store_count(ctx, &held, nullptr, nullptr));
    if (!ok) break;
    try {
      keys.resize((size_t)held * 3); t.resize((size_t)held * HKF_MAP_BRICK_VOX); w.resize((size_t)held * HKF_MAP_BRICK_VOX);
      if (color) col.resize((size_t)held * HKF_MAP_BRICK_VOX * 3);
    } catch (const std::bad_alloc&) { ok = false; break; }
    ok = !held || 0 == dm->check(kf_read_brick_store(ctx, 0, held, keys.data(), t.data(), w.data(), color ? col.data() : nullptr));
  }
  // 3. the window where the file's stood, on the coarse lattice: 8 * floor(origin / 2^L / 8) per axis
  int32_t o[3];
  const int64_t step = (int64_t)8 << levels;
  for (int k = 0; k < 3; ++k) {
    const int64_t v = h.origin_vox[k];
    o[k] = (int32_t)(8 * (v >= 0 ? v / step : -((-v + step - 1) / step)));
  }
  if (!ok || dm->check(kf_place_window(ctx, o[0], o[1], o[2]))) { dm->check(kf_reset_volume(ctx)); return false; }
  // 4. the file's pose in the new window's coordinates: fp64, rounded to fp32 once
  Mat44 pose; memcpy(pose.entries, h.pose, 64);
  const double s_file = (double)h.size_m / (double)h.resolution, s_ctx = (double)h.size_m / (double)res;
  for (int k = 0; k < 3; ++k) pose.entries[4 * k + 3] = (float)(((double)pose.entries[4 * k + 3] + (double)h.origin_vox[k] * s_file) - (double)o[k] * s_ctx);
  _camera_pose_finder->setCameraPose(pose);
  _frame_id = h.frame_id; _last_tracked = true; _pending = false;
  const bool resident = _camera_pose_finder->deviceResident();
  const kf_mat44 kp = to_kf(pose);
  kf_raycast_params rp = {p->_raycast_params.fRayIncrement};  // loadMap's raycast
  return 0 == dm->check(kf_raycast_volume(ctx, p->_switch_params.useRGBData, resident ? nullptr : &kp, &rp, &p->_depth_camera_params,
                                          p->_depth_prepocess_params.fMinTrunc, p->_depth_prepocess_params.fMaxTrunc));
}
bool HybKinectfu::recentre() {
  const AppParams* p = AppParams::instance();
  int32_t d[3];
  hkf_recentre_shift(_camera_pose_finder->getCameraPose().entries, p->_volume_params.fVolumeMeterSize, p->_volume_params.nResolution,
                     p->_volume_params.fRecentreDist, d);
  if (d[0] == 0 && d[1] == 0 && d[2] == 0) return true;
  return shiftVolume(d[0], d[1], d[2]);
}
// what DataViewer shows, without the maps crossing to the host (HybKinectfu.cpp:145-158): 4 bytes per pixel come back
static bool read_view(CudaDeviceDataMan* dm, std::vector<uint8_t>& bgra) {
  uint32_t cols = 0, rows = 0;
  if (dm->check(kf_view_size(dm->ctx(), &cols, &rows))) return false;
  bgra.resize((size_t)cols * rows * 4);
  return dm->check(kf_read_view(dm->ctx(), bgra.data(), bgra.size())) == 0;
}
bool HybKinectfu::renderView(const Mat44* pose, const kf_camera_params& cam, int mode, std::vector<uint8_t>& bgra) {
  if (!_inited) return false;
  const AppParams* p = AppParams::instance();
  CudaDeviceDataMan* dm = CudaDeviceDataMan::instance();
  // (a finder that keeps its pose on the host: "the current pose" is the host's copy)
  kf_mat44 kp; const kf_mat44* tp = nullptr;
  if (pose) { kp = to_kf(*pose); tp = &kp; }
  else if (!_camera_pose_finder->deviceResident()) { kp = to_kf(_camera_pose_finder->getCameraPose()); tp = &kp; }
  kf_raycast_params rp = {p->_raycast_params.fRayIncrement};
  if (dm->check(kf_render_view(dm->ctx(), mode, tp, &cam, &rp, p->_depth_prepocess_params.fMinTrunc, p->_depth_prepocess_params.fMaxTrunc, nullptr, nullptr))) return false;
  return read_view(dm, bgra);
}
bool HybKinectfu::renderViewAt(int mode, const int frame[3], const Mat44* pose, const kf_camera_params& cam, std::vector<uint8_t>& bgra) {
  if (!_inited || !frame) return false;
  const AppParams* p = AppParams::instance();
  CudaDeviceDataMan* dm = CudaDeviceDataMan::instance();
  const int32_t f32[3] = {frame[0], frame[1], frame[2]};
  kf_mat44 kp; const kf_mat44* tp = nullptr;
  if (pose) { kp = to_kf(*pose); tp = &kp; }
  else if (!_camera_pose_finder->deviceResident()) {            // the host's copy, into the frame's coordinates: the same expression as k_shift_pose
    int o[3]; volumeOrigin(o);
    Mat44 moved = _camera_pose_finder->getCameraPose();
    const float cell = volume_cell();
    for (int k = 0; k < 3; ++k) moved.entries[4 * k + 3] = moved.entries[4 * k + 3] - (float)(frame[k] - o[k]) * cell;
    kp = to_kf(moved); tp = &kp;
  }
  kf_raycast_params rp = {p->_raycast_params.fRayIncrement};
  if (dm->check(kf_render_view_at(dm->ctx(), mode, f32, tp, &cam, &rp, p->_depth_prepocess_params.fMinTrunc, p->_depth_prepocess_params.fMaxTrunc, nullptr, nullptr))) return false;
  return read_view(dm, bgra);
}
bool HybKinectfu::renderMapView(int mode, const Mat44& world_pose, const kf_camera_params& cam, std::vector<uint8_t>& bgra) {
  if (!_inited) return false;
  const AppParams* p = AppParams::instance();
  int32_t f[3]; Mat44 local;
  hkf_view_frame(world_pose.entries, p->_volume_params.fVolumeMeterSize, p->_volume_params.nResolution, f, local.entries);
  const int frame[3] = {(int)f[0], (int)f[1], (int)f[2]};
  return renderViewAt(mode, frame, &local, cam, bgra);
}
bool HybKinectfu::viewModelMaps(int mode, std::vector<uint8_t>& bgra) {
  if (!_inited) return false;
  CudaDeviceDataMan* dm = CudaDeviceDataMan::instance();
  if (dm->check(kf_view_model_maps(dm->ctx(), mode))) return false;
  return read_view(dm, bgra);
}
bool HybKinectfu::lastTracked() {
  if (_pending && _camera_pose_finder) { _last_tracked = _camera_pose_finder->syncPose(); _pending = false; }
  return _last_tracked;
}
Mat44 HybKinectfu::getCameraPose() {
  if (!_camera_pose_finder) return Mat44::getIdentity();
  lastTracked();
  return _camera_pose_finder->getCameraPose();
}

// ---- MeshData: the pieces of src/utils/mesh/meshData.* that saveMesh uses ---------------------------------------------------------------
namespace {
struct I3 { int x, y, z; bool operator==(const I3& o) const { return x == o.x && y == o.y && z == o.z; } };
struct I3Hash { size_t operator()(const I3& v) const { return ((size_t)v.x * 73856093u) ^ ((size_t)v.y * 19349669u) ^ ((size_t)v.z * 83492791u); } };
inline int sgn(float v) { return (0 < v) - (v < 0); }
inline I3 virtual_voxel(const float* v, float voxel) {          // meshData.h:750-753
  float r = (float)(1.0 / (double)voxel);
  return I3{(int)(v[0] * r + (float)(sgn(v[0]) * 0.5)), (int)(v[1] * r + (float)(sgn(v[1]) * 0.5)), (int)(v[2] * r + (float)(sgn(v[2]) * 0.5))};
}
}
unsigned MeshData::mergeCloseVertices(float thresh) {            // meshData.cpp:198-283 (approx): first vertex in a 3x3x3 cell block wins
  const unsigned numV = (unsigned)(vertices.size() / 3);
  std::vector<unsigned> lookup(numV);
  std::vector<float> nv, nc; nv.reserve(vertices.size());
  const bool has_col = colors.size() == (size_t)numV * 4;
  std::unordered_map<I3, unsigned, I3Hash> grid; grid.reserve(numV * 2);
  unsigned cnt = 0;
  for (unsigned v = 0; v < numV; ++v) {
    I3 c = virtual_voxel(&vertices[3 * v], thresh);
    unsigned nn = (unsigned)-1;
    for (int i = -1; i <= 1 && nn == (unsigned)-1; ++i)
      for (int j = -1; j <= 1 && nn == (unsigned)-1; ++j)
        for (int k = -1; k <= 1; ++k) { auto it = grid.find(I3{c.x + i, c.y + j, c.z + k}); if (it != grid.end()) { nn = it->second; break; } }
    if (nn == (unsigned)-1) {
      grid[c] = cnt; lookup[v] = cnt++;
      nv.insert(nv.end(), &vertices[3 * v], &vertices[3 * v] + 3);
      if (has_col) nc.insert(nc.end(), &colors[4 * v], &colors[4 * v] + 4);
    } else lookup[v] = nn;
  }
  for (auto& f : faces) f = lookup[f];
  vertices.swap(nv);
  if (has_col) colors.swap(nc);
  removeDegeneratedFaces();                                      // meshData.cpp:281
  return cnt;
}
unsigned MeshData::removeDegeneratedFaces() {                    // meshData.cpp:289-310: a face that names a vertex twice (an edge the weld collapsed) goes
  size_t w = 0;
  for (size_t i = 0; i + 2 < faces.size(); i += 3) {
    const unsigned a = faces[i], b = faces[i + 1], c = faces[i + 2];
    if (a == b || a == c || b == c) continue;
    faces[w] = a; faces[w + 1] = b; faces[w + 2] = c; w += 3;
  }
  faces.resize(w);
  return (unsigned)(w / 3);
}
unsigned MeshData::removeDuplicateFaces() {                      // meshData.cpp:42-82: same index set in any order = duplicate, first kept
  struct Key { unsigned a, b, c; bool operator==(const Key& o) const { return a == o.a && b == o.b && c == o.c; } };
  struct KeyHash { size_t operator()(const Key& k) const { return ((size_t)k.a * 73856093u) ^ ((size_t)k.b * 19349669u) ^ ((size_t)k.c * 83492791u); } };
  std::unordered_set<Key, KeyHash> seen; seen.reserve(faces.size() / 3 * 2);
  std::vector<unsigned> nf; nf.reserve(faces.size());
  for (size_t i = 0; i + 2 < faces.size(); i += 3) {
    unsigned s[3] = {faces[i], faces[i + 1], faces[i + 2]};
    std::sort(s, s + 3);
    if (seen.insert(Key{s[0], s[1], s[2]}).second) nf.insert(nf.end(), &faces[i], &faces[i] + 3);
  }
  faces.swap(nf);
  return (unsigned)(faces.size() / 3);
}
void MeshData::computeVertexNormals() {                          // meshData.h:713-736: unit face normals accumulated per vertex, renormalised
  normals.assign(vertices.size(), 0.f);
  auto nrm = [](float* n) { float l = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]); if (l < 1e-8) { n[0] = n[1] = n[2] = 0.f; } else { float r = (float)(1.0 / (double)l); n[0] *= r; n[1] *= r; n[2] *= r; } };
  for (size_t i = 0; i + 2 < faces.size(); i += 3) {
    const float* a = &vertices[3 * faces[i]]; const float* b = &vertices[3 * faces[i + 1]]; const float* c = &vertices[3 * faces[i + 2]];
    float e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    float n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    nrm(n);
    for (int k = 0; k < 3; ++k) { float* d = &normals[3 * faces[i + k]]; d[0] += n[0]; d[1] += n[1]; d[2] += n[2]; }
  }
  for (size_t v = 0; v + 2 < normals.size(); v += 3) nrm(&normals[v]);
}
bool MeshData::saveToFile(const std::string& filename) const {  // MeshIO.h:50-76 (dispatch), MeshIO.cpp:490-662 (writers): same bytes as the reference's files
  const size_t nv = vertices.size() / 3, nf = faces.size() / 3;
  if (nv == 0) return false;                                     // MeshIO.h:52 "empty mesh"
  const bool has_col = colors.size() == nv * 4 && nv > 0, has_n = normals.size() == nv * 3 && nv > 0;
  std::string ext = filename.substr(filename.find_last_of(".") + 1);      // MeshIO.h:20-26: text after the last '.', case-insensitive
  for (auto& ch : ext) ch = (char)tolower(ch);
  if (ext == "obj") {                                            // MeshIO.cpp:609-662
    std::ofstream f(filename);
    if (!f.is_open()) return false;
    f << "####\n#\n# OBJ file Generated by MLIB\n#\n####\n# Object " << filename << "\n#\n# Vertices: " << nv << "\n# Faces: " << nf << "\n#\n####\n";
    for (size_t i = 0; i < nv; ++i) {
      f << "v " << vertices[3 * i] << " " << vertices[3 * i + 1] << " " << vertices[3 * i + 2];
      if (has_col) f << " " << colors[4 * i] << " " << colors[4 * i + 1] << " " << colors[4 * i + 2];
      f << "\n";
    }
    if (has_n) for (size_t i = 0; i < nv; ++i) f << "vn " << normals[3 * i] << " " << normals[3 * i + 1] << " " << normals[3 * i + 2] << "\n";
    for (size_t i = 0; i < nf; ++i) f << "f " << faces[3 * i] + 1 << " " << faces[3 * i + 1] + 1 << " " << faces[3 * i + 2] + 1 << " \n";
    return f.good();
  }
  if (ext == "ply") {                                            // MeshIO.cpp:490-571: binary little-endian, interleaved vertex records
    std::ofstream f(filename, std::ios::binary);
    if (!f.is_open()) return false;
    f << "ply\nformat binary_little_endian 1.0\ncomment MLIB generated\nelement vertex " << nv << "\nproperty float x\nproperty float y\nproperty float z\n";
    if (has_n) f << "property float nx\nproperty float ny\nproperty float nz\n";
    if (has_col) f << "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n";
    f << "element face " << nf << "\nproperty list uchar int vertex_indices\nend_header\n";
    std::vector<unsigned char> rec;
    rec.reserve(nv * 28);
    for (size_t i = 0; i < nv; ++i) {
      const unsigned char* p = (const unsigned char*)&vertices[3 * i];
      rec.insert(rec.end(), p, p + 12);
      if (has_n) { const unsigned char* q = (const unsigned char*)&normals[3 * i]; rec.insert(rec.end(), q, q + 12); }
      if (has_col) {
        // :547-548: uchar3(r*255, g*255, b*255) copied as FOUR bytes -- the reference's 4th (alpha) byte is whatever follows the
        // 3-byte local on its stack; we write 255 (opaque), the only byte of the file that is not defined by the reference
        rec.push_back((unsigned char)(colors[4 * i] * 255)); rec.push_back((unsigned char)(colors[4 * i + 1] * 255)); rec.push_back((unsigned char)(colors[4 * i + 2] * 255));
        rec.push_back(255);
      }
    }
    f.write((const char*)rec.data(), (std::streamsize)rec.size());
    for (size_t i = 0; i < nf; ++i) { const unsigned char three = 3; f.write((const char*)&three, 1); f.write((const char*)&faces[3 * i], 12); }
    return f.good();
  }
  if (ext == "off") {                                            // MeshIO.cpp:574-606: "COFF", integer colours with a trailing blank
    std::ofstream f(filename);
    if (!f.is_open()) return false;
    f << "COFF\n" << nv << " " << nf << " " << 0 << "\n";
    for (size_t i = 0; i < nv; ++i) {
      f << vertices[3 * i] << " " << vertices[3 * i + 1] << " " << vertices[3 * i + 2];
      if (has_col) f << " " << (unsigned)(colors[4 * i] * 255) << " " << (unsigned)(colors[4 * i + 1] * 255) << " " << (unsigned)(colors[4 * i + 2] * 255) << " " << (unsigned)(colors[4 * i + 3] * 255) << " ";
      f << "\n";
    }
    for (size_t i = 0; i < nf; ++i) f << 3 << " " << faces[3 * i] << " " << faces[3 * i + 1] << " " << faces[3 * i + 2] << "\n";
    return f.good();
  }
  return false;                                                  // MeshIO.h:72 "unknown file format"
}

// ---- MeshGeneratorMarchingcube (src/MeshGeneratorMarchingcube.cpp) -------------------------------------------------------------------------
void MeshGeneratorMarchingcube::generateMesh() {                // :23-29
  const AppParams* p = AppParams::instance();
  CudaDeviceDataMan* dm = CudaDeviceDataMan::instance();
  _world = false;
  if (p->_volume_params.bMapMesh && p->_volume_params.nBrickStoreBricks > 0) {   // the map: store and window on the world's tile lattice, world coordinates
    uint64_t dropped = 0; uint32_t tiles = 0;
    if (0 == kf_brick_store_count(dm->ctx(), nullptr, &dropped, nullptr) && dropped)
      fprintf(stderr, "generateMesh: the brick store has dropped %llu bricks for want of room: the map mesh has holes there\n", (unsigned long long)dropped);
    if (dm->check(kf_clear_triangles(dm->ctx()))) return;
    _world = 0 == dm->check(kf_marching_cubes_map(dm->ctx(), p->_switch_params.useRGBData, mesh_threshold(), KF_MC_WORLD, &tiles));
    return;
  }
  if (p->_volume_params.nStreamMeshTriangles > 0) {           // streaming: [world soup, the current window], everything in world coordinates
    const int32_t lo[3] = {0, 0, 0}, hi[3] = {(int32_t)p->_volume_params.nResolution, (int32_t)p->_volume_params.nResolution, (int32_t)p->_volume_params.nResolution};
    if (dm->check(kf_clear_triangles(dm->ctx())) || dm->check(kf_append_world_soup(dm->ctx()))) return;
    _world = 0 == dm->check(kf_marching_cubes_region(dm->ctx(), p->_switch_params.useRGBData, mesh_threshold(), lo, hi, KF_MC_WORLD));
    return;
  }
  dm->check(kf_marching_cubes(dm->ctx(), p->_switch_params.useRGBData, 300 * p->_volume_params.fVolumeMeterSize / p->_volume_params.nResolution));
}
void MeshGeneratorMarchingcube::setMapMesh(bool on) { AppParams::instance()->_volume_params.bMapMesh = on; }
unsigned MeshGeneratorMarchingcube::triangleCount() {
  uint32_t n = 0; CudaDeviceDataMan* dm = CudaDeviceDataMan::instance();
  dm->check(kf_triangle_count(dm->ctx(), &n));
  return n;
}
bool MeshGeneratorMarchingcube::copyTrianglesToCPU() {          // :30-60
  CudaDeviceDataMan* dm = CudaDeviceDataMan::instance();
  unsigned n = triangleCount();
  if (n == 0) return false;
  std::vector<kf_triangle> tris(n);
  if (dm->check(kf_read_triangles(dm->ctx(), tris.data(), 0, n))) return false;
  setTriangles(tris.data(), n, AppParams::instance()->_switch_params.useRGBData);
  return true;
}
void MeshGeneratorMarchingcube::setTriangles(const kf_triangle* tris, unsigned n, bool col) {   // :39-58, the copy loop
  _meshes = MeshData();
  _meshes.vertices.resize((size_t)n * 9);
  if (col) _meshes.colors.resize((size_t)n * 12);
  for (unsigned i = 0; i < n; ++i) {
    const kf_vertex* v[3] = {&tris[i].v0, &tris[i].v1, &tris[i].v2};
    for (int k = 0; k < 3; ++k) {
      memcpy(&_meshes.vertices[(size_t)(3 * i + k) * 3], v[k]->pos, 12);
      if (col) { float* c = &_meshes.colors[(size_t)(3 * i + k) * 4]; c[0] = v[k]->color[2]; c[1] = v[k]->color[1]; c[2] = v[k]->color[0]; c[3] = 1.0f; }   // :53 x<->z swap
    }
  }
}
void MeshGeneratorMarchingcube::weldMesh() {                    // :69-84
  // The reference sizes its index buffer by the VERTEX count (:70) and fills one face per triangle: the surplus two thirds are
  // (0,0,0) faces, which mergeCloseVertices' closing removeDegeneratedFaces drops again -- same result as one face per triangle.
  const size_t nv = _meshes.vertices.size() / 3;
  _meshes.faces.resize(nv);
  for (size_t i = 0; i < nv; ++i) _meshes.faces[i] = (unsigned)i;   // index buffer of the triangle soup
  _meshes.mergeCloseVertices(0.0001f);
  _meshes.removeDuplicateFaces();
  _meshes.computeVertexNormals();
}
void MeshGeneratorMarchingcube::dropMeshParts() { if (dropsParts()) dropParts(_meshes, _min_part_faces, _largest_only); }
bool MeshGeneratorMarchingcube::weldOnDevice() {               // :69-86 as kf_weld_mesh; false (mesh untouched) when there is nothing to weld or the device refuses
  CudaDeviceDataMan* dm = CudaDeviceDataMan::instance();
  if (!dm->ctx() || triangleCount() == 0) return false;
  const bool col = AppParams::instance()->_switch_params.useRGBData;
  uint32_t nv = 0, nf = 0;
  if (kf_weld_mesh(dm->ctx(), col, 0.0001f) != 0) return false;
  if (dropsParts() && kf_mesh_drop_parts(dm->ctx(), _min_part_faces, _largest_only, nullptr, nullptr) != 0) return false;
  if (kf_mesh_counts(dm->ctx(), &nv, &nf, nullptr) != 0) return false;
  MeshData m;
  m.vertices.resize((size_t)nv * 3); m.normals.resize((size_t)nv * 3); m.faces.resize((size_t)nf * 3);
  if (col) m.colors.resize((size_t)nv * 4);
  if (kf_read_mesh(dm->ctx(), m.vertices.data(), m.normals.data(), col ? m.colors.data() : nullptr, m.faces.data()) != 0) return false;
  _meshes = std::move(m);
  return true;
}
bool MeshGeneratorMarchingcube::saveMesh(const std::string& filename) {   // :61-96
  if (!_device_weld || !weldOnDevice()) {
    if (!copyTrianglesToCPU()) return false;
    weldMesh();
    dropMeshParts();
  }
  if (!_world) {                                                 // a moved volume: the file holds world coordinates (a zero origin leaves every byte)
    int32_t o[3] = {0, 0, 0};
    CudaDeviceDataMan* dm = CudaDeviceDataMan::instance();
    if (dm->ctx() && kf_volume_origin(dm->ctx(), o) == 0)
      hkf_world_positions(_meshes.vertices.data(), _meshes.vertices.size() / 3, o, volume_cell());
  }
  // the reference returns 0 here even on success (:95); we report whether the file was written
  return _meshes.saveToFile(filename);
}
