// slabs_capi.cpp -- a flat C surface over HybKinectfuSlabs (hybkf_slabs.hpp) for ctypes callers, in the style of host_capi.cpp's hkf_app_*.
#include "hybkf_slabs.hpp"
#include <string.h>

static HybKinectfuSlabs* g_slabs = nullptr;
#include <string>

static struct { bool use_rgb = false, angle_weight = true; } g_switch;      // [Switch] useRGBData / colorAngleWeight, applied by hkf_slabs_init
static std::string g_traj_write;                                            // [IO] trajWriteFilename + [Switch] recordTrajectory, applied by hkf_slabs_init

extern "C" {

// AppParams::setDefaults + the camera / volume / truncation arguments hkf_app_init takes, then HybKinectfuSlabs::init over `members`
// slabs cut at cuts[0..members] (NULL: even slabs); devices: one per member (NULL: `device` for all)
int hkf_slabs_init(unsigned volume_res, float volume_size, unsigned depth_cols, unsigned depth_rows, float cx, float cy, float fx, float fy,
                   unsigned max_triangles, float sdf_trunc, float integrate_dist, float trunc_max, int device,
                   int backend, unsigned members, const unsigned* cuts, const int* devices, unsigned halo) {
  AppParams* p = AppParams::instance();
  p->setDefaults(volume_res, volume_size);
  p->_depth_camera_params = {depth_cols, depth_rows, cx, cy, fx, fy};
  p->_rgb_camera_params = p->_depth_camera_params;
  p->_marchingcube_params.uMaxTriangles = max_triangles;
  if (sdf_trunc > 0) { p->_integrate_params.fSdfTruncation = sdf_trunc; p->_raycast_params.fRayIncrement = 0.7f * sdf_trunc; }
  if (integrate_dist > 0) p->_integrate_params.fMaxIntegrateDist = integrate_dist;
  if (trunc_max > 0) p->_depth_prepocess_params.fMaxTrunc = trunc_max;
  p->device = device;
  p->_switch_params.useRGBData = g_switch.use_rgb;
  if (g_switch.use_rgb) p->_switch_params.colorAngleWeight = g_switch.angle_weight;
  p->_io_params.trajWriteFilename = g_traj_write; p->_switch_params.recordTrajectory = !g_traj_write.empty();
  delete g_slabs; g_slabs = nullptr;
  SlabLayout layout;
  layout.backend = backend;
  if (members == 0 || members > KF_GROUP_MAX_MEMBERS) return KF_GROUP_ERR_ARG;
  layout.cuts = cuts ? std::vector<unsigned>(cuts, cuts + members + 1) : SlabLayout::evenCuts(volume_res, members);
  if (devices) layout.devices.assign(devices, devices + members);
  layout.halo = halo;
  g_slabs = new HybKinectfuSlabs();
  if (!g_slabs->init(layout)) { const int e = g_slabs->lastError(); delete g_slabs; g_slabs = nullptr; return e ? e : KF_GROUP_ERR_STATE; }
  return 0;
}
// call BEFORE hkf_slabs_init: useRGBData (and, with it, colorAngleWeight) for the next init; off until called
void hkf_slabs_configure_color(int use_rgb, int angle_weight) { g_switch.use_rgb = use_rgb != 0; g_switch.angle_weight = angle_weight != 0; }
// call BEFORE hkf_slabs_init: the trajectory file of the next init (NULL / empty: none), as hkf_app_configure_io's traj_write
void hkf_slabs_configure_traj(const char* traj_write) { g_traj_write = traj_write ? traj_write : ""; }
void hkf_slabs_shutdown() { delete g_slabs; g_slabs = nullptr; }
void* hkf_slabs_group() { return g_slabs ? (void*)g_slabs->group() : nullptr; }

// HybKinectfuSlabs::processNewFrame; 1 tracked, 0 lost, <0 error
int hkf_slabs_process_frame(const uint16_t* mm, int on_device, unsigned frame_id) {
  if (!g_slabs) return -1;
  const CameraParams& c = AppParams::instance()->_depth_camera_params;
  DepthFrameData d; d.mm = mm; d.cols = (int)c.cols; d.rows = (int)c.rows; d.frame_id = frame_id; d.on_device = on_device != 0;
  ColorFrameData col;
  if (!g_slabs->processNewFrame(d, col)) return -2;
  return g_slabs->lastTracked() ? 1 : 0;
}
// the same with the frame's time stamp (what the trajectory recorder writes), as hkf_app_process_frame
int hkf_slabs_process_frame_stamped(const uint16_t* mm, int on_device, unsigned frame_id, double stamp) {
  if (!g_slabs) return -1;
  const CameraParams& c = AppParams::instance()->_depth_camera_params;
  DepthFrameData d; d.mm = mm; d.cols = (int)c.cols; d.rows = (int)c.rows; d.frame_id = frame_id; d.time_stamp = stamp; d.on_device = on_device != 0;
  ColorFrameData col;
  if (!g_slabs->processNewFrame(d, col)) return -2;
  return g_slabs->lastTracked() ? 1 : 0;
}
int hkf_slabs_enqueue_frame(const uint16_t* mm, int on_device, unsigned frame_id) {
  if (!g_slabs) return -1;
  const CameraParams& c = AppParams::instance()->_depth_camera_params;
  DepthFrameData d; d.mm = mm; d.cols = (int)c.cols; d.rows = (int)c.rows; d.frame_id = frame_id; d.on_device = on_device != 0;
  ColorFrameData col;
  return g_slabs->enqueueFrame(d, col) ? 0 : -2;
}
// the same two with the frame's BGR image (rows x cols x 3 bytes, where mm lies: host or device; NULL: none)
int hkf_slabs_process_frame_color(const uint16_t* mm, const uint8_t* bgr, int on_device, unsigned frame_id) {
  if (!g_slabs) return -1;
  const CameraParams& c = AppParams::instance()->_depth_camera_params;
  const CameraParams& rc = AppParams::instance()->_rgb_camera_params;
  DepthFrameData d; d.mm = mm; d.cols = (int)c.cols; d.rows = (int)c.rows; d.frame_id = frame_id; d.on_device = on_device != 0;
  ColorFrameData col; col.bgr = bgr; col.cols = (int)rc.cols; col.rows = (int)rc.rows; col.frame_id = frame_id;
  if (!g_slabs->processNewFrame(d, col)) return -2;
  return g_slabs->lastTracked() ? 1 : 0;
}
int hkf_slabs_enqueue_frame_color(const uint16_t* mm, const uint8_t* bgr, int on_device, unsigned frame_id) {
  if (!g_slabs) return -1;
  const CameraParams& c = AppParams::instance()->_depth_camera_params;
  const CameraParams& rc = AppParams::instance()->_rgb_camera_params;
  DepthFrameData d; d.mm = mm; d.cols = (int)c.cols; d.rows = (int)c.rows; d.frame_id = frame_id; d.on_device = on_device != 0;
  ColorFrameData col; col.bgr = bgr; col.cols = (int)rc.cols; col.rows = (int)rc.rows; col.frame_id = frame_id;
  return g_slabs->enqueueFrame(d, col) ? 0 : -2;
}
int hkf_slabs_get_pose(float out16[16]) {
  if (!g_slabs) return -1;
  Mat44 m = g_slabs->getCameraPose();
  memcpy(out16, m.entries, 64);
  return g_slabs->lastTracked() ? 1 : 0;
}
int hkf_slabs_generate_mesh() { if (!g_slabs) return -1; g_slabs->generateMesh(); return (int)g_slabs->triangleCount(); }
int hkf_slabs_save_mesh(const char* filename, unsigned* n_vertices, unsigned* n_faces) {
  if (!g_slabs) return -1;
  const bool ok = g_slabs->saveMesh(filename);
  if (n_vertices) *n_vertices = (unsigned)(g_slabs->mesh().vertices.size() / 3);
  if (n_faces) *n_faces = (unsigned)(g_slabs->mesh().faces.size() / 3);
  return ok ? 1 : 0;
}
// HybKinectfuSlabs::viewModelMaps into `out` (cols * rows * 4 bytes); 0, -1 without a group, -2 view failed, -3 `out` too small
int hkf_slabs_view_model_maps(int mode, uint8_t* out, size_t out_cap) {
  if (!g_slabs) return -1;
  std::vector<uint8_t> img;
  if (!g_slabs->viewModelMaps(mode, img)) return -2;
  if (!out || out_cap < img.size()) return -3;
  memcpy(out, img.data(), img.size());
  return 0;
}
// HybKinectfuSlabs::renderView, with hkf_app_render_view's arguments and return values (pose16 NULL: the current camera pose)
int hkf_slabs_render_view(int mode, const float* pose16, unsigned cols, unsigned rows, float cx, float cy, float fx, float fy, uint8_t* out, size_t out_cap) {
  if (!g_slabs) return -1;
  Mat44 m; if (pose16) memcpy(m.entries, pose16, 64);
  const kf_camera_params cam = {cols, rows, cx, cy, fx, fy};
  std::vector<uint8_t> img;
  if (!g_slabs->renderView(pose16 ? &m : nullptr, cam, mode, img)) return -2;
  if (!out || out_cap < img.size()) return -3;
  memcpy(out, img.data(), img.size());
  return 0;
}
// the moving volume: HybKinectfuSlabs::shiftVolume / volumeOrigin, and AppParams::_volume_params.fRecentreDist (call AFTER hkf_slabs_init, which restores
// the defaults; 0 = off), as hkf_app_*.  hkf_slabs_shift_volume: 1 shifted, 0 refused, -1 without a group
int hkf_slabs_shift_volume(int dx, int dy, int dz) { if (!g_slabs) return -1; return g_slabs->shiftVolume(dx, dy, dz) ? 1 : 0; }
int hkf_slabs_volume_origin(int out3[3]) { if (!g_slabs) return -1; g_slabs->volumeOrigin(out3); return 0; }
int hkf_slabs_set_recentre(float dist) { if (!g_slabs) return -1; AppParams::instance()->_volume_params.fRecentreDist = dist; return 0; }
// HybKinectfuSlabs::saveMap / loadMap: 0 refused -- always: the map file is built on the brick store, which a slab group does not have --, -1 without a group
int hkf_slabs_save_map(const char* path) { if (!g_slabs) return -1; return path && g_slabs->saveMap(path) ? 1 : 0; }
int hkf_slabs_load_map(const char* path) { if (!g_slabs) return -1; return path && g_slabs->loadMap(path) ? 1 : 0; }
// merging maps is built on the brick store too: always -1, nothing touched
int hkf_slabs_merge_map(const char*, int, int, int) { return -1; }
int hkf_slabs_merge_map_rigid(const char*, const float*) { return -1; }
int hkf_slabs_align_map(const char*, const float*, float*, void*) { return -1; }
int hkf_slabs_load_map_coarser(const char*) { return -1; }
// erasing from the map is built on the brick store too: always -1, nothing touched
int hkf_slabs_erase_map_box(const float*, const float*, int, uint64_t*) { return -1; }
int hkf_slabs_erase_map_weak(float, uint64_t*) { return -1; }
// querying the map reads window and brick store: always -1, nothing written
// HybKinectfuSlabs::relocalise: slab groups hold part of a window each and no store -- always refused, nothing touched
int hkf_slabs_relocalise(const uint16_t*, unsigned, const RelocParams*, RelocReport*) { return -1; }
int hkf_slabs_sample_map(const double*, uint32_t, float*, float*, float*, uint8_t*) { return -1; }
int hkf_slabs_cast_map_rays(const double*, const float*, const float*, const float*, uint32_t, uint8_t*, float*, float*, uint8_t*, float*) { return -1; }
// so does the distance field: always -1, nothing written
int hkf_slabs_distance_field(const float*, const float*, float, float, uint32_t, uint64_t, float*, uint8_t*, int32_t*, uint32_t*, uint32_t*) { return -1; }
int hkf_slabs_last_error() { return g_slabs ? g_slabs->lastError() : 0; }
}
