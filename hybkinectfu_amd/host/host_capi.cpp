// host_capi.cpp -- a flat C surface over the C++ host classes so tests and bench.py (ctypes) can drive them exactly the
// way src/MainController.cpp drives the reference: init -> per frame processNewFrame -> generateMesh/saveMesh.
#include "hybkf_host.hpp"
#include "png_reader.hpp"
#include "map_file.hpp"
#include "erase_box_voxels.hpp"
#include "map_query_voxels.hpp"
#include "edt_box_voxels.hpp"
#include "mesh_parts.hpp"
#include <string.h>

static HybKinectfu* g_app = nullptr;
static MeshGeneratorMarchingcube* g_mesh = nullptr;
static DataSourceProducerRGBDDataset* g_source = nullptr;
// the [IO] / [Switch] entries of src/config.ini that select the dataset reader, the file tracker and the trajectory recorder;
// hkf_app_init applies them after AppParams::setDefaults
static struct { std::string rgbd_dir, traj_read, traj_write; bool use_traj_file = false, record_traj = false, use_rgb = false; } g_io;

extern "C" {

// MainController::init (src/MainController.cpp:74-108) with parameters instead of config.ini
int hkf_app_init(unsigned volume_res, float volume_size, unsigned depth_cols, unsigned depth_rows, float cx, float cy, float fx, float fy,
                 int use_sdf_tracker, int host_loop, unsigned max_triangles, float sdf_trunc, float integrate_dist, float trunc_max,
                 int device, unsigned slab_z_begin, unsigned slab_z_end, unsigned slab_halo) {
  AppParams* p = AppParams::instance();
  p->setDefaults(volume_res, volume_size);
  p->_depth_camera_params = {depth_cols, depth_rows, cx, cy, fx, fy};
  p->_rgb_camera_params = p->_depth_camera_params;
  p->_switch_params.useSdfTracker = use_sdf_tracker != 0;
  p->_marchingcube_params.uMaxTriangles = max_triangles;
  if (sdf_trunc > 0) { p->_integrate_params.fSdfTruncation = sdf_trunc; p->_raycast_params.fRayIncrement = 0.7f * sdf_trunc; }
  if (integrate_dist > 0) p->_integrate_params.fMaxIntegrateDist = integrate_dist;
  if (trunc_max > 0) p->_depth_prepocess_params.fMaxTrunc = trunc_max;
  p->device = device; p->slab_z_begin = slab_z_begin; p->slab_z_end = slab_z_end; p->slab_halo = slab_halo;
  p->_io_params.rgbdReadFilename = g_io.rgbd_dir; p->_io_params.trajReadFilename = g_io.traj_read; p->_io_params.trajWriteFilename = g_io.traj_write;
  p->_switch_params.useTrajFromFile = g_io.use_traj_file; p->_switch_params.recordTrajectory = g_io.record_traj;
  p->_switch_params.useRGBData = g_io.use_rgb; p->_switch_params.useDatasetRGBD = !g_io.rgbd_dir.empty();
  delete g_app; g_app = nullptr; delete g_mesh; g_mesh = nullptr; delete g_source; g_source = nullptr;
  if (!CudaDeviceDataMan::instance()->init()) return CudaDeviceDataMan::instance()->lastError();
  g_app = new HybKinectfu();
  if (!g_app->init()) return 1002;
  g_app->poseFinder()->setHostLoop(host_loop != 0);
  g_mesh = new MeshGeneratorMarchingcube();
  return 0;
}
void hkf_app_shutdown() {
  delete g_app; g_app = nullptr; delete g_mesh; g_mesh = nullptr; delete g_source; g_source = nullptr;
  CudaDeviceDataMan::instance()->release();
}
// call BEFORE hkf_app_init; empty strings / zeros switch a feature off
void hkf_app_configure_io(const char* rgbd_dir, const char* traj_read, const char* traj_write, int use_rgb) {
  g_io.rgbd_dir = rgbd_dir ? rgbd_dir : ""; g_io.traj_read = traj_read ? traj_read : ""; g_io.traj_write = traj_write ? traj_write : "";
  g_io.use_traj_file = !g_io.traj_read.empty(); g_io.record_traj = !g_io.traj_write.empty(); g_io.use_rgb = use_rgb != 0;
}
// MainController::mainLoop body (src/MainController.cpp:33-48) on the dataset reader: read the next frame, process it.
// returns 1 tracked, 0 lost, -3 end of data / unreadable frame, <0 other errors; *stamp = the depth frame's time stamp
int hkf_app_process_dataset_frame(unsigned frame_id, double* stamp) {
  if (!g_app) return -1;
  if (!g_source) { g_source = new DataSourceProducerRGBDDataset(); if (!g_source->init()) { delete g_source; g_source = nullptr; return -4; } }
  DepthFrameData d; ColorFrameData c;
  d.frame_id = frame_id; c.frame_id = frame_id;
  if (!g_source->readNewFrame(d, c)) return -3;
  if (stamp) *stamp = d.time_stamp;
  if (!g_app->processNewFrame(d, c)) return -2;
  return g_app->lastTracked() ? 1 : 0;
}
void* hkf_app_ctx() { return CudaDeviceDataMan::instance()->ctx(); }

// HybKinectfu::processNewFrame; returns 1 when the frame was tracked, 0 when lost, <0 on error
int hkf_app_process_frame(const uint16_t* mm, int on_device, unsigned frame_id, double stamp) {
  if (!g_app) return -1;
  const CameraParams& c = AppParams::instance()->_depth_camera_params;
  DepthFrameData d; d.mm = mm; d.cols = (int)c.cols; d.rows = (int)c.rows; d.frame_id = frame_id; d.time_stamp = stamp; d.on_device = on_device != 0;
  ColorFrameData col;
  if (!g_app->processNewFrame(d, col)) return -2;
  return g_app->lastTracked() ? 1 : 0;
}
// the same with the frame's BGR image (host memory, rgb camera's size; used when hkf_app_configure_io switched useRGBData on)
int hkf_app_process_frame_color(const uint16_t* mm, const uint8_t* bgr, unsigned frame_id, double stamp) {
  if (!g_app) return -1;
  const CameraParams& c = AppParams::instance()->_depth_camera_params;
  const CameraParams& rc = AppParams::instance()->_rgb_camera_params;
  DepthFrameData d; d.mm = mm; d.cols = (int)c.cols; d.rows = (int)c.rows; d.frame_id = frame_id; d.time_stamp = stamp; d.on_device = false;
  ColorFrameData col; col.bgr = bgr; col.cols = (int)rc.cols; col.rows = (int)rc.rows; col.frame_id = frame_id; col.time_stamp = stamp;
  if (!g_app->processNewFrame(d, col)) return -2;
  return g_app->lastTracked() ? 1 : 0;
}
// streaming: no host synchronisation
int hkf_app_enqueue_frame(const uint16_t* mm, int on_device, unsigned frame_id) {
  if (!g_app) return -1;
  const CameraParams& c = AppParams::instance()->_depth_camera_params;
  DepthFrameData d; d.mm = mm; d.cols = (int)c.cols; d.rows = (int)c.rows; d.frame_id = frame_id; d.on_device = on_device != 0;
  ColorFrameData col;
  return g_app->enqueueFrame(d, col) ? 0 : -2;
}
int hkf_app_get_pose(float out16[16]) {
  if (!g_app) return -1;
  Mat44 m = g_app->getCameraPose();
  memcpy(out16, m.entries, 64);
  return g_app->lastTracked() ? 1 : 0;
}
// HybKinectfu::renderView / viewModelMaps: the picture into `out` (cols * rows * 4 bytes: b, g, r, a).  pose16 NULL: the current camera pose.
// returns 0, -1 without an application, -2 when the view failed (CudaDeviceDataMan::lastError has the status), -3 when `out` is too small
static int copy_view(const std::vector<uint8_t>& img, uint8_t* out, size_t out_cap) {
  if (!out || out_cap < img.size()) return -3;
  memcpy(out, img.data(), img.size());
  return 0;
}
int hkf_app_render_view(int mode, const float* pose16, unsigned cols, unsigned rows, float cx, float cy, float fx, float fy, uint8_t* out, size_t out_cap) {
  if (!g_app) return -1;
  Mat44 m; if (pose16) memcpy(m.entries, pose16, 64);
  const kf_camera_params cam = {cols, rows, cx, cy, fx, fy};
  std::vector<uint8_t> img;
  if (!g_app->renderView(pose16 ? &m : nullptr, cam, mode, img)) return -2;
  return copy_view(img, out, out_cap);
}
// HybKinectfu::renderViewAt / renderMapView with hkf_app_render_view's arguments and return values.  frame3: the window's origin in voxels of the first
// cube; pose16 of hkf_app_render_view_at in that frame's coordinates (NULL: the current camera pose), world_pose16 of hkf_app_render_map_view in the first cube's
int hkf_app_render_view_at(int mode, const int* frame3, const float* pose16, unsigned cols, unsigned rows, float cx, float cy, float fx, float fy, uint8_t* out, size_t out_cap) {
  if (!g_app) return -1;
  if (!frame3) return -2;
  Mat44 m; if (pose16) memcpy(m.entries, pose16, 64);
  const kf_camera_params cam = {cols, rows, cx, cy, fx, fy};
  std::vector<uint8_t> img;
  if (!g_app->renderViewAt(mode, frame3, pose16 ? &m : nullptr, cam, img)) return -2;
  return copy_view(img, out, out_cap);
}
int hkf_app_render_map_view(int mode, const float* world_pose16, unsigned cols, unsigned rows, float cx, float cy, float fx, float fy, uint8_t* out, size_t out_cap) {
  if (!g_app) return -1;
  if (!world_pose16) return -2;
  Mat44 m; memcpy(m.entries, world_pose16, 64);
  const kf_camera_params cam = {cols, rows, cx, cy, fx, fy};
  std::vector<uint8_t> img;
  if (!g_app->renderMapView(mode, m, cam, img)) return -2;
  return copy_view(img, out, out_cap);
}
int hkf_app_view_model_maps(int mode, uint8_t* out, size_t out_cap) {
  if (!g_app) return -1;
  std::vector<uint8_t> img;
  if (!g_app->viewModelMaps(mode, img)) return -2;
  return copy_view(img, out, out_cap);
}
// the moving volume: HybKinectfu::shiftVolume / volumeOrigin, and AppParams::_volume_params.fRecentreDist (call AFTER hkf_app_init, which restores the
// defaults; 0 = off).  hkf_app_shift_volume: 1 shifted, 0 refused, -1 without an application
int hkf_app_shift_volume(int dx, int dy, int dz) { if (!g_app) return -1; return g_app->shiftVolume(dx, dy, dz) ? 1 : 0; }
int hkf_app_volume_origin(int out3[3]) { if (!g_app) return -1; g_app->volumeOrigin(out3); return 0; }
int hkf_app_set_recentre(float dist) { if (!g_app) return -1; AppParams::instance()->_volume_params.fRecentreDist = dist; return 0; }
// AppParams::_volume_params.nStreamMeshTriangles (call AFTER hkf_app_init, which restores the defaults; 0 = off): HybKinectfu::setStreamMesh.
// hkf_app_set_stream_mesh: 0 ok, -1 without an application, -2 refused (CudaDeviceDataMan::lastError has the status).  hkf_app_world_soup_count: the
// triangles streamed out so far, -1 without an application
int hkf_app_set_stream_mesh(unsigned max_triangles) { if (!g_app) return -1; return g_app->setStreamMesh(max_triangles) ? 0 : -2; }
int hkf_app_world_soup_count() { if (!g_app) return -1; return (int)g_app->worldSoupCount(); }
// AppParams::_volume_params.nBrickStoreBricks (call AFTER hkf_app_init, which restores the defaults; 0 = off): HybKinectfu::setBrickStore.
// hkf_app_set_brick_store: 0 ok, -1 without an application, -2 refused.  hkf_app_brick_store_count: out3 = bricks held, dropped, restored; -2 when the
// read failed
int hkf_app_set_brick_store(unsigned max_bricks) { if (!g_app) return -1; return g_app->setBrickStore(max_bricks) ? 0 : -2; }
int hkf_app_brick_store_count(uint64_t out3[3]) {
  if (!g_app || !out3) return -1;
  unsigned held = 0; uint64_t dropped = 0, restored = 0;
  if (!g_app->brickStoreCounts(held, dropped, restored)) return -2;
  out3[0] = held; out3[1] = dropped; out3[2] = restored;
  return 0;
}
// The map on disk: HybKinectfu::saveMap / loadMap / frameId.  1 done, 0 refused or failed (stderr says why), -1 without an application.
// hkf_map_file_info needs neither application nor device: every check of the reader (map_file.hpp), then the header's fields -- u32x4[0..3] = version,
// resolution, brick edge, colour flag; f32x2 = size, max weight; origin3; frame_id; pose16; u64x2 = n_bricks, dropped.  Any pointer may be NULL.
// Returns 0 or the reader's HKF_MAP_ERR_* (negative).
int hkf_app_save_map(const char* path) { if (!g_app) return -1; return path && g_app->saveMap(path) ? 1 : 0; }
int hkf_app_load_map(const char* path) { if (!g_app) return -1; return path && g_app->loadMap(path) ? 1 : 0; }
// HybKinectfu::loadMapCoarser: a file of 2, 4 or 8 times this instance's resolution, halved on the device while it is loaded.  Same answers as hkf_app_load_map
int hkf_app_load_map_coarser(const char* path) { if (!g_app) return -1; return path && g_app->loadMapCoarser(path) ? 1 : 0; }
// HybKinectfu::mergeMap, the offset in whole bricks: 1 merged, 0 refused or failed, -1 without an application
int hkf_app_merge_map(const char* path, int ox, int oy, int oz) {
  if (!g_app) return -1;
  const int off[3] = {ox, oy, oz};
  return path && g_app->mergeMap(path, off) ? 1 : 0;
}
// HybKinectfu::mergeMap under a rigid transform: m = the row-major 4x4 from the file's world frame to this session's, in metres.  Same answers
int hkf_app_merge_map_rigid(const char* path, const float m[16]) {
  if (!g_app) return -1;
  if (!path || !m) return 0;
  Mat44 t;
  memcpy(t.entries, m, 64);
  return g_app->mergeMap(path, t) ? 1 : 0;
}
// HybKinectfu::alignMap: guess and found row-major 4x4 in metres, report a kf_align_report (may be NULL).  1 converged, 0 refused, failed or not converged
// (found and report are then written only when the alignment ran), -1 without an application
int hkf_app_align_map(const char* path, const float guess[16], float found[16], void* report) {
  if (!g_app) return -1;
  if (!path || !guess || !found) return 0;
  Mat44 g, f;
  memcpy(g.entries, guess, 64); memcpy(f.entries, guess, 64);
  const bool ok = g_app->alignMap(path, g, f, (kf_align_report*)report);
  memcpy(found, f.entries, 64);
  return ok ? 1 : 0;
}
// HybKinectfu::eraseMapBox (lo, hi: WORLD metres) and eraseMapWeak: 1 erased, 0 refused or failed, -1 without an application.  out2 (may be NULL): bricks removed,
// observed voxels cleared (eraseMapWeak: out1, bricks removed).  hkf_erase_map_box_voxels needs no application: the voxel box of a box in metres
int hkf_app_erase_map_box(const float lo_m[3], const float hi_m[3], int keep_inside, uint64_t out2[2]) {
  if (!g_app) return -1;
  if (!lo_m || !hi_m) return 0;
  unsigned removed = 0; uint64_t cleared = 0;
  const bool ok = g_app->eraseMapBox(lo_m, hi_m, keep_inside != 0, &removed, &cleared);
  if (out2) { out2[0] = removed; out2[1] = cleared; }
  return ok ? 1 : 0;
}
int hkf_app_erase_map_weak(float min_weight, uint64_t out1[1]) {
  if (!g_app) return -1;
  unsigned removed = 0;
  const bool ok = g_app->eraseMapWeak(min_weight, &removed);
  if (out1) out1[0] = removed;
  return ok ? 1 : 0;
}
int hkf_erase_map_box_voxels(const float lo_m[3], const float hi_m[3], float cell, int32_t lo_vox[3], int32_t hi_vox[3]) {
  if (!lo_m || !hi_m || !lo_vox || !hi_vox) return -1;
  hkf_erase_box_voxels(lo_m, hi_m, cell, lo_vox, hi_vox);
  return 0;
}
// HybKinectfu::relocalise: 1 accepted (the next frame tracks from the found pose), 0 refused or not accepted (nothing of the session changed), -1 without an
// application.  params NULL: the defaults.  hkf_reloc_defaults_get / hkf_reloc_points / hkf_reloc_lattice / hkf_reloc_rank need no application (reloc_search.hpp).
int hkf_app_relocalise(const uint16_t* mm, unsigned frame_id, const RelocParams* params, RelocReport* report) {
  if (!g_app) return -1;
  const CameraParams& c = AppParams::instance()->_depth_camera_params;
  DepthFrameData d; d.mm = mm; d.cols = (int)c.cols; d.rows = (int)c.rows; d.frame_id = frame_id; d.on_device = false;
  const RelocParams def = hkf_reloc_defaults();
  return g_app->relocalise(d, params ? *params : def, report) ? 1 : 0;
}
void hkf_reloc_defaults_get(RelocParams* out) { if (out) *out = hkf_reloc_defaults(); }
uint32_t hkf_reloc_points(const float* verts, uint32_t n_pix, float cell, uint32_t max_points, float* out, float* median_depth_m) {
  return reloc_points(verts, n_pix, cell, max_points, out, median_depth_m);
}
int64_t hkf_reloc_lattice(const double* centre, const int32_t* n, double trans_step, double rot_step, double* out, int64_t cap) {
  return reloc_lattice(centre, n, trans_step, rot_step, out, cap);
}
uint32_t hkf_reloc_rank(const kf_pose_score* scores, uint32_t n, uint32_t min_obs, uint32_t M, uint32_t* best) { return reloc_rank(scores, n, min_obs, M, best); }
// HybKinectfu::sampleMap / castMapRays (positions, t: WORLD metres): 1 done, 0 refused or failed, -1 without an application.  Any output may be NULL.
// hkf_map_query_voxels needs no application: count3 coordinates in metres as fp64 voxel positions
int hkf_app_sample_map(const double* world_m, uint32_t n, float* distance_m, float* weight, float* gradient, uint8_t* color) {
  if (!g_app) return -1;
  return g_app->sampleMap(world_m, n, distance_m, weight, gradient, color) ? 1 : 0;
}
int hkf_app_cast_map_rays(const double* origin_m, const float* dir, const float* t_min_m, const float* t_max_m, uint32_t n, uint8_t* status, float* t_m, float* normal,
                          uint8_t* color, float* weight) {
  if (!g_app) return -1;
  return g_app->castMapRays(origin_m, dir, t_min_m, t_max_m, n, status, t_m, normal, color, weight) ? 1 : 0;
}
int hkf_map_query_voxels(const double* world_m, uint32_t count3, float cell, double* vox) {
  if (!world_m || !vox) return -1;
  hkf_query_voxels(world_m, count3, cell, vox);
  return 0;
}
// HybKinectfu::distanceField (the box and max_dist_m in WORLD metres): 1 done, 0 refused or failed, -1 without an application.  hkf_app_distance_field_box
// computes nothing on the device: the voxel box and the clamped radius the field would have, so that the caller can size dist (float) and cls (a byte) --
// capacity items each, nx * ny * nz are needed; a capacity below that is refused with nothing written.  lo_vox, dims, radius (may be NULL): as found.
int hkf_app_distance_field_box(const float lo_m[3], const float hi_m[3], float max_dist_m, int32_t lo_vox[3], uint32_t dims[3], uint32_t* radius) {
  if (!g_app) return -1;
  if (!lo_m || !hi_m || !lo_vox || !dims) return 0;
  const float cell = AppParams::instance()->_volume_params.fVolumeMeterSize / (float)AppParams::instance()->_volume_params.nResolution;
  if (radius) *radius = hkf_edt_radius(max_dist_m, cell);
  uint64_t count = 0;
  return hkf_edt_box_voxels(lo_m, hi_m, cell, lo_vox, dims) && hkf_edt_voxel_count(dims, &count) ? 1 : 0;       // (0 also for a box of more than HKF_EDT_MAX_VOXELS voxels)
}
int hkf_app_distance_field(const float lo_m[3], const float hi_m[3], float max_dist_m, float level, uint32_t site_mask, uint64_t capacity, float* dist, uint8_t* cls,
                           int32_t lo_vox[3], uint32_t dims[3], uint32_t* radius) {
  if (!g_app) return -1;
  if (!lo_m || !hi_m || !dist || !cls) return 0;
  int32_t lo[3]; uint32_t n3[3], r = 0;
  uint64_t count = 0;
  if (hkf_app_distance_field_box(lo_m, hi_m, max_dist_m, lo, n3, &r) != 1 || !hkf_edt_voxel_count(n3, &count) || count > capacity) return 0;
  std::vector<float> d; std::vector<uint8_t> c;
  if (!g_app->distanceField(lo_m, hi_m, max_dist_m, level, site_mask, d, c, n3, &r, lo)) return 0;
  memcpy(dist, d.data(), d.size() * sizeof(float)); memcpy(cls, c.data(), c.size());
  if (lo_vox) memcpy(lo_vox, lo, sizeof(lo));
  if (dims) memcpy(dims, n3, sizeof(n3));
  if (radius) *radius = r;
  return 1;
}
int hkf_app_frame_id() { if (!g_app) return -1; return (int)g_app->frameId(); }
int hkf_map_file_info(const char* path, uint32_t* u32x4, float* f32x2, int32_t* origin3, uint32_t* frame_id, float* pose16, uint64_t* u64x2) {
  HkfMapHeader h;
  const int st = hkf_map_info(path, &h);
  if (st != HKF_MAP_OK) return st;
  if (u32x4) { u32x4[0] = h.version; u32x4[1] = h.resolution; u32x4[2] = h.brick_edge; u32x4[3] = h.has_color; }
  if (f32x2) { f32x2[0] = h.size_m; f32x2[1] = h.max_weight; }
  if (origin3) memcpy(origin3, h.origin_vox, 12);
  if (frame_id) *frame_id = h.frame_id;
  if (pose16) memcpy(pose16, h.pose, 64);
  if (u64x2) { u64x2[0] = h.n_bricks; u64x2[1] = h.dropped; }
  return 0;
}
// MeshGeneratorMarchingcube::setMapMesh (call AFTER hkf_app_init, which restores the defaults): with a brick store reserved, generateMesh builds the map mesh
int hkf_app_set_map_mesh(int on) { if (!g_mesh) return -1; g_mesh->setMapMesh(on != 0); return 0; }
int hkf_app_generate_mesh() { if (!g_mesh) return -1; g_mesh->generateMesh(); return (int)g_mesh->triangleCount(); }
int hkf_app_save_mesh(const char* filename, unsigned* n_vertices, unsigned* n_faces) {
  if (!g_mesh) return -1;
  bool ok = g_mesh->saveMesh(filename);
  if (n_vertices) *n_vertices = (unsigned)(g_mesh->mesh().vertices.size() / 3);
  if (n_faces) *n_faces = (unsigned)(g_mesh->mesh().faces.size() / 3);
  return ok ? 1 : 0;
}
// MeshGeneratorMarchingcube::setDeviceWeld: the application's saveMesh welds on the device from now on (0: on the host again)
int hkf_app_set_device_weld(int on) { if (!g_mesh) return -1; g_mesh->setDeviceWeld(on != 0); return 0; }
// MeshGeneratorMarchingcube::setMinPartFaces: the application's saveMesh drops the mesh's small parts after the weld (0, 0: off again)
int hkf_app_set_min_part_faces(unsigned n, int largest_only) { if (!g_mesh) return -1; g_mesh->setMinPartFaces(n, largest_only != 0); return 0; }

// ---- GPU-free mesh post-processing on a caller-supplied triangle soup (kf_triangle layout) ---------------------------------------
static MeshGeneratorMarchingcube* g_soup = nullptr;
int hkf_mesh_from_soup(const void* triangles, unsigned n, int with_color, unsigned* n_vertices, unsigned* n_faces) {
  delete g_soup; g_soup = new MeshGeneratorMarchingcube();
  g_soup->setTriangles((const kf_triangle*)triangles, n, with_color != 0);
  g_soup->weldMesh();
  if (n_vertices) *n_vertices = (unsigned)(g_soup->mesh().vertices.size() / 3);
  if (n_faces) *n_faces = (unsigned)(g_soup->mesh().faces.size() / 3);
  return 0;
}
// which: 0 = the soup mesh (hkf_mesh_from_soup), 1 = the application's mesh (after hkf_app_save_mesh)
static const MeshData* mesh_of(int which) { return which == 0 ? (g_soup ? &g_soup->mesh() : nullptr) : (g_mesh ? &g_mesh->mesh() : nullptr); }
int hkf_mesh_sizes(int which, unsigned* n_vertices, unsigned* n_faces, unsigned* n_colors) {
  const MeshData* m = mesh_of(which); if (!m) return -1;
  *n_vertices = (unsigned)(m->vertices.size() / 3); *n_faces = (unsigned)(m->faces.size() / 3); *n_colors = (unsigned)(m->colors.size() / 4);
  return 0;
}
int hkf_mesh_read(int which, float* vertices, float* normals, float* colors, unsigned* faces) {
  const MeshData* m = mesh_of(which); if (!m) return -1;
  if (vertices) memcpy(vertices, m->vertices.data(), m->vertices.size() * 4);
  if (normals) memcpy(normals, m->normals.data(), m->normals.size() * 4);
  if (colors) memcpy(colors, m->colors.data(), m->colors.size() * 4);
  if (faces) memcpy(faces, m->faces.data(), m->faces.size() * 4);
  return 0;
}
// the parts of the mesh on one host thread (mesh_parts.hpp; the rule: include/hybkf.h): labels / part_faces n_vertices words each, either may be null
int hkf_mesh_parts(int which, unsigned* labels, unsigned* part_faces) {
  const MeshData* m = mesh_of(which); if (!m) return -1;
  std::vector<unsigned> l, s;
  meshParts(*m, l, s);
  if (labels && !l.empty()) memcpy(labels, l.data(), l.size() * 4);
  if (part_faces && !s.empty()) memcpy(part_faces, s.data(), s.size() * 4);
  return 0;
}
// dropParts on the mesh itself
int hkf_mesh_drop_parts(int which, unsigned min_faces, int largest_only) {
  MeshData* m = which == 0 ? (g_soup ? &g_soup->mesh() : nullptr) : (g_mesh ? &g_mesh->mesh() : nullptr); if (!m) return -1;
  dropParts(*m, min_faces, largest_only != 0);
  return 0;
}
int hkf_mesh_save(int which, const char* filename) { const MeshData* m = mesh_of(which); return m && m->saveToFile(filename) ? 1 : 0; }

// ---- GPU-free entry points of the dataset / trajectory code (CPU tests) ---------------------------------------------------------
// reads frames [0, n) of a TUM directory into caller buffers: depth n x rows x cols u16 mm, bgr n x rows x cols x 3 (may be null)
int hkf_dataset_read(const char* dir, unsigned cols, unsigned rows, int with_color, int n, uint16_t* depth_mm, uint8_t* bgr,
                     double* depth_stamps, double* color_stamps) {
  AppParams* p = AppParams::instance();
  p->_io_params.rgbdReadFilename = dir ? dir : ""; p->_switch_params.useRGBData = with_color != 0;
  p->_depth_camera_params.cols = cols; p->_depth_camera_params.rows = rows;
  DataSourceProducerRGBDDataset src;
  if (!src.init()) return -4;
  int k = 0;
  for (; k < n; ++k) {
    DepthFrameData d; ColorFrameData c;
    if (!src.readNewFrame(d, c)) break;
    memcpy(depth_mm + (size_t)k * cols * rows, d.mm, (size_t)cols * rows * 2);
    if (depth_stamps) depth_stamps[k] = d.time_stamp;
    if (with_color && bgr) memcpy(bgr + (size_t)k * c.cols * c.rows * 3, c.bgr, (size_t)c.cols * c.rows * 3);
    if (with_color && color_stamps) color_stamps[k] = c.time_stamp;
  }
  return k;
}
int hkf_png_read(const char* path, unsigned* width, unsigned* height, unsigned* channels, unsigned* bit_depth, uint8_t* out, size_t out_cap) {
  PngImage img;
  if (!readPng(path, img)) return 0;
  *width = img.width; *height = img.height; *channels = img.channels; *bit_depth = img.bit_depth;
  if (out && img.data.size() <= out_cap) memcpy(out, img.data.data(), img.data.size());
  return 1;
}
void hkf_pyrdown16(const uint16_t* src, int cols, int rows, uint16_t* dst) {
  std::vector<uint16_t> o; DataSourceProducerRGBDDataset::pyrDown16(src, cols, rows, o); memcpy(dst, o.data(), o.size() * 2);
}
void hkf_quat_from_pose(const float pose16[16], float q_xyzw[4]) { Mat44 m; memcpy(m.entries, pose16, 64); TrajectoryRecorder::quaternionFromRotation(m, q_xyzw); }
void hkf_pose_from_quat(const float t[3], const float q_xyzw[4], float pose16[16]) {
  Mat44 m = CameraPoseFinderFromFile::transformFromQuaternion(t, q_xyzw); memcpy(pose16, m.entries, 64);
}
int hkf_trajectory_write(const char* path, const float* poses16, const double* stamps, int n) {
  TrajectoryRecorder rec(path);
  for (int k = 0; k < n; ++k) { Mat44 m; memcpy(m.entries, poses16 + 16 * k, 64); if (!rec.recordCameraPose(m, stamps[k])) return k; }
  return n;
}
// nearest-in-time association over a list file: out_stamps[k] = stamp matched to targets[k] (-1: ran off the end)
int hkf_table_nearest(const char* path, int header_lines, const double* targets, int n, double* out_stamps) {
  TimedTable t;
  if (!t.load(path, header_lines, false)) return -1;
  for (int k = 0; k < n; ++k) { TimedRow r; out_stamps[k] = t.nearest(targets[k], r) ? r.stamp : -1.0; }
  return (int)t.size();
}
}
