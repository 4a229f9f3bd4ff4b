// hybkf_slabs.cpp -- HybKinectfuSlabs (hybkf_slabs.hpp) over the slab group's C ABI.
#include "hybkf_slabs.hpp"
#include <string.h>

std::vector<unsigned> SlabLayout::evenCuts(unsigned resolution, unsigned members) {
  std::vector<unsigned> cuts(1, 0);
  const unsigned nb = resolution / 8, base = members ? nb / members : 0, extra = members ? nb % members : 0;
  unsigned b = 0;
  for (unsigned r = 0; r < members; ++r) { b += base + (r < extra ? 1 : 0); cuts.push_back(b * 8); }
  return cuts;
}

HybKinectfuSlabs::~HybKinectfuSlabs() {
  delete _recorder; _recorder = nullptr;
  if (_group) kf_group_destroy(_group);
  _group = nullptr;
}

static float volume_cell() {                                   // KfVolume::cell: the fp32 quotient (tsdfVolume.h:44-46)
  const AppParams* p = AppParams::instance();
  return p->_volume_params.fVolumeMeterSize / (float)p->_volume_params.nResolution;
}

bool HybKinectfuSlabs::init(const SlabLayout& layout) {            // HybKinectfu::init (src/HybKinectfu.cpp:28-61) with a group for the data manager
  if (_inited) return false;
  const AppParams* p = AppParams::instance();
  kf_config cfg; memset(&cfg, 0, sizeof(cfg));
  cfg.depth_camera = p->_depth_camera_params; cfg.rgb_camera = p->_rgb_camera_params;
  cfg.volume.resolution = p->_volume_params.nResolution; cfg.volume.size_m = p->_volume_params.fVolumeMeterSize; cfg.volume.max_weight = p->_volume_params.fWeightMax;
  cfg.pyramid_levels = p->_icp_params.nPyramidLevels; cfg.max_triangles = p->_marchingcube_params.uMaxTriangles;
  _color = p->_switch_params.useRGBData;                       // as HybKinectfu does (CudaDeviceDataMan::init)
  cfg.has_color = _color ? 1 : 0; cfg.device = p->device;
  kf_group_params gp; memset(&gp, 0, sizeof(gp));
  gp.trunc_min = p->_depth_prepocess_params.fMinTrunc; gp.trunc_max = p->_depth_prepocess_params.fMaxTrunc;
  gp.sigma_pixel = p->_depth_prepocess_params.fSigmaPixel; gp.sigma_depth = p->_depth_prepocess_params.fSigmaDepth;
  const IcpParams& ip = p->_icp_params;
  gp.icp = {ip.nPyramidLevels, ip.fNormSinThres, ip.fDistThres, ip.fDistShake, ip.fAngleShake};
  gp.integrate = {p->_integrate_params.fSdfTruncation, p->_integrate_params.fMaxIntegrateDist};
  gp.raycast.ray_increment = p->_raycast_params.fRayIncrement;
  if (layout.cuts.size() < 2) return check(KF_GROUP_ERR_ARG);
  const uint32_t members = (uint32_t)layout.cuts.size() - 1;
  if (!layout.devices.empty() && layout.devices.size() != members) return check(KF_GROUP_ERR_ARG);
  if (layout.backend == KF_GROUP_RCCL_RANK && layout.unique_id.size() != KF_GROUP_UNIQUE_ID_BYTES) return check(KF_GROUP_ERR_ARG);
  std::vector<int32_t> devs(layout.devices.begin(), layout.devices.end());
  const uint8_t* uid = layout.unique_id.empty() ? nullptr : layout.unique_id.data();
  const int st = _color ? kf_group_create_color(&cfg, &gp, p->_switch_params.colorAngleWeight ? 1 : 0, layout.backend, members, layout.cuts.data(),
                                                devs.empty() ? nullptr : devs.data(), layout.halo, uid, layout.rank, layout.world, &_group)
                        : kf_group_create(&cfg, &gp, layout.backend, members, layout.cuts.data(), devs.empty() ? nullptr : devs.data(), layout.halo,
                                          uid, layout.rank, layout.world, &_group);
  if (!check(st)) return false;
  Mat44 camera_pose0 = Mat44::getIdentity();                   // the same expression as HybKinectfu::init
  camera_pose0.setTranslation((float)(p->_volume_params.fVolumeMeterSize / 2.0), (float)(p->_volume_params.fVolumeMeterSize / 2.0),
                              -p->_depth_prepocess_params.fMinTrunc);
  kf_mat44 k; memcpy(k.m, camera_pose0.entries, sizeof(k.m));
  if (!check(kf_group_set_pose(_group, &k))) return false;
  _pose = camera_pose0;
  if (p->_switch_params.recordTrajectory) _recorder = new TrajectoryRecorder(p->_io_params.trajWriteFilename);
  _inited = true;
  return true;
}

bool HybKinectfuSlabs::enqueueFrame(const DepthFrameData& d, const ColorFrameData& c) {
  if (!_inited) return false;
  if (_color) {
    // useRGBData: the frame's BGR image goes to every member (where the depth frame lies: host or device).  A frame without one is refused -- it
    // would fuse whatever the members' rgb maps held before
    if (!c.bgr) return check(KF_GROUP_ERR_ARG);
    const CameraParams& rc = AppParams::instance()->_rgb_camera_params;      // the members read a whole rgb-camera image (kf_upload_rgb's check)
    if (c.cols != (int)rc.cols || c.rows != (int)rc.rows) return check(KF_GROUP_ERR_ARG);
    if (!check(kf_group_frame_color(_group, d.mm, c.bgr, d.on_device ? 1 : 0, (uint32_t)d.cols, (uint32_t)d.rows, d.frameId()))) return false;
  } else if (!check(kf_group_frame(_group, d.mm, d.on_device ? 1 : 0, (uint32_t)d.cols, (uint32_t)d.rows, d.frameId()))) return false;
  _pending = true;
  return true;
}

bool HybKinectfuSlabs::processNewFrame(const DepthFrameData& d, const ColorFrameData& c) {   // :98-160
  if (!enqueueFrame(d, c) || !syncVerdict()) return false;
  if (_last_tracked && _recorder) {                             // HybKinectfu::processNewFrame: the pose in world coordinates, before the window moves
    int o[3]; volumeOrigin(o);
    const int32_t o32[3] = {o[0], o[1], o[2]};
    Mat44 w = _pose;
    hkf_world_pose(w.entries, o32, volume_cell());
    _recorder->recordCameraPose(w, d.timeStamp());
  }
  if (_last_tracked && AppParams::instance()->_volume_params.fRecentreDist > 0.f) return recentre();
  return true;
}

// ---- the moving volume (HybKinectfu::shiftVolume / volumeOrigin / recentre over the group) ------------------------------------------------------
void HybKinectfuSlabs::volumeOrigin(int out[3]) {
  int32_t o[3] = {0, 0, 0};
  if (_inited) check(kf_group_volume_origin(_group, o));
  for (int k = 0; k < 3; ++k) out[k] = (int)o[k];
}

bool HybKinectfuSlabs::shiftVolume(int dx, int dy, int dz) {
  if (!_inited) return false;
  lastTracked();                                                // the host's pose is the one the members hold
  if (!check(kf_group_shift_volume(_group, dx, dy, dz))) return false;
  if (dx == 0 && dy == 0 && dz == 0) return true;
  const float cell = volume_cell();                             // the same expression as on the device
  _pose.entries[3] = _pose.entries[3] - (float)dx * cell;
  _pose.entries[7] = _pose.entries[7] - (float)dy * cell;
  _pose.entries[11] = _pose.entries[11] - (float)dz * cell;
  return check(kf_group_raycast(_group));
}

bool HybKinectfuSlabs::recentre() {
  const AppParams* p = AppParams::instance();
  int32_t d[3];
  hkf_recentre_shift(_pose.entries, p->_volume_params.fVolumeMeterSize, p->_volume_params.nResolution, p->_volume_params.fRecentreDist, d);
  if (d[0] == 0 && d[1] == 0 && d[2] == 0) return true;
  return shiftVolume(d[0], d[1], d[2]);
}

bool HybKinectfuSlabs::syncVerdict() {
  kf_track_result r;
  if (!check(kf_group_track_result(_group, &r, 1))) return false;
  memcpy(_pose.entries, r.pose.m, sizeof(_pose.entries));
  _last_tracked = r.tracked != 0; _pending = false;
  return true;
}

bool HybKinectfuSlabs::lastTracked() {
  if (_pending) syncVerdict();
  return _last_tracked;
}

Mat44 HybKinectfuSlabs::getCameraPose() {
  lastTracked();
  return _pose;
}

// member 0 holds the merged model maps (and, in a colour group, KF_MAP_RAYCAST_RGB) after step 9 of the frame; its stream is where that step ran
bool HybKinectfuSlabs::viewModelMaps(int mode, std::vector<uint8_t>& bgra) {
  if (!_inited) return false;
  kf_ctx* ctx = nullptr;
  if (!check(kf_group_member(_group, 0, &ctx))) return false;
  if (!check(kf_view_model_maps(ctx, mode))) return false;
  uint32_t cols = 0, rows = 0;
  if (!check(kf_view_size(ctx, &cols, &rows))) return false;
  bgra.resize((size_t)cols * rows * 4);
  return check(kf_read_view(ctx, bgra.data(), bgra.size()));
}

bool HybKinectfuSlabs::renderView(const Mat44* pose, const kf_camera_params& cam, int mode, std::vector<uint8_t>& bgra) {
  if (!_inited) return false;
  const AppParams* p = AppParams::instance();
  kf_mat44 kp; const kf_mat44* tp = nullptr;
  if (pose) { memcpy(kp.m, pose->entries, sizeof(kp.m)); tp = &kp; }
  if (!check(kf_group_render_view(_group, mode, tp, &cam, p->_depth_prepocess_params.fMinTrunc, p->_depth_prepocess_params.fMaxTrunc, nullptr, nullptr))) return false;
  uint32_t cols = 0, rows = 0;
  if (!check(kf_group_view_size(_group, &cols, &rows))) return false;
  bgra.resize((size_t)cols * rows * 4);
  return check(kf_group_read_view(_group, bgra.data(), bgra.size()));
}

void HybKinectfuSlabs::generateMesh() {                        // MeshGeneratorMarchingcube::generateMesh, src/MeshGeneratorMarchingcube.cpp:23-29
  if (!_inited) return;
  const AppParams* p = AppParams::instance();
  check(kf_group_marching_cubes(_group, 300 * p->_volume_params.fVolumeMeterSize / p->_volume_params.nResolution));
}

unsigned HybKinectfuSlabs::triangleCount() {
  uint32_t n = 0;
  if (_inited) check(kf_group_triangle_count(_group, &n));
  return n;
}

bool HybKinectfuSlabs::saveMesh(const std::string& filename) {   // :61-96 on the slab-major triangle sequence
  const unsigned n = triangleCount();
  if (n == 0) return false;
  std::vector<kf_triangle> tris(n);
  if (!check(kf_group_read_triangles(_group, tris.data(), 0, n))) return false;
  _mesh.setTriangles(tris.data(), n, _color);
  _mesh.weldMesh();
  _mesh.dropMeshParts();
  int o[3]; volumeOrigin(o);                                   // a moved volume: the file holds world coordinates (a zero origin leaves every byte)
  const int32_t o32[3] = {o[0], o[1], o[2]};
  hkf_world_positions(_mesh.data().vertices.data(), _mesh.data().vertices.size() / 3, o32, volume_cell());
  return _mesh.mesh().saveToFile(filename);
}
