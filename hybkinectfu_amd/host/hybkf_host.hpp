// hybkf_host.hpp -- C++ host classes above the C ABI (include/hybkf.h), mirroring the reference's plugin surface for the
// per-frame path: AppParams, FrameData, CameraPoseFinder{,ICP,SDF}, HybKinectfu, MeshGenerator{,Marchingcube}.
// Same class and method names, argument meaning and bool/void error behaviour as the reference, so a caller written
// against src/HybKinectfu.h, src/CameraPoseFinder.h and src/MeshGenerator.h compiles against this header unchanged apart
// from FrameData, which is a plain view instead of a cv::Mat wrapper (OpenCV is not part of the hot path).
// Paths cited are relative to /root/reference.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "../../include/hybkf.h"
#include "reloc_search.hpp"

// ---- src/AppParams.h:12-95,156-166 -----------------------------------------------------------------------------------
struct IOParams { std::string meshFilename, rgbdReadFilename, rgbdWriteFilename, trajReadFilename, trajWriteFilename; };
struct IcpParams { unsigned nPyramidLevels; float fNormSinThres, fDistThres, fDistShake, fAngleShake; };
struct SDFTrackerParams { unsigned maxIterNums; float fDistShake, fAngleShake; };
typedef kf_camera_params CameraParams;                       // {cols, rows, cx, cy, fx, fy}, 24 bytes
struct RayCasterParams { float fRayIncrement; };
struct DepthPrepocessParams { float fMaxTrunc, fMinTrunc, fSigmaDepth, fSigmaPixel; };
// fRecentreDist (not in the reference): the moving volume's policy.  0 (default): off, the cube stays where init put it.  > 0: after a tracked
// processNewFrame whose focus point lies farther than this (metres, any axis) from the volume's centre, the window is shifted towards it by whole bricks
// nStreamMeshTriangles (not in the reference): 0 (default): off.  > 0: HybKinectfu::init reserves a world soup of that many triangles and switches
// stream-out on (kf_set_stream_out with the mesh generator's colour switch and threshold): every shift first extracts the surface that is about to
// leave, and MeshGeneratorMarchingcube::generateMesh hands out [world soup, current window], all in world coordinates
// nBrickStoreBricks (not in the reference): 0 (default): off.  > 0: HybKinectfu::init reserves a brick store of that many bricks
// (kf_brick_store_reserve): every shift keeps the observed bricks that leave the window and restores the ones it finds when the window returns
// bMapMesh (not in the reference): false (default): off.  true, with a brick store reserved: MeshGeneratorMarchingcube::generateMesh builds the MAP mesh --
// kf_marching_cubes_map over store and window, world coordinates, no duplicates -- instead of [world soup, current window] (setMapMesh)
struct tsdfVolumeParams { unsigned nResolution; float fVolumeMeterSize, fWeightMax; float fRecentreDist; unsigned nStreamMeshTriangles; unsigned nBrickStoreBricks; bool bMapMesh; };
struct MarchingcubeParams { unsigned uMaxTriangles; };
struct IntegrateParams { float fSdfTruncation, fMaxIntegrateDist; };
struct SwitchParams { bool recordRGBD, recordTrajectory, useRGBData, colorAngleWeight, useDatasetRGBD, useTrajFromFile, useSdfTracker; };

class AppParams {
public:
  static AppParams* instance() { static AppParams v; return &v; }
  // values of src/config.ini with the VGA 525/319.5/239.5 camera; raycast increment = factor * trunc
  // (src/AppParamsProducer.cpp:113-117)
  void setDefaults(unsigned volume_resolution, float volume_size_meter);
  SwitchParams _switch_params;
  CameraParams _rgb_camera_params, _depth_camera_params;
  DepthPrepocessParams _depth_prepocess_params;
  IcpParams _icp_params;
  SDFTrackerParams _sdf_tracker_params;
  tsdfVolumeParams _volume_params;
  IntegrateParams _integrate_params;
  RayCasterParams _raycast_params;
  MarchingcubeParams _marchingcube_params;
  IOParams _io_params;
  // not in the reference: which GPU / z-slab this process owns (one process per GPU).  HybKinectfu passes slab_* to its one context but
  // raycasts the whole volume and merges nothing; for slabs whose model maps are merged use HybKinectfuSlabs (hybkf_slabs.hpp)
  int device = 0; unsigned slab_z_begin = 0, slab_z_end = 0, slab_halo = 0;
protected:
  AppParams() { setDefaults(256, 3.0f); }
};

// ---- src/cuda/Mat.h:196-440 ------------------------------------------------------------------------------------------
struct Mat44 {
  float entries[16];                                         // row-major; entries[3], [7], [11] = translation
  static Mat44 getIdentity();
  Mat44 getInverse() const;                                  // cofactor expansion, the reference's expression order
  Mat44 operator*(const Mat44& o) const;
  void setTranslation(float x, float y, float z) { entries[3] = x; entries[7] = y; entries[11] = z; }
};

// ---- src/FrameData.h:57-113: 16-bit millimetre depth (0 = invalid) / BGR 8-bit colour, as plain views ------------------
struct DepthFrameData {
  const uint16_t* mm = nullptr; int cols = 0, rows = 0; double time_stamp = 0; unsigned frame_id = 0;
  bool on_device = false;                                    // mm already lives in HBM (bench / streaming input)
  unsigned frameId() const { return frame_id; }
  double timeStamp() const { return time_stamp; }
};
struct ColorFrameData {
  const uint8_t* bgr = nullptr; int cols = 0, rows = 0; double time_stamp = 0; unsigned frame_id = 0;
};

// ---- src/cuda/CudaDeviceDataMan.h:15-78: owner of all device state, here a kf_ctx --------------------------------------
class CudaDeviceDataMan {
public:
  static CudaDeviceDataMan* instance() { static CudaDeviceDataMan v; return &v; }
  bool init();                                               // from AppParams, CudaDeviceDataMan.h:24-51
  void release();
  kf_ctx* ctx() const { return _ctx; }
  int lastError() const { return _err; }
  int check(int status) { if (status) _err = status; return status; }
private:
  kf_ctx* _ctx = nullptr; int _err = 0;
};

// ---- src/CameraPoseFinder.h:15-43 ---------------------------------------------------------------------------------------
class CameraPoseFinder {
public:
  CameraPoseFinder() : _inited(false) {}
  virtual ~CameraPoseFinder() {}
  virtual bool init(const Mat44& reference_transform);
  virtual bool findCameraPose(const DepthFrameData& depth_frame, const ColorFrameData& color_frame);
  Mat44 getCameraPose() const { return _pose; }
  void setCameraPose(const Mat44& transform);
  // the host's copy only, for a pose the device already holds (HybKinectfu::shiftVolume: kf_shift_volume moved the device-resident pose itself)
  void adoptCameraPose(const Mat44& transform) { _pose = transform; }
  // false (default): the Gauss-Newton loop runs on the device (kf_icp_track / kf_sdf_track), one read-back per frame;
  // true: the reference's own host loop -- one kernel wrapper + 27-float read-back + host 6x6 solve per iteration.
  void setHostLoop(bool on) { _host_loop = on; }
  // streaming use: enqueue tracking only; the verdict and pose stay on the device until syncPose()
  bool enqueueCameraPose(const DepthFrameData& depth_frame);
  bool syncPose();                                           // blocking read of (tracked, pose) into _pose
  // the same read-back split in two (kf_request_track_result / kf_wait_track_result): work enqueued between the two calls
  // overlaps with the host's wait.  deviceResident(): the verdict and the pose of this finder live on the device until read.
  bool requestPose();
  bool waitPose();
  // A tracker written against the reference's interface (src/CameraPoseFinder.h:38-39: TWO pure virtuals, initPoseFinder and
  // estimateCameraPose) computes its pose on the host: not device resident.  The built-in ICP / SDF finders override this.
  virtual bool deviceResident() const { return false; }
protected:
  Mat44 _pose;
  bool _host_loop = false;
  virtual bool initPoseFinder() = 0;
  virtual bool estimateCameraPose(const DepthFrameData& depth_frame, const ColorFrameData& color_frame) = 0;
  // NOT pure: the default estimates on the host and publishes the pose (+ "tracked") to the device, which is all a
  // two-virtual plugin can do; the built-in finders override it with their device-resident loops.
  virtual bool enqueueEstimate(const DepthFrameData& depth_frame);
private:
  bool _inited;
};

// ---- src/CameraPoseFinderICP.h / .cpp --------------------------------------------------------------------------------------
class CameraPoseFinderICP : public CameraPoseFinder {
public:
  bool deviceResident() const override { return !_host_loop; }
protected:
  bool initPoseFinder() override;
  bool estimateCameraPose(const DepthFrameData& depth_frame, const ColorFrameData& color_frame) override;
  bool enqueueEstimate(const DepthFrameData& depth_frame) override;
private:
  bool vector6ToTransformMatrix(const float x[6], Mat44& output);
  bool minimizePointToPlaneErrFunc(unsigned level, float six_dof[6], const Mat44& cur_transform, const Mat44& last_transform_inv);
  std::vector<int> _iter_nums;
  std::vector<CameraParams> _camera_params_pyramid;
};

// ---- src/CameraPoseFinderSDF.h / .cpp --------------------------------------------------------------------------------------
class CameraPoseFinderSDF : public CameraPoseFinder {
public:
  bool deviceResident() const override { return !_host_loop; }
protected:
  bool initPoseFinder() override;
  bool estimateCameraPose(const DepthFrameData& depth_frame, const ColorFrameData& color_frame) override;
  bool enqueueEstimate(const DepthFrameData& depth_frame) override;
  bool vector6ToTransformMatrix(const float x[6], Mat44& output);
};

// ---- src/CameraPoseFinderFromFile.{h,cpp}: poses from a TUM trajectory file (timestamp tx ty tz qx qy qz qw), the entry nearest in
// time to the depth frame, re-based so that frame 0 keeps the initial pose ---------------------------------------------------------------------
struct TimedRow { double stamp = 0; std::string text; float v[7] = {0, 0, 0, 0, 0, 0, 0}; };
// The reference walks its list files with getline / tellg / seekg; the same association rule on an in-memory table: rows are
// consumed in order, the first row at or after the target is compared with the row read just before it IN THE SAME QUERY, and
// when the earlier one is nearer the later row is pushed back for the next query (CameraPoseFinderFromFile.cpp:34-65,
// DataSourceProducerRGBDDataset.cpp:67-99).
class TimedTable {
public:
  bool load(const std::string& filename, int header_lines, bool numeric_fields);
  bool nearest(double target, TimedRow& out);                // false: ran off the end before reaching the target
  bool next(TimedRow& out);                                  // plain sequential read (depth list)
  size_t size() const { return _rows.size(); }
private:
  std::vector<TimedRow> _rows; size_t _cursor = 0;
};

class CameraPoseFinderFromFile : public CameraPoseFinder {
public:
  bool deviceResident() const override { return false; }     // poses are computed on the host
  static Mat44 transformFromQuaternion(const float t[3], const float q_xyzw[4]);   // Eigen's Quaternion -> Matrix3f, in fp32
protected:
  bool initPoseFinder() override;
  bool estimateCameraPose(const DepthFrameData& depth_frame, const ColorFrameData& color_frame) override;
  bool enqueueEstimate(const DepthFrameData& depth_frame) override;
private:
  TimedTable _trajectory;
  Mat44 _refer_transform;
};

// ---- the moving volume's host arithmetic (recentre.cpp; no reference counterpart, no device, C linkage: the CPU tests call them) -----------------
extern "C" {
// How far to shift for `pose` (row-major camera -> world in the window's coordinates): the focus point t + R (0, 0, size_m / 2) against the centre
// (size_m / 2 each way).  If any component of (focus - centre) exceeds `dist` in magnitude, out[i] = trunc((focus - centre)[i] / (8 cell)) * 8 voxels
// (truncation toward zero, cell = size_m / res), else zeros; dist <= 0 or a pose that is not finite gives zeros.  fp32, one rounding per operation.
void hkf_recentre_shift(const float pose[16], float size_m, uint32_t res, float dist, int32_t out[3]);
// The frame of the map a view from `world_pose` (camera -> world in the FIRST cube's coordinates, as hkf_world_pose gives them) looks into: frame[i] =
// trunc((focus - centre)[i] / (8 cell)) * 8 voxels with hkf_recentre_shift's focus t + R (0, 0, size_m / 2), truncation and +-1e6-brick clamp -- the window
// centred on the focus to within a brick -- and local_pose = world_pose with t - (float)frame * cell: the pose in that frame's coordinates.  A pose that
// is not finite gives frame 0 and the pose unchanged.  fp32, one rounding per operation.
void hkf_view_frame(const float world_pose[16], float size_m, uint32_t res, int32_t frame[3], float local_pose[16]);
// volume coordinates -> world coordinates: + (float)origin_vox * cell on the pose's translation / on n xyz positions.  A zero origin leaves every bit.
void hkf_world_pose(float pose[16], const int32_t origin_vox[3], float cell);
void hkf_world_positions(float* xyz, size_t n, const int32_t origin_vox[3], float cell);
// The cells that a shift by d voxels makes unextractable for good (their 27 voxels include one that leaves), as up to three disjoint half-open boxes
// lo[b] <= (x, y, z) < hi[b] in the order the stream-out emits them: the x strip in full, the y strip without it, the z strip without both.
// Returns the number of (non-empty) boxes written; 0 for a zero shift.
int hkf_departing_boxes(const int32_t d[3], uint32_t res, int32_t lo[3][3], int32_t hi[3][3]);
}

// ---- src/TrajectoryRecorder.{h,cpp}: TUM-format trajectory writer ---------------------------------------------------------------------------------
class TrajectoryRecorder {
public:
  explicit TrajectoryRecorder(const std::string& record_filename);
  virtual ~TrajectoryRecorder();
  bool recordCameraPose(const Mat44& mat, double timestamp);
  static void quaternionFromRotation(const Mat44& mat, float q_xyzw[4]);           // Eigen's Matrix3f -> Quaternion, in fp32
protected:
  FILE* _record_file;
};

// ---- src/DataSourceProducer.h, src/DataSourceProducerRGBDDataset.{h,cpp}: TUM RGB-D dataset reader ------------------------------------------------
class DataSourceProducer {
public:
  DataSourceProducer() : _capture_color(false), _inited(false) {}
  virtual ~DataSourceProducer() {}
  bool init();                                               // source directory and colour switch from AppParams
  bool readNewFrame(DepthFrameData& depth_data, ColorFrameData& rgb_data);
protected:
  virtual bool initDataSource() = 0;
  virtual bool readDataFromSource(DepthFrameData& depth_data, ColorFrameData& rgb_data) = 0;
  std::string _sourcefilename;
  bool _capture_color;
private:
  bool _inited;
};

class DataSourceProducerRGBDDataset : public DataSourceProducer {
public:
  DataSourceProducerRGBDDataset() : _depth_factor(5) {}
  // (cols+1)/2 x (rows+1)/2 Gaussian pyramid step of a 16-bit image, cv::pyrDown's integer arithmetic (5-tap 1 4 6 4 1 both
  // ways, reflect-101 border, (sum + 128) >> 8)
  static void pyrDown16(const uint16_t* src, int cols, int rows, std::vector<uint16_t>& dst);
protected:
  bool initDataSource() override;
  bool readDataFromSource(DepthFrameData& depth_data, ColorFrameData& rgb_data) override;
private:
  const float _depth_factor;                                 // TUM depth PNGs hold 1/5000 m; /5 -> millimetres
  TimedTable _depth_list, _rgb_list;
  std::vector<uint16_t> _depth_store;                        // the views handed out point into these until the next read
  std::vector<uint8_t> _bgr_store;
};

// ---- src/HybKinectfu.h / .cpp ------------------------------------------------------------------------------------------------
class HybKinectfu {
public:
  HybKinectfu();
  virtual ~HybKinectfu();
  bool init();
  bool processNewFrame(const DepthFrameData& depth_frame, const ColorFrameData& rgb_frame);
  // Streaming variant: enqueue the whole frame (upload, preprocess, track, integrate-if-tracked, raycast) with no host
  // synchronisation; the tracking verdict is applied on the device.  lastTracked()/getCameraPose() sync.
  bool enqueueFrame(const DepthFrameData& depth_frame, const ColorFrameData& rgb_frame);
  bool lastTracked();
  Mat44 getCameraPose();
  CameraPoseFinder* poseFinder() { return _camera_pose_finder; }
  // The pictures the reference paints on the host after every frame (DataViewer::viewNormal / viewColors, HybKinectfu.cpp:145-158), made on the
  // device (kf_render_view / kf_view_model_maps) and read back as cols * rows * 4 bytes (b, g, r, a); mode = KF_VIEW_*.  The increment and the
  // planes come from AppParams, as processNewFrame uses them.  renderView: any camera, from `pose` (nullptr: the current camera pose); it leaves
  // tracking state alone.  viewModelMaps: the tracking camera's view from the current model maps, no march.  Blocking (the read-back).
  bool renderView(const Mat44* pose, const kf_camera_params& cam, int mode, std::vector<uint8_t>& bgra);
  bool viewModelMaps(int mode, std::vector<uint8_t>& bgra);
  // The same picture of a window that stands elsewhere in the map (kf_render_view_at: the brick store's bricks where the window has moved on; nothing
  // moves, tracking state is left alone).  renderViewAt: the window at `frame` (voxels of the first cube, multiples of 8), `pose` in that frame's
  // coordinates (nullptr: the current camera pose, translated into the frame).  renderMapView: `world_pose` in the first cube's coordinates (what
  // worldPose returns); the frame is the one that centres the window on the view's focus (hkf_view_frame).  Single GPU, like the brick store.
  bool renderViewAt(int mode, const int frame[3], const Mat44* pose, const kf_camera_params& cam, std::vector<uint8_t>& bgra);
  bool renderMapView(int mode, const Mat44& world_pose, const kf_camera_params& cam, std::vector<uint8_t>& bgra);
  // The moving volume (no reference counterpart).  shiftVolume: kf_shift_volume by (dx, dy, dz) voxels, multiples of 8, then the raycast with the
  // moved pose and the stock parameters, so the model maps show the new window before the next frame is tracked.  A finder that keeps its pose on
  // the host gets the translated pose through setCameraPose -- the same fp32 expression as on the device.  false: not initialised, or the shift
  // was refused (a component that is no multiple of 8, a z-slab context).  volumeOrigin: the sum of all shifts, in voxels.
  // With AppParams::_volume_params.fRecentreDist > 0 processNewFrame recentres by itself after a tracked frame (hkf_recentre_shift on the pose it
  // has just waited for); enqueueFrame never does: it holds no host pose to decide on.  The recorded trajectory and saved meshes are in WORLD
  // coordinates (volume coordinates + origin * cell); with a zero origin they are what they always were, byte for byte.
  bool shiftVolume(int dx, int dy, int dz);
  void volumeOrigin(int out[3]);
  // Streaming the departing surface (AppParams::_volume_params.nStreamMeshTriangles; init calls this when it is > 0): reserves the world soup and
  // switches stream-out on; 0 frees the soup and switches it off.  worldSoupCount: the triangles the soup holds (blocking).
  bool setStreamMesh(unsigned max_triangles);
  unsigned worldSoupCount();
  // The brick store (AppParams::_volume_params.nBrickStoreBricks; init calls this when it is > 0): reserves a store of max_bricks bricks, so that a
  // window that returns finds what it left; 0 frees it.  brickStoreCounts: bricks held, dropped for want of room, restored (blocking).
  bool setBrickStore(unsigned max_bricks);
  bool brickStoreCounts(unsigned& held, uint64_t& dropped, uint64_t& restored);
  // The map on disk (map_file.hpp; needs the brick store).  saveMap: the window is captured into the store (kf_brick_store_capture: nothing moves, later
  // frames are what they are without the call), the store is read out in chunks and written with the current pose, origin and frameId().  false: no store,
  // a brick dropped during the capture (the file would have a hole nobody asked for), an I/O error.  Bricks dropped BEFORE the call are logged and
  // recorded in the header.  loadMap: reads and checks the whole file and refuses (false, nothing touched) one whose resolution, size, max weight or
  // colour differ from this instance's; then resets the volume, reserves the store at max(its capacity, the file's bricks), writes the bricks back
  // (kf_write_brick_store), places the window at the saved origin (kf_place_window), sets pose and frame id and raycasts as shiftVolume does, so
  // that the next processNewFrame is TRACKED against the loaded model.  A failure after the file was accepted (a read error, a device error) leaves an
  // empty volume and an empty store, never a half-loaded map.  frameId: the id of the last frame processed, or the one loadMap set.
  // The pose saved is the host's copy; with a device-resident finder it is read from the device, which also holds a pose that kf_place_window moved on the
  // raw context.  A finder that keeps its pose on the host does not see such a move: placing the window behind this class's back is not supported there.
  bool saveMap(const std::string& path);
  bool loadMap(const std::string& path);
  // loadMapCoarser: loadMap for a file recorded at 2^L times this instance's resolution, L in [1, 3], with the same size, max weight and colour flag: the
  // map is halved L times on the device (kf_merge_brick_store_halved: the mean tsdf of the observed children, their least weight, their mean colour).
  // L == 0 is loadMap; any other file is refused (false) with nothing touched.  The whole file is read into host memory; then the volume is reset and, level
  // by level, the store is reserved at max(its capacity, the level's coarse bricks: kf_halved_brick_keys), the finer map is merged halved into it and, for
  // the next level, read out again.  The window is placed at 8 * floor(origin_file / 2^L / 8) per axis (floor also for a negative origin).  The pose is the
  // file's with its translation moved into the new window's coordinates, in fp64 and rounded to fp32 once:
  //   t_k = (float)(((double)t_file_k + origin_file_k * (double)size / (double)resolution_file) - origin_new_k * (double)size / (double)resolution)
  // Frame id, the raycast and what a failure leaves are loadMap's.
  bool loadMapCoarser(const std::string& path);
  // mergeMap: fuses the map file into this session's map, voxel by voxel (kf_merge_brick_store: the weighted running average, exact in fp32, so merging
  // A into B and B into A give the same bricks).  offsetBricks (nullptr: zero) translates the file's keys by whole bricks into this session's world
  // frame; offsets that are no whole bricks go through the other mergeMap, and alignMap finds its transform.  The file is checked as loadMap checks it, and every
  // translated key must lie in the key range: refused (false) with nothing touched otherwise.  Then: the window is captured into the store (false when a
  // brick did not fit), the store is grown to held + the file's bricks where its capacity is below that (read out, reserved, written back: its dropped and
  // restored counts start again), the file's bricks are merged, the window is re-read from the store (kf_refill_window) and the model maps are raycast
  // as shiftVolume does, so the next processNewFrame is TRACKED against the merged model.  Pose and frame id stay this session's; the file's pose,
  // origin and frame id are ignored.  A store that was never reserved is reserved by the call, with room for every brick of the window.
  bool mergeMap(const std::string& path, const int offsetBricks[3]);
  // mergeMap under a rigid transform: srcToDst maps the file's world frame to this session's, in metres, as poses are (entries[3], [7], [11] the
  // translation).  The file's map is resampled at this session's voxel centres (kf_merge_brick_store_rigid: trilinear, the least weight of the corners),
  // then merged as above.  In voxels the translation is (double)t_m / (double)cell with cell the fp32 quotient size / resolution; the rotation is taken
  // as it stands.  The same checks and the same steps as the other mergeMap, but: the whole file is read into host memory, the candidate bricks
  // (kf_rigid_brick_keys) take the place of the file's bricks when the store is grown, and the merge is one call.  Refused (false) with nothing touched
  // also for a matrix that is no rigid transform (kf_rigid_brick_keys' rule) or that moves a brick out of the key range.  A file of another cell size is
  // refused like any other volume that is not this instance's.
  bool mergeMap(const std::string& path, const Mat44& srcToDst);
  // alignMap: finds the srcToDst that mergeMap(path, srcToDst) needs, refined from `guess` (both in metres, as poses are) by Gauss-Newton on the SDF-to-SDF
  // error between this session's map and the file's (kf_align_brick_store).  A refinement, not a search: the guess must lie within about the truncation
  // band of the answer (some 10 degrees and a few voxels on a box-like scene).  mergeMap's file and parameter checks, refused (false) with nothing touched;
  // then the window is captured into the store (a store that was never reserved is reserved; false when a brick did not fit), rotations are taken about
  // the middle of kf_brick_store_bounds' box, and one call runs at most 30 steps with at least 1000 pairs, down to the rule's resolution.  It merges
  // nothing: window, pose, model maps and frame id stay.  `found`: the transform of the last successful evaluation, in metres (the rotation rounded to
  // fp32); true only when the verdict is KF_ALIGN_CONVERGED.  report (may be nullptr): the call's report.
  bool alignMap(const std::string& path, const Mat44& guess, Mat44& found, kf_align_report* report);
  // eraseMapBox: clears the voxels of this session's map whose centres lie inside the box (keepInside: outside it -- the map cropped to the box); bricks
  // left with nothing observed leave the store and their slots are free again (kf_brick_store_erase_box).  The box is in WORLD metres, the first cube's
  // coordinates -- those of the map mesh's vertices and of worldPose --, half-open: voxel g is in it iff lo_m <= (g + 1/2) * cell < hi_m on every axis
  // (hkf_erase_box_voxels, erase_box_voxels.hpp; cell the fp32 quotient size / resolution).  A NaN corner is refused (false) with nothing touched.
  // eraseMapWeak: removes every brick whose greatest weight is below minWeight (kf_brick_store_erase_weak); the others stay bit for bit.
  // Both, in this order: a frame still in flight settles; the window is captured into the store (a store that was never reserved is reserved with room for
  // every brick of the window; false with nothing erased when a brick did not fit); the erase; the window is re-read from the store (kf_refill_window) and
  // the model maps are raycast as shiftVolume does, so the next processNewFrame is TRACKED against the erased model.  Pose and frame id stay.  Surface
  // already streamed into the world soup (setStreamMesh) is not taken back.  bricksRemoved / voxelsCleared (may be nullptr): the call's counts.
  bool eraseMapBox(const float lo_m[3], const float hi_m[3], bool keepInside, unsigned* bricksRemoved = nullptr, uint64_t* voxelsCleared = nullptr);
  bool eraseMapWeak(float minWeight, unsigned* bricksRemoved = nullptr);
  // relocalise: finds the camera again in this session's map from one depth frame (kf_map_score_poses, kf_map_refine_poses; reloc_search.hpp).  A frame in flight
  // settles; the frame is uploaded and preprocessed as processNewFrame does (and its vertex pyramid built), nothing is tracked or fused; the valid vertices of pyramid level params.level
  // (default: the coarsest), at most params.max_points (4096) of them, are the points.  The centre pose is params.guess (camera -> WORLD metres) or the current
  // pose; around it a lattice of 2 n + 1 candidates per axis (n = 2 on all six), translation steps of params.trans_step (default fSdfTruncation) along the
  // world's axes, rotation steps of params.rot_step (default atan(fSdfTruncation / median depth): one step moves the median point by one truncation, the
  // Gauss-Newton basin) about the camera's own centre.  All candidates are scored, the best params.top (16) refined about R * mean(points) + t, scored once
  // more, and the best of those is accepted when its n_in >= accept_inliers * points, its n_obs >= min_obs and its verdict is neither FEW_PAIRS nor SINGULAR.
  // On accept: with a store reserved and the pose's frame (hkf_view_frame) different from the window's origin the window is captured and placed there; the
  // pose is set, the model maps are raycast as loadMap does, and the next processNewFrame is TRACKED from there.  false -- refused, nothing eligible or not
  // accepted --: pose, window, store, volume and frame id are what they were; only the frame's preprocessing buffers have changed.  The search is a lattice
  // around a guess: its reach is the lattice's extent and nothing more.  report (may be nullptr): what was found, accepted or not.
  bool relocalise(const DepthFrameData& depth_frame, const RelocParams& params, RelocReport* report);
  // sampleMap: the map at n points in WORLD metres (world_m: 3 n doubles, the first cube's coordinates -- those of the map mesh's vertices and of worldPose),
  // read where it lies, window and store (kf_map_sample): the position in voxels is x / (double)cell (hkf_query_voxels, map_query_voxels.hpp; cell the
  // fp32 quotient size / resolution).  distance_m: tsdf * fSdfTruncation, the signed distance in metres inside the truncation band (+-fSdfTruncation beyond
  // it); weight: the least of the eight corners'; gradient (3 n): the distance's gradient, metres per metre, (grad * fSdfTruncation) / cell -- it points out of
  // the surface; color (4 n bytes).  A point one of whose eight corners was never observed gives zeros.  Any output may be nullptr.
  // castMapRays: the first surface crossing of n rays (kf_map_cast_rays): origins in world metres, dir (3 n) used as given (unit vectors: t is metres), t_min_m /
  // t_max_m per ray in metres (divided by cell in fp32), the step fRayIncrement / cell; status (KF_RAY_MISS / _HIT / _BROKEN), t_m = t * cell, the unit normal,
  // colour and weight of the hit; zeros where there is none.  Any output may be nullptr.
  // Both only read: nothing of the session changes, no frame is waited for beyond the stream's order.  false: not initialised, a null input, the call failed.
  bool sampleMap(const double* world_m, size_t n, float* distance_m, float* weight, float* gradient, uint8_t* color);
  bool castMapRays(const double* origin_m, const float* dir, const float* t_min_m, const float* t_max_m, size_t n, uint8_t* status, float* t_m, float* normal, uint8_t* color,
                   float* weight);
  // distanceFieldVoxels: the map's distance field over the box lo_vox / dims of world voxels (kf_map_distance_field: the squared distance in voxels to the
  // nearest site within `radius` voxels, KF_EDT_FAR beyond; the class bytes), indexed (z * ny + y) * nx + x.  A box with an edge above 128 voxels is computed
  // in tiles of at most 128 per axis (hkf_edt_tile, edt_box_voxels.hpp) and stitched: the same bytes, by the field's sub-box guarantee, and no box is too
  // large for the call's cap.  dist2 / cls: nx * ny * nz items each, either may be nullptr.
  // distanceField: the same in WORLD metres.  The box is eraseMapBox's (voxel g is in it iff lo_m <= (g + 1/2) * cell < hi_m); the radius is
  // floor(maxDist_m / cell) clamped to 1 .. 255 and reported back in radiusVox; distance_m = sqrtf((float)d2) * cell, +infinity where no site lies within the
  // radius.  distance_m and cls are resized to nx * ny * nz, dims receives the box's size in voxels, loVox (may be nullptr) its first voxel.
  // Both only read: they capture nothing and move nothing.  false: not initialised, a null or empty box, a box of more than 2^31 voxels (hkf_edt_voxel_count:
  // refused before anything is sized), no memory for the arrays, a refused call.
  bool distanceFieldVoxels(const int32_t lo_vox[3], const uint32_t dims[3], uint32_t radius, float level, uint32_t siteMask, uint16_t* dist2, uint8_t* cls);
  bool distanceField(const float lo_m[3], const float hi_m[3], float maxDist_m, float level, uint32_t siteMask, std::vector<float>& distance_m, std::vector<uint8_t>& cls,
                     uint32_t dims[3], uint32_t* radiusVox, int32_t* loVox = nullptr);
  unsigned frameId() const { return _frame_id; }
private:
  bool recentre();
  // the steps both mergeMaps share.  mergeMakeRoom: a store reserved if there was none, the window captured, the store grown to held + `incoming` bricks;
  // mergeShow: the window re-read from the store, the model maps raycast from this session's pose
  bool mergeMakeRoom(bool color, uint64_t incoming);
  bool mergeShow();
  Mat44 worldPose(const Mat44& pose);
  void copyFrameToGPU(const DepthFrameData& depth_frame, const ColorFrameData& color_frame);
  CameraPoseFinder* _camera_pose_finder;
  TrajectoryRecorder* _camera_pose_recorder = nullptr;       // switch recordTrajectory (HybKinectfu.cpp:47-50,129-132)
  bool _inited;
  bool _last_tracked = true;      // verdict of the last processNewFrame
  bool _pending = false;          // frames enqueued whose verdict still lives on the device
  unsigned _frame_id = 0;         // frameId() of the last frame handed to processNewFrame / enqueueFrame (saveMap records it, loadMap sets it)
};

// ---- src/MeshGenerator.h, src/MeshGeneratorMarchingcube.{h,cpp}, src/utils/mesh/meshData.* (the parts saveMesh uses) ----------
struct MeshData {
  std::vector<float> vertices;                               // xyz
  std::vector<float> colors;                                 // rgba, empty when the volume has no colour
  std::vector<float> normals;                                // xyz
  std::vector<unsigned> faces;                               // 3 indices per face
  unsigned mergeCloseVertices(float thresh);                 // meshData.cpp:198-283, approx = true path (hash grid, first come wins); ends with removeDegeneratedFaces
  unsigned removeDegeneratedFaces();                         // meshData.cpp:289-310: faces with a repeated index are dropped
  unsigned removeDuplicateFaces();                           // meshData.cpp:42-82
  void computeVertexNormals();                               // meshData.h:713-736
  bool saveToFile(const std::string& filename) const;        // by extension: .obj / .ply / .off (MeshIO.cpp:492-662)
};

class MeshGenerator {
public:
  virtual ~MeshGenerator() {}
  virtual void generateMesh() = 0;
  virtual bool saveMesh(const std::string& filename) = 0;
};

class MeshGeneratorMarchingcube : public MeshGenerator {
public:
  void generateMesh() override;
  bool saveMesh(const std::string& filename) override;
  unsigned triangleCount();
  const MeshData& mesh() const { return _meshes; }
  MeshData& mesh() { return _meshes; }
  // the two halves of copyTrianglesToCPU + saveMesh that need no device: usable on any triangle soup (CPU tests pin them
  // against the reference's own ml::MeshData, tests/golden/mesh_*.npz)
  void setTriangles(const kf_triangle* tris, unsigned n, bool with_color);   // :39-58
  void weldMesh();                                                           // :69-84 index buffer, weld, dedupe, normals
  // saveMesh welds on the device (kf_weld_mesh: the same mesh, bit for bit) and reads the indexed mesh back instead of the soup.
  // Off by default; if the device weld fails, saveMesh welds on the host as before.
  void setDeviceWeld(bool on) { _device_weld = on; }
  bool deviceWeld() const { return _device_weld; }
  // saveMesh drops, after the weld, every connected part of the mesh with fewer than n faces -- with largest_only all but the largest (the rule:
  // include/hybkf.h, kf_mesh_drop_parts).  On the device (kf_mesh_drop_parts, before the read-back) under setDeviceWeld(true), on the host
  // (mesh_parts.hpp) otherwise: the same file either way.  The default (0, false) is off: saveMesh writes the bytes it always wrote.
  void setMinPartFaces(unsigned n, bool largest_only = false) { _min_part_faces = n; _largest_only = largest_only; }
  bool dropsParts() const { return _min_part_faces > 0 || _largest_only; }
  void dropMeshParts();                                                      // the host side of it, on the mesh as it stands (nothing when off)
  // AppParams::_volume_params.bMapMesh: with a brick store reserved, generateMesh clears the triangle buffer and meshes the whole map (kf_marching_cubes_map)
  void setMapMesh(bool on);
protected:
  bool copyTrianglesToCPU();
  bool weldOnDevice();                                                       // :61-86 without the 72 bytes per triangle crossing to the host
  MeshData _meshes;
  bool _device_weld = false;
  unsigned _min_part_faces = 0;
  bool _largest_only = false;
  bool _world = false;            // the triangles of the last generateMesh are in world coordinates already (streaming on, or the map mesh): saveMesh adds no origin
};
