// hybkf_slabs.hpp -- HybKinectfuSlabs: the reference's HybKinectfu surface (src/HybKinectfu.h) over a slab group (include/hybkf_group.h),
// for C++ callers that want more than one GPU -- or the z-slab protocol on one GPU.  It reads the same AppParams as HybKinectfu (camera,
// volume, ICP, depth preprocess, integrate, raycast) plus a SlabLayout.  HybKinectfu itself stays the one-context class and ignores
// AppParams::slab_*.  It honours _switch_params.useRGBData / colorAngleWeight as HybKinectfu does: a colour group (kf_group_create_color), every frame's
// ColorFrameData::bgr handed to the members, coloured triangles and a coloured mesh; with useRGBData set a frame without a BGR image is refused.  Built as libhybkf_slabs.so, above libhybkf_host.so, libhybkf_group.so and libhybkf.so.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>
#include "hybkf_host.hpp"
#include "../../include/hybkf_group.h"

struct SlabLayout {
  int backend = KF_GROUP_LOCAL;                  // KF_GROUP_LOCAL / KF_GROUP_RCCL_ALL / KF_GROUP_RCCL_RANK
  std::vector<unsigned> cuts;                    // members + 1 brick-aligned z cuts, 0 .. resolution (RCCL_RANK: {z0, z1}, this rank's own slab)
  std::vector<int> devices;                      // one per member; empty: AppParams::device for all
  unsigned halo = 0;                             // 0: the thinnest the raycast accepts (pipeline.slab_halo_layers)
  std::vector<uint8_t> unique_id;                // RCCL_RANK: kf_group_unique_id of rank 0, handed to every rank
  unsigned rank = 0, world = 1;                  // RCCL_RANK
  // equal slabs over `members` members (sizes differing by at most one brick layer), pipeline.slab_ranges without a work probe
  static std::vector<unsigned> evenCuts(unsigned resolution, unsigned members);
};

class HybKinectfuSlabs {
public:
  HybKinectfuSlabs() {}
  ~HybKinectfuSlabs();
  HybKinectfuSlabs(const HybKinectfuSlabs&) = delete;             // owns its group: one owner, one kf_group_destroy
  HybKinectfuSlabs& operator=(const HybKinectfuSlabs&) = delete;
  bool init(const SlabLayout& layout);
  // one frame through every member and the merge; blocks for the tracking verdict, like HybKinectfu::processNewFrame
  bool processNewFrame(const DepthFrameData& depth_frame, const ColorFrameData& rgb_frame);
  // streaming: no host synchronisation; lastTracked() / getCameraPose() read the verdict
  bool enqueueFrame(const DepthFrameData& depth_frame, const ColorFrameData& rgb_frame);
  bool lastTracked();
  Mat44 getCameraPose();
  // marching cubes on every member; saveMesh welds the slab-major triangles (= the whole volume's order) and writes .ply / .obj / .off
  void generateMesh();
  bool saveMesh(const std::string& filename);
  unsigned triangleCount();
  // MeshGeneratorMarchingcube::setMinPartFaces: saveMesh drops the mesh's small parts after its (host) weld; (0, false) is off
  void setMinPartFaces(unsigned n, bool largest_only = false) { _mesh.setMinPartFaces(n, largest_only); }
  const MeshData& mesh() const { return _mesh.mesh(); }
  // HybKinectfu::viewModelMaps through member 0: after a frame's merge every member holds the whole volume's model maps.  cols * rows * 4 bytes
  // (b, g, r, a); mode = KF_VIEW_*, KF_VIEW_COLOR on a colour group only.  Blocking.
  bool viewModelMaps(int mode, std::vector<uint8_t>& bgra);
  // HybKinectfu::renderView over the group (kf_group_render_view: every member marches the view's rays through its own layers, the merge gives the
  // whole volume's picture): any camera, from `pose` (nullptr: the current camera pose, device-resident on every member); the increment and the
  // planes come from AppParams, as processNewFrame uses them; it leaves tracking state alone.  Blocking (the read-back).
  bool renderView(const Mat44* pose, const kf_camera_params& cam, int mode, std::vector<uint8_t>& bgra);
  // The moving volume, with HybKinectfu's semantics (hybkf_host.hpp).  shiftVolume: kf_group_shift_volume by (dx, dy, dz) voxels, multiples of 8 -- brick
  // layers travel between the members for a z shift --, then the merged raycast (kf_group_raycast), so every member's model maps show the new window
  // before the next frame is tracked.  false: not initialised, or the shift was refused.  volumeOrigin: the sum of all shifts, in voxels.
  // With AppParams::_volume_params.fRecentreDist > 0 processNewFrame recentres by itself after a tracked frame (hkf_recentre_shift on the pose it has
  // just waited for); enqueueFrame never does: it holds no host pose to decide on.  getCameraPose stays in the window's coordinates; the recorded
  // trajectory (switch recordTrajectory, AppParams::_io_params.trajWriteFilename) and saved meshes are in WORLD coordinates (hkf_world_pose /
  // hkf_world_positions); with a zero origin every byte is what it always was.  A group's window forgets what leaves it: brick store, stream-out
  // and map mesh (nBrickStoreBricks, nStreamMeshTriangles, bMapMesh) are HybKinectfu's alone.
  bool shiftVolume(int dx, int dy, int dz);
  void volumeOrigin(int out[3]);
  // HybKinectfu's map on disk is built on the brick store, a single-GPU feature: a slab group has no store to save from or load into.  Always false.
  bool saveMap(const std::string&) { return false; }
  bool loadMap(const std::string&) { return false; }
  bool loadMapCoarser(const std::string&) { return false; }
  bool mergeMap(const std::string&, const int*) { return false; }
  bool mergeMap(const std::string&, const Mat44&) { return false; }
  bool alignMap(const std::string&, const Mat44&, Mat44&, kf_align_report*) { return false; }
  bool eraseMapBox(const float*, const float*, bool, unsigned* = nullptr, uint64_t* = nullptr) { return false; }
  bool eraseMapWeak(float, unsigned* = nullptr) { return false; }
  bool relocalise(const DepthFrameData&, const RelocParams&, RelocReport*) { return false; }     // always refused: no store, part of a window each
  bool sampleMap(const double*, size_t, float*, float*, float*, uint8_t*) { return false; }
  bool castMapRays(const double*, const float*, const float*, const float*, size_t, uint8_t*, float*, float*, uint8_t*, float*) { return false; }
  bool distanceFieldVoxels(const int32_t*, const uint32_t*, uint32_t, float, uint32_t, uint16_t*, uint8_t*) { return false; }
  bool distanceField(const float*, const float*, float, float, uint32_t, std::vector<float>&, std::vector<uint8_t>&, uint32_t*, uint32_t*, int32_t* = nullptr) { return false; }
  kf_group* group() const { return _group; }
  int lastError() const { return _err; }
private:
  struct SlabMesh : MeshGeneratorMarchingcube { MeshData& data() { return _meshes; } };
  bool check(int status) { if (status) _err = status; return status == 0; }
  bool syncVerdict();
  bool recentre();
  kf_group* _group = nullptr;
  SlabMesh _mesh;
  TrajectoryRecorder* _recorder = nullptr;                   // switch recordTrajectory, as in HybKinectfu
  Mat44 _pose = Mat44::getIdentity();
  bool _inited = false, _last_tracked = true, _pending = false, _color = false;
  int _err = 0;
};
