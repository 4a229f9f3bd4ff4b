/*
 * hybkf.h -- C ABI of the MI355X-native KinectFusion core (libhybkf.so).
 *
 * This is the drop-in boundary for the reference's per-frame path: every entry point replaces one of
 * the reference's `extern "C" void cuda*()` launch wrappers (src/cuda/CudaWrappers.h:22-36) or one of the
 * direct accesses its host classes make to the CudaDeviceDataMan singleton (src/cuda/CudaDeviceDataMan.h:54-67).
 * Differences from the reference boundary, all deliberate:
 *   - state lives in an explicit, opaque `kf_ctx` (one per GPU / z-slab) instead of a process singleton;
 *   - every call returns an int status (0 = ok) instead of void, and never throws;
 *   - calls are asynchronous on the context's HIP stream; only the kf_read_ and kf_download_ calls and kf_synchronize block;
 *   - the Gauss-Newton loops of CameraPoseFinderICP/SDF can run entirely on the device (kf_icp_track /
 *     kf_sdf_track) so the 19 host round trips per frame of the reference (src/CameraPoseFinderICP.cpp:117)
 *     disappear; the per-iteration wrappers are still exported for drop-in use and for parity tests.
 * Plain pointers and sizes only; no C++ or torch types.  Paths cited are relative to /root/reference.
 */
#ifndef HYBKF_H_
#define HYBKF_H_
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kf_ctx kf_ctx;

/* src/AppParams.h:36-43 (24 bytes) */
typedef struct kf_camera_params { uint32_t cols, rows; float cx, cy, fx, fy; } kf_camera_params;
/* src/cuda/Mat.h:196-206: row-major 4x4, m[3], m[7], m[11] = translation, camera -> world */
typedef struct kf_mat44 { float m[16]; } kf_mat44;
/* src/AppParams.h:86-90 */
typedef struct kf_integrate_params { float sdf_truncation; float max_integrate_dist; } kf_integrate_params;
/* src/AppParams.h:59-62 */
typedef struct kf_raycast_params { float ray_increment; } kf_raycast_params;
/* src/AppParams.h:70-75 */
typedef struct kf_volume_params { uint32_t resolution; float size_m; float max_weight; } kf_volume_params;
/* src/AppParams.h:22-30 */
typedef struct kf_icp_params { uint32_t pyramid_levels; float norm_sin_thres, dist_thres, dist_shake, angle_shake; } kf_icp_params;
/* src/AppParams.h:31-35 */
typedef struct kf_sdf_tracker_params { uint32_t max_iter_nums; float dist_shake, angle_shake; } kf_sdf_tracker_params;
/* src/cuda/MarchingcubeData.h:15-27 (24 / 72 bytes) */
typedef struct kf_vertex { float pos[3]; float color[3]; } kf_vertex;
typedef struct kf_triangle { kf_vertex v0, v1, v2; } kf_triangle;

/* What CudaDeviceDataMan::init() reads from AppParams (src/cuda/CudaDeviceDataMan.h:24-51), plus the z-slab. */
typedef struct kf_config {
  kf_camera_params depth_camera;
  kf_camera_params rgb_camera;
  kf_volume_params volume;        /* resolution must be a multiple of 8 */
  uint32_t pyramid_levels;        /* 1..3 */
  uint32_t max_triangles;
  int32_t  has_color;             /* allocate the colour plane + rgb maps */
  int32_t  device;                /* HIP device ordinal */
  uint32_t slab_z_begin;          /* z range of voxel layers this context OWNS; 0 / resolution for one GPU */
  uint32_t slab_z_end;
  uint32_t slab_halo;             /* extra layers stored (and integrated) on each side, clipped to the volume */
} kf_config;

/* map ids for kf_download_map / kf_upload_map (members of CudaDeviceDataMan.h:56-67) */
enum {
  KF_MAP_RAW_DEPTH = 0, KF_MAP_TRUNCED_DEPTH = 1, KF_MAP_FILTERED_DEPTH = 2,   /* float,  cols*rows    */
  KF_MAP_NEW_VERTICES = 3, KF_MAP_NEW_NORMALS = 4,                             /* float4, per level    */
  KF_MAP_MODEL_VERTICES = 5, KF_MAP_MODEL_NORMALS = 6,                         /* float4, per level    */
  KF_MAP_RAW_RGB = 7, KF_MAP_RAYCAST_RGB = 8                                   /* uchar3, cols*rows    */
};

/* status of the device-side tracker after kf_icp_track / kf_sdf_track */
enum { KF_TRACK_OK = 0, KF_TRACK_LOST_DET = 1, KF_TRACK_LOST_SHAKE = 2,
       KF_TRACK_STALLED = 3 /* (no longer produced: a device-side wait that times out is finished by one workgroup alone, see kf_track_result::launch_form) */ };

typedef struct kf_track_result {
  kf_mat44 pose;            /* CameraPoseFinder::_pose after the call (unchanged when lost) */
  int32_t  tracked;         /* bool returned by findCameraPose */
  int32_t  status;          /* KF_TRACK_* */
  int32_t  iterations;      /* Gauss-Newton iterations actually applied */
  int32_t  launch_form;     /* how the last kf_icp_track / kf_sdf_track call was launched: 0 none (frame 0), 1 persistent device loop, 2 one launch per
                             * Gauss-Newton step / iteration (GPU shared, a second context, after a stall), 3 persistent loop that timed
                             * out waiting for a workgroup that was not resident and was finished by one workgroup alone (the frame is kept,
                             * milliseconds late).  ICP: the same pose bits in every form.  SDF: forms 1 and 3 give the same bits, form 2
                             * agrees with them to tolerance only (it deals pixels and maps the increment differently) */
} kf_track_result;

typedef struct kf_volume_stats {
  uint64_t updated_last;    /* N_upd: voxels that passed the update predicate in the last integrate */
  uint64_t weight_gt0;      /* voxels with weight > 0 (owned slab only) */
  uint64_t bricks_active;   /* 8^3 bricks queued for the last integrate's fusion pass (after max_weight fused frames, bricks of saturated free
                             * space that is seen as free space again are counted into updated_last without being queued) */
  uint64_t bricks_total;
  uint64_t updated_total;   /* running sum of updated_last since kf_reset_volume */
  uint64_t frames_fused;    /* integrate calls that ran */
  uint64_t frames_lost;     /* integrate calls skipped because the device-side tracker reported lost */
} kf_volume_stats;

const char* kf_error_string(int status);
const char* kf_version(void);

/* CudaDeviceDataMan::init  src/cuda/CudaDeviceDataMan.h:24-51 */
int kf_create(const kf_config* cfg, kf_ctx** out);
int kf_destroy(kf_ctx* ctx);
int kf_synchronize(kf_ctx* ctx);
void* kf_stream(kf_ctx* ctx);                        /* hipStream_t of the context */
/* enqueue on a caller-owned hipStream_t.  NULL means "back to the private stream", NOT the null stream: a framework whose
 * default stream has the null handle (PyTorch) must create a stream of its own and make it current around its own work */
int kf_set_stream(kf_ctx* ctx, void* hip_stream);
int kf_reset_volume(kf_ctx* ctx);                    /* tsdfvolume::init clearData  src/cuda/tsdfVolume.h:29-37 */

/* HybKinectfu::copyFrameToGPU  src/HybKinectfu.cpp:63-96 : u16 mm -> f32 m ((float)((double)mm*0.001)) into raw_depth */
int kf_upload_depth_mm(kf_ctx* ctx, const uint16_t* host_mm, uint32_t cols, uint32_t rows);
/* the same copy AHEAD of its use (src/HybKinectfu.cpp:63-96 run early): the frame goes into a free upload slot and does not replace the current one;
 * up to two frames may be staged (a third: KF_ERR_STATE), kf_take_next_depth makes the oldest of them the current frame (KF_ERR_STATE if none);
 * kf_upload_depth_mm drops whatever is staged.  *dev_mm (may be NULL) = where the frame lies on the device, for kf_prefetch_frame: its front end
 * then rides in its predecessor's launches.  Staging TWO ahead -- upload frame k+2 while frame k is processed and frame k+1 rides along -- takes
 * the PCIe copy off the critical path: a host-fed stream then runs at the rate of one that is already in HBM (bench.py value_pcie_inclusive). */
int kf_upload_depth_mm_next(kf_ctx* ctx, const uint16_t* host_mm, uint32_t cols, uint32_t rows, const uint16_t** dev_mm);
int kf_take_next_depth(kf_ctx* ctx);
int kf_set_depth_mm_device(kf_ctx* ctx, const uint16_t* dev_mm, uint32_t cols, uint32_t rows);   /* frame already in HBM */
int kf_upload_rgb(kf_ctx* ctx, const uint8_t* host_bgr, uint32_t cols, uint32_t rows);
/* the counterpart of kf_set_depth_mm_device for colour: a BGR frame (3 bytes per pixel, rgb_camera's size) already in HBM.  It is widened into the
 * context's raw rgb map where the stream stands; the caller keeps dev_bgr unchanged until then (stream order, or kf_synchronize) */
int kf_set_rgb_device(kf_ctx* ctx, const uint8_t* dev_bgr, uint32_t cols, uint32_t rows);

/* cudaTruncDepth  src/cuda/DataPreprocesser.cu:80-88 */
int kf_trunc_depth(kf_ctx* ctx, float trunc_min, float trunc_max);
/* cudaBiliearFilterDepth  src/cuda/DataPreprocesser.cu:89-100 */
int kf_bilateral_filter_depth(kf_ctx* ctx, float sigma_pixel, float sigma_depth);
/* cudaCalculateNewVertices / cudaCalculateNewNormals  src/cuda/VerticesNormalsCalculater.cu:67-85 */
int kf_calculate_new_vertices(kf_ctx* ctx, const kf_camera_params* depth_camera);
int kf_calculate_new_normals(kf_ctx* ctx);
/* the four above fused (what HybKinectfu::processNewFrame runs, src/HybKinectfu.cpp:106-110) */
int kf_preprocess(kf_ctx* ctx, float trunc_min, float trunc_max, float sigma_pixel, float sigma_depth,
                  const kf_camera_params* depth_camera);
/* No reference counterpart (the reference synchronises after every launch): have kf_preprocess's work for the NEXT frame -- a device
 * u16 millimetre image, as for kf_set_depth_mm_device -- done ahead of time into a second buffer set.  Default form: the call only
 * leaves a note.  Called BEFORE kf_icp_track, the next frame's conversion + gate + bilateral filter ride in the tracking launch as extra
 * workgroups on the CUs the persistent loop leaves idle, and its integrate tile tables and vertices / normals as extra workgroups of the
 * next kf_raycast_volume(_slab) launch; when the tracker took another launch form (or the call came after it) the whole filter rides in
 * the raycast launch and the vertices / normals launch follows it -- same stream, no events either way.  KF_PREFETCH_FUSED=0 selects
 * the older form: the two preprocess launches on a side stream, concurrent with whatever is enqueued next.  Either way the next
 * kf_set_depth_mm_device(same pointer) + kf_preprocess(same parameters) adopts the result; any other sequence ignores it.
 * Results are bit-identical to the unprefetched path. */
int kf_prefetch_frame(kf_ctx* ctx, const uint16_t* dev_depth_mm, uint32_t cols, uint32_t rows, float trunc_min, float trunc_max,
                      float sigma_pixel, float sigma_depth, const kf_camera_params* depth_camera);

/* cudaDownSample{New,Model}{Vertices,Normals}  src/cuda/sample.cu:63-112 */
int kf_downsample_new_vertices(kf_ctx* ctx);
int kf_downsample_new_normals(kf_ctx* ctx);
int kf_downsample_model_vertices(kf_ctx* ctx);
int kf_downsample_model_normals(kf_ctx* ctx);

/* cudaCalPointToPlaneErrSolverParams  src/cuda/CalPointToPlaneErrSolverParams.cu:110-129 -> rigid_align_buf_reduced */
int kf_cal_point_to_plane_solver_params(kf_ctx* ctx, uint32_t pyramid_level, const kf_mat44* cur_transform,
                                        const kf_mat44* last_transform_inv, const kf_camera_params* cam,
                                        float dist_thres, float norm_sin_thres);
/* cudaCalSDFSolverParams  src/cuda/CalSDFErrSolverParams.cu:110-138 */
int kf_cal_sdf_solver_params(kf_ctx* ctx, const kf_camera_params* cam, const kf_mat44* cur_transform);
/* rigid_align_buf_reduced.clone(CPU)  src/CameraPoseFinderICP.cpp:117 : blocking 27-float read-back */
int kf_read_solver_params(kf_ctx* ctx, float out27[27]);

/* Device-resident pose + whole Gauss-Newton loops.
 * kf_set_pose: CameraPoseFinder::init / setCameraPose (src/CameraPoseFinder.h:22-36).
 * kf_icp_track: CameraPoseFinderICP::estimateCameraPose (src/CameraPoseFinderICP.cpp:50-94) incl. the four pyramid builds.
 * kf_sdf_track: CameraPoseFinderSDF::estimateCameraPose (src/CameraPoseFinderSDF.cpp:44-106).
 * frame_id == 0 returns "tracked" without touching the pose, as the reference does.  Asynchronous. */
int kf_set_pose(kf_ctx* ctx, const kf_mat44* pose);
int kf_icp_track(kf_ctx* ctx, uint32_t frame_id, const kf_icp_params* icp, const kf_camera_params* depth_camera);
int kf_sdf_track(kf_ctx* ctx, uint32_t frame_id, const kf_sdf_tracker_params* sdf, const kf_camera_params* depth_camera);
int kf_read_track_result(kf_ctx* ctx, kf_track_result* out);          /* blocking */
/* the same read-back in two halves: `request` enqueues the copy where the stream stands, `wait` blocks until that copy has
 * arrived -- work enqueued in between (integrate and raycast with transform == NULL) keeps the GPU busy meanwhile */
int kf_request_track_result(kf_ctx* ctx);
int kf_wait_track_result(kf_ctx* ctx, kf_track_result* out);
/* Fault injection (tests, rehearsals; no reference counterpart): each of the next `launches` launches of the persistent ICP loop gets one
 * workgroup that exits at once, as if a foreign process had kept it off the chip.  The others time out after 20 ms and one of them finishes
 * the frame's Gauss-Newton loop alone: same pose bits, launch_form 3, no frame lost. */
int kf_inject_track_stall(kf_ctx* ctx, int launches);
/* diagnostics: culls that ran as the tail of a tracking launch and were consumed by kf_integrate_volume / were undone (see kf_integrate_volume) */
int kf_cull_tail_counts(kf_ctx* ctx, uint32_t* consumed, uint32_t* undone);
/* diagnostics: which instantiation of the fusion pass and which cull the last kf_integrate_volume launched (host-side bookkeeping at the dispatch,
 * no device work).  The environment switches (KF_INTEGRATE_*, KF_CULL_*, KF_OBSERVED_COUNT), the volume's size and the context's state pick the form;
 * every form gives the same bits, and the tests check each against the CPU oracle with this read-back telling them which one ran. */
enum { KF_FUSE_NONE = 0, KF_FUSE_PAIRS = 1 /* k_integrate_pairs<bricks, defer, color, layers, count> */, KF_FUSE_PIPE = 2 /* k_integrate_pairs_pipe<defer, count> */,
       KF_FUSE_BRICKS = 3 /* k_integrate_bricks<color, bricks> */ };
enum { KF_CULL_NONE = 0, KF_CULL_TAIL = 1 /* run by the tracking launch's tail, consumed */, KF_CULL_MACRO = 2 /* k_integrate_cull<defer> */,
       KF_CULL_SIFT = 3 /* k_integrate_cull_sift<defer> */ };
typedef struct kf_fusion_form {
  int32_t  kernel;          /* KF_FUSE_* (KF_FUSE_NONE before the first call, and for the timing experiments of the KF_EXPERIMENTS build) */
  int32_t  bricks;          /* bricks in flight per workgroup (BR) */
  int32_t  defer, color, layers, count;   /* 0 / 1: the instantiation's template switches */
  int32_t  cull;            /* KF_CULL_* */
  int32_t  cull_defer;      /* 0 / 1: the cull's template switch (0 for the tail) */
  uint32_t grid;            /* workgroups of the fusion launch */
  uint32_t calls;           /* kf_integrate_volume calls that launched a fusion pass since kf_create */
} kf_fusion_form;
int kf_get_fusion_form(kf_ctx* ctx, kf_fusion_form* out);
/* diagnostics: which form the last raycast launch (kf_raycast_volume and its z-slab variants) took -- host-side bookkeeping at the dispatch, no device
 * work.  The environment switches (KF_RAYCAST_*), the volume's size and a pending kf_prefetch_frame pick the form; every form gives the same bits.
 * Test-only switches besides those of DESIGN.md: KF_RAYCAST_BOUNDS=2 takes the super / macro list path of the tile bounds at any volume size,
 * KF_RAYCAST_NEG_LDS=0 keeps the per-brick bits out of LDS (the march reads brick flags from global memory, as from ~570^3 up). */
enum { KF_RC_NONE = 0, KF_RC_PLAIN = 1 /* k_raycast */, KF_RC_FILTER = 2 /* k_raycast_prefetch<fast>, the next frame's filter riding */,
       KF_RC_BEHIND = 3 /* k_raycast_prefetch<fast>, riders behind a filter that ran in the tracking launch */ };
enum { KF_RC_BOUNDS_NONE = 0, KF_RC_BOUNDS_MESO = 1 /* direct scan of the meso table */, KF_RC_BOUNDS_MACRO = 2 /* direct scan of the macro table */,
       KF_RC_BOUNDS_LIST = 3 /* super cells listed, then their macro cells */ };
enum { KF_RC_OUT_MAPS = 0 /* the model maps */, KF_RC_OUT_T = 1 /* kf_raycast_volume_slab */, KF_RC_OUT_TA = 2 /* kf_raycast_volume_slab_cross */,
       KF_RC_OUT_TA_SPEC = 3 /* kf_raycast_volume_slab_cross_spec */ };
typedef struct kf_raycast_form {
  int32_t  kernel;          /* KF_RC_* */
  int32_t  fast;            /* k_raycast_prefetch's template switch (the riders' sentinel form of the bilateral filter); 0 for k_raycast */
  int32_t  output;          /* KF_RC_OUT_* */
  int32_t  tile_bounds;     /* 0 / 1: rc_tile_bounds runs */
  int32_t  bounds_path;     /* KF_RC_BOUNDS_* (KF_RC_BOUNDS_NONE without tile bounds) */
  int32_t  meso_lds;        /* 0 / 1: the meso table is in LDS */
  int32_t  neg_lds;         /* 0 / 1: the per-brick bits are in LDS */
  int32_t  shared_grad;     /* RaycastArgs::shared_grad: 0 / 1 / 2 */
  int32_t  view_half;       /* the gathers' view in brick layers to either side (0: most) */
  int32_t  pyramid;         /* 0 / 1: levels 1 and 2 of the model maps' pyramids were written by this launch */
  uint32_t grid;            /* workgroups of the launch (the riders' included) */
  uint32_t calls;           /* raycast launches since kf_create */
} kf_raycast_form;
int kf_get_raycast_form(kf_ctx* ctx, kf_raycast_form* out);

/* cudaIntegrateVolume  src/cuda/integrateVolume.cu:78-96.  transform == NULL: use the device-resident pose and
 * integrate only if the last kf_*_track call tracked (src/HybKinectfu.cpp:123-140).
 * Three launches per streamed frame: after a call with transform == NULL the next kf_icp_track (persistent loop, volumes without deferred weights
 * and of at most ~6400 macro cells of 32^3 voxels) runs this call's brick cull as the tail of its own launch, for the parameters seen here; the
 * kf_integrate_volume that follows consumes it when it asks for exactly that (pose on the device, same parameters, depth map, slab) and
 * otherwise undoes it and culls in a launch of its own -- the result never depends on it.  kf_cull_tail_counts: how often either happened. */
int kf_integrate_volume(kf_ctx* ctx, int has_color, int use_angle_weight_color, const kf_mat44* transform,
                        const kf_integrate_params* integrate_params, const kf_camera_params* depth_camera,
                        const kf_camera_params* rgb_camera);
/* Deferred free-space weights (no reference counterpart: a property of this implementation of integrateKernel / updateVoxel,
 * src/cuda/integrateVolume.cu:15-77, src/cuda/tsdfVolume.h:57-75 -- results are bit-identical either way).  A wave of the fusion pass
 * whose 128 voxels all hold tsdf 1 and are all observed as free space again only counts the observation; the count is applied to the
 * weights (w <- fminf(w + k, max_weight)) when anything else writes into those voxels and by kf_download_volume.  mode 1: on, 0: off (the
 * plain read-modify-write kernel on every frame), -1 (default): on for volumes of 768^3 voxels and finer, where the fusion pass is memory-bound
 * (KF_INTEGRATE_SAT=0 / 2 in the environment: never / always).  Needs 1 <= max_weight <= 65000 and no colour; otherwise the plain kernel runs
 * whatever the mode. */
int kf_set_defer(kf_ctx* ctx, int mode);
/* cudaRaycastingVolume  src/cuda/raycastingVolume.cu:158-176.  transform == NULL: device-resident pose. */
int kf_raycast_volume(kf_ctx* ctx, int has_color, const kf_mat44* transform, const kf_raycast_params* raycast_params,
                      const kf_camera_params* depth_camera, float near_plane, float far_plane);

/* z-slab partitioning (no counterpart in the single-GPU reference: raycastKernel / raySample / gradientForPoint,
 * src/cuda/raycastingVolume.cu:16-156, run on one whole volume).  What pipeline.SlabPipeline runs per frame:
 *   kf_raycast_volume_slab_cross  every slab context marches every ray and writes, per pixel, ONE 64-bit word: (bits of the ray parameter of the first
 *                                 crossing whose negative sample lies in the layers it owns) << 32 | bits of the VERTEX's ray parameter alpha
 *                                 (:89-90) -- +inf / 0 without a crossing, alpha 0 where the reference gives up at the crossing (:87-88);
 *   MIN all-reduce of the words   (caller; positive floats order like their bits: the first crossing along the ray wins and brings its alpha);
 *   kf_slab_ray_normals           every context rebuilds the winners' vertices from the pixels' rays -- a pure function of pose and camera, which all
 *                                 contexts hold bit for bit -- and the one that OWNS a vertex's voxel layer evaluates gradientForPoint (:16-42) for it:
 *                                 dev_cand[px] = 3 floats (the unit normal), all-zero bits elsewhere.  (The vertex is an extrapolation that can land far from the
 *                                 crossing, outside the crossing slab's halo: its taps belong to the vertex's owner.)
 *   integer SUM all-reduce        of dev_cand (caller; one contributor per pixel: the owner's bits);
 *   kf_set_model_maps_rays        vertices from alpha, normals from dev_cand -> model maps and levels 1, 2 of their pyramids.
 * Same transform / camera / increment / planes in all three calls (NULL transform: the device-resident pose). */
int kf_raycast_volume_slab_cross(kf_ctx* ctx, const kf_mat44* transform, const kf_raycast_params* raycast_params,
                                 const kf_camera_params* depth_camera, float near_plane, float far_plane, uint64_t* dev_ta);
int kf_slab_ray_normals(kf_ctx* ctx, const kf_mat44* transform, const kf_raycast_params* raycast_params, const kf_camera_params* depth_camera,
                        float near_plane, float far_plane, const uint64_t* dev_ta_min, float* dev_cand);
int kf_set_model_maps_rays(kf_ctx* ctx, const kf_mat44* transform, const kf_camera_params* depth_camera, const uint64_t* dev_ta_min, const float* dev_cand);
/* The same merge with the normals evaluated SPECULATIVELY by the marching launch (what pipeline.SlabPipeline runs): a context's own crossing is the likely
 * winner of its pixel, and its vertex nearly always lies in the layers the context owns -- so kf_raycast_volume_slab_cross_spec also evaluates
 * gradientForPoint (:16-42) there, in the shadow of the march, and leaves dev_ta_own[px] = a second copy of its word (the caller all-reduces dev_ta in place)
 * and dev_spec[px] = 3 floats: that gradient, or zeros when the vertex is not this context's.  kf_slab_ray_normals_spec then copies dev_spec where the
 * context's own word won (dev_ta_own[px] == dev_ta_min[px]) and evaluates only the rest -- vertices this context owns under a crossing another context
 * met.  Same dev_cand as kf_slab_ray_normals, bit for bit; the caller pairs the buffers of ONE frame (same volume state, pose, camera, increment, planes). */
int kf_raycast_volume_slab_cross_spec(kf_ctx* ctx, const kf_mat44* transform, const kf_raycast_params* raycast_params, const kf_camera_params* depth_camera,
                                      float near_plane, float far_plane, uint64_t* dev_ta, uint64_t* dev_ta_own, float* dev_spec);
int kf_slab_ray_normals_spec(kf_ctx* ctx, const kf_mat44* transform, const kf_raycast_params* raycast_params, const kf_camera_params* depth_camera,
                             float near_plane, float far_plane, const uint64_t* dev_ta_min, const uint64_t* dev_ta_own, const float* dev_spec, float* dev_cand);
/* COLOUR FORMS of the ray-form merge, for contexts created with has_color (KF_ERR_STATE without a colour plane).  The candidate is 4 words per
 * pixel: the normal's three, then the uchar4 colour word (b, g, r, 0 from the low byte up) of interpolateColor at the VERTEX org + dir * alpha
 * (raycastingVolume.cu:91-92, tsdfVolume.h:123-148); all-zero bits = no colour.  The colour is the vertex OWNER's to evaluate, like the gradient (its
 * eight voxels lie within one layer of the vertex's), and it is evaluated before and independently of the gradient: a pixel whose gradient fails keeps
 * its colour, as in kf_raycast_volume(has_color = 1).  One contributor per pixel, so the integer SUM over 4 words returns its bits.
 *   kf_raycast_volume_slab_cross_spec_color   kf_raycast_volume_slab_cross_spec with dev_spec of 4 words per pixel (normal, colour), zeros when the
 *                                             vertex is not this context's.  A kernel of its own: a pending kf_prefetch_frame does not ride in it
 *                                             (the note is void at the next kf_preprocess; same bits).
 *   kf_slab_ray_normals_color                 both uses in one: with dev_ta_own / dev_spec it copies the speculated 4 words where the context's own
 *                                             word won and evaluates gradient AND colour for the vertices it owns under another context's crossing;
 *                                             with both NULL it evaluates every vertex it owns.  dev_cand: 4 words per pixel, zeros elsewhere.
 *   kf_set_model_maps_rays_color              kf_set_model_maps_rays from 4-word candidates; also writes KF_MAP_RAYCAST_RGB from the fourth word, whatever
 *                                             the normal.  Every pixel of the three maps is written.
 * Colour excludes deferred weights (kf_set_defer): a colour context runs the plain fusion kernel at every volume size. */
int kf_raycast_volume_slab_cross_spec_color(kf_ctx* ctx, const kf_mat44* transform, const kf_raycast_params* raycast_params, const kf_camera_params* depth_camera,
                                            float near_plane, float far_plane, uint64_t* dev_ta, uint64_t* dev_ta_own, float* dev_spec);
int kf_slab_ray_normals_color(kf_ctx* ctx, const kf_mat44* transform, const kf_raycast_params* raycast_params, const kf_camera_params* depth_camera,
                              float near_plane, float far_plane, const uint64_t* dev_ta_min, const uint64_t* dev_ta_own, const float* dev_spec, float* dev_cand);
int kf_set_model_maps_rays_color(kf_ctx* ctx, const kf_mat44* transform, const kf_camera_params* depth_camera, const uint64_t* dev_ta_min, const float* dev_cand);
/* MAP FORM of the merge (the earlier protocol, kept for per-kernel tests): the slab that meets a crossing evaluates the whole hit itself -- dev_t[px] =
 * the crossing's ray parameter (+inf if none), dev_v / dev_n[px] = float4 vertex / normal (zeros when the march gives up there) -- and the caller keeps,
 * per pixel, the entry with the smallest t (kf_slab_mask_candidates zeroes the losers for an integer SUM).  It drops the rare pixel whose extrapolated
 * vertex leaves the crossing slab's halo; SlabPipeline does not use it. */
int kf_raycast_volume_slab(kf_ctx* ctx, int has_color, const kf_mat44* transform, const kf_raycast_params* raycast_params,
                           const kf_camera_params* depth_camera, float near_plane, float far_plane,
                           float* dev_t, float* dev_v, float* dev_n);
int kf_slab_mask_candidates(kf_ctx* ctx, const float* dev_t, const float* dev_tmin, float* dev_v, float* dev_n);
int kf_set_model_maps_device(kf_ctx* ctx, const float* dev_v, const float* dev_n);   /* model_{vertices,normals}_pyramid[0] <- device buffers */

/* Pixel-partitioned ICP ("partition pixels across GPUs, all-reduce the 27-float system").  `dev_sums` is a
 * caller-owned 32-float device buffer.  kf_icp_partition_begin builds the pyramids and arms the loop; for step = 0 ..
 * kf_icp_partition_steps()-1, kf_icp_partition_step consumes the all-reduced system of the previous step from dev_sums,
 * sums this rank's share (image rows part/parts) of the pixels and leaves its 27 sums in dev_sums for the caller to
 * all-reduce (SUM); kf_icp_partition_finish applies the last system and commits the pose.  Asynchronous. */
int kf_icp_partition_begin(kf_ctx* ctx, uint32_t frame_id);
int kf_icp_partition_steps(kf_ctx* ctx);
int kf_icp_partition_step(kf_ctx* ctx, uint32_t step, const kf_icp_params* icp, const kf_camera_params* depth_camera,
                          uint32_t part, uint32_t parts, float* dev_sums);
int kf_icp_partition_finish(kf_ctx* ctx, const kf_icp_params* icp, const float* dev_sums);
/* The same protocol for CameraPoseFinderSDF on z-slabs (src/CameraPoseFinderSDF.cpp:44-106, src/cuda/CalSDFErrSolverParams.cu:68-138): a pixel is
 * summed by the context that OWNS the voxel of its world point (the 13 lookups around it reach into the halo at most: a thinner halo is
 * refused with an argument error); the caller all-reduces (SUM) the 27-float system in `dev_sums` between the calls.  All max_iter_nums steps
 * are issued on every rank (after convergence they return at once), so the ranks' collective calls line up. */
int kf_sdf_partition_begin(kf_ctx* ctx, uint32_t frame_id);
int kf_sdf_partition_step(kf_ctx* ctx, uint32_t step, const kf_sdf_tracker_params* params, const kf_camera_params* depth_camera, float* dev_sums);
int kf_sdf_partition_finish(kf_ctx* ctx, const kf_sdf_tracker_params* params, const kf_camera_params* depth_camera, const float* dev_sums);

/* cudaMarchingcube  src/cuda/marchingcube.cu:154-164.  Triangles are appended after those already stored
 * (the reference never clears its counter, src/cuda/MarchingcubeData.h:56,99) in the canonical order (z, y, x, k). */
int kf_marching_cubes(kf_ctx* ctx, int has_color, float threshold_marchingcube);
int kf_clear_triangles(kf_ctx* ctx);                                   /* MarchingcubeData::clearData */
int kf_triangle_count(kf_ctx* ctx, uint32_t* count);                   /* MarchingcubeData::triangleNums, blocking */
int kf_read_triangles(kf_ctx* ctx, kf_triangle* dst, uint32_t first, uint32_t count);   /* MarchingcubeData::clone(CPU) */
/* the counterpart of kf_read_triangles (MarchingcubeData::clone towards the device, src/cuda/MarchingcubeData.h:129): host triangles into
 * [first, first + count) of the buffer; the triangle count becomes first + count.  KF_ERR_ARG beyond max_triangles.  Blocking.
 * What welds a soup that did not come from this context's volume. */
int kf_write_triangles(kf_ctx* ctx, const kf_triangle* src, uint32_t first, uint32_t count);

/* The indexed mesh of the triangles in the buffer, made on the device: what MeshGeneratorMarchingcube::saveMesh does on one host thread
 * between its copy and its file writer (src/MeshGeneratorMarchingcube.cpp:69-86) -- MeshData::mergeCloseVertices(thresh, approx)
 * with its closing removeDegeneratedFaces (src/utils/mesh/meshData.cpp:179-310), removeDuplicateFaces (:42-82) and
 * computeVertexNormals (src/utils/mesh/meshData.h:713-736).  Same vertices, face indices and normals, bit for bit, whatever the
 * scheduling.  The reference welds with thresh = 0.0001f.  The soup is only read: kf_read_triangles returns it unchanged afterwards.
 * Scratch and mesh live in the context: allocated on the call, kept for the next one, freed by kf_weld_release / kf_destroy.
 * KF_ERR_ARG: thresh <= 0, more than 2^32 / 3 triangles.  KF_ERR_ALLOC: no memory for the scratch (also above ~357 M triangles).  An
 * empty buffer gives an empty mesh.  Blocks a few times on a 4-byte read-back (one per round of the cell selection, see n_rounds). */
int kf_weld_mesh(kf_ctx* ctx, int has_color, float thresh);
/* sizes of the last kf_weld_mesh's mesh and the rounds its cell selection took (1 - 3 on real soups); KF_ERR_STATE before a weld.  Blocking.
 * (the sizes of MeshData's m_Vertices and m_FaceIndicesVertices, src/utils/mesh/meshData.h:561-569) */
int kf_mesh_counts(kf_ctx* ctx, uint32_t* n_vertices, uint32_t* n_faces, uint32_t* n_rounds);
/* the mesh itself (MeshData's m_Vertices, m_Normals, m_Colors, m_FaceIndicesVertices, src/utils/mesh/meshData.h:561-569, as MeshGeneratorMarchingcube.cpp:39-58 fills them):
 * vertices / normals 3 floats, colours 4 floats (rgba: the triangle's colour with x and z swapped, a = 1, :53; written only after a weld
 * with has_color), faces 3 indices each.  Any pointer may be NULL.  KF_ERR_STATE before a weld.  Blocking. */
int kf_read_mesh(kf_ctx* ctx, float* vertices, float* normals, float* colors, uint32_t* faces);
/* frees the weld's scratch and mesh (MeshData::clear, src/utils/mesh/meshData.h:440); the next kf_weld_mesh allocates again */
int kf_weld_release(kf_ctx* ctx);

/* The parts of the mesh, and dropping the small ones on the device.  The reference has nothing for it (MeshData knows removeIsolatedVertices,
 * src/utils/mesh/meshData.cpp:320-356, and no notion of a piece); every user of such a mesh removes the crumbs that sensor noise and half-observed
 * bricks leave floating in free space, by face count or by keeping the largest piece.  The rule:
 *   input mesh      the mesh of the last kf_weld_mesh: n_v vertices, n_f faces.
 *   connectivity    two vertices are connected when one face names both; a PART is a connected set of vertices.
 *   label           a part's label is the smallest vertex index in it.
 *   face membership a face belongs to the part of its vertices (all three lie in one part by construction).
 *   part size       part_faces(label) = the number of faces of the part.
 *   orphans         a vertex that no face names is an orphan: a part of 0 faces (the weld leaves one where a vertex's only faces were degenerate).
 *   keep            with min_faces and largest_only, a part is kept iff part_faces >= max(min_faces, 1); orphans never are.
 *   largest only    with largest_only != 0 a part is additionally kept only if it has the greatest face count; a tie goes to the smallest label.
 *                   Nothing is kept if no part reaches min_faces.
 *   face order      kept faces stay in their order.
 *   vertex order    kept vertices stay in ascending old index and are renumbered densely -- the soup's order, like everything the weld emits, and NOT
 *                   the first-use order of removeIsolatedVertices.
 *   attributes      positions, normals and colours of kept vertices are copied verbatim.  Normals are not recomputed: every face that names a kept vertex
 *                   is kept, in the same relative order, so computeVertexNormals would add the same unit normals in the same order and give the same bits.
 *   faces           are remapped to the new vertex indices.
 * Every output is a function of the mesh alone, whatever the scheduling: integer atomics only, labelling in rounds with one 4-byte read-back each.
 *
 * kf_mesh_parts: labels the current mesh.  n_parts: parts with at least one face; largest_faces: the face count of the largest; n_orphans; n_rounds: the
 *   rounds the labelling took (at most n_v).  Any pointer may be NULL.  Blocking.  KF_ERR_ARG on a NULL context, KF_ERR_STATE before a weld or after
 *   kf_weld_release.  An empty mesh gives zeros.  The labels are kept until the next weld, drop or release.
 * kf_read_mesh_parts: per vertex its part's label and its part's face count, n_v words each; either may be NULL.  Labels the mesh first if that was not done.
 * kf_mesh_drop_parts: rewrites the mesh by the rule.  parts_dropped: parts with a face that went; orphans_dropped: orphans that went (all of them).
 *   Afterwards kf_mesh_counts and kf_read_mesh report the cleaned mesh, n_rounds unchanged.  The soup is only read (kf_read_triangles is unchanged), a
 *   second identical call changes nothing, and the next kf_weld_mesh gives the full mesh again.  The buffers are the context's, grown as the weld's are
 *   and freed by kf_weld_release / kf_destroy. */
int kf_mesh_parts(kf_ctx* ctx, uint32_t* n_parts, uint32_t* largest_faces, uint32_t* n_orphans, uint32_t* n_rounds);
int kf_read_mesh_parts(kf_ctx* ctx, uint32_t* vertex_label, uint32_t* vertex_part_faces);
int kf_mesh_drop_parts(kf_ctx* ctx, uint32_t min_faces, int largest_only, uint32_t* parts_dropped, uint32_t* orphans_dropped);

/* Viewer frames.  The reference shows three pictures per frame (src/HybKinectfu.cpp:145-158): DataViewer::viewNormal on the new and the model
 * normals and DataViewer::viewColors on the raycast colours -- each a blocking clone(CPU) of a whole map and a loop on one host thread
 * (src/DataViewer.cpp:13-44).  Here the picture is made on the device, 4 bytes per pixel (b, g, r, a from the low byte up) in a context-owned image
 * that grows on demand and is freed by kf_destroy; both producers are asynchronous on the context's stream, so a view enqueued after
 * kf_integrate_volume sees that frame's volume.  Bytes 0-2 by mode, byte 3 = 255 on a hit (vertex w == 1), else 0; fp32, one rounding per operation:
 *   KF_VIEW_NORMALS  (unsigned char)((255.f * (n.c + 1.f)) / 2.f) for c = x, y, z: DataViewer.cpp:24-26 byte for byte (127, 127, 127 without a normal);
 *   KF_VIEW_SHADED   one grey level, 0 without a hit: d = eye - v (eye: the pose's translation), s = (d.x*d.x + d.y*d.y) + d.z*d.z,
 *                    c = ((n.x*d.x + n.y*d.y) + n.z*d.z) / sqrtf(s) clamped to [0, 1] (NaN -> 0), g = (unsigned char)(32.f + 223.f * c);
 *   KF_VIEW_COLOR    b, g, r of interpolateColor at the vertex (src/cuda/raycastingVolume.cu:91-92): KF_MAP_RAYCAST_RGB's bytes, kept whether or
 *                    not the gradient succeeded, 0 without a crossing.  KF_ERR_STATE on a context without a colour plane.
 * kf_render_view: a free viewpoint -- the march of kf_raycast_volume (raycastKernel, src/cuda/raycastingVolume.cu:121-156: same vertices, normals
 *   and colours, bit for bit) for `view_cam`, any size from 1 to 4096 each way, from `pose` (NULL: the device-resident pose).  dev_v / dev_n: optional
 *   caller-owned float4 maps of view_cam's size that receive what kf_raycast_volume would have written; either may be NULL.  It is a bystander to
 *   tracking: the model maps, KF_MAP_RAYCAST_RGB, kf_get_raycast_form's record, a pending kf_prefetch_frame and the stage timers are left as they
 *   are.  KF_ERR_ARG: bad mode, bad camera, NULL context or increment.  KF_ERR_STATE: a z-slab context that does not own the whole volume (it sees
 *   only its own layers: the free viewpoint over z-slabs is the merged view below, which kf_group_render_view of hybkf_group.h runs).
 * kf_view_model_maps: the tracking camera's view without a march -- the same bytes from level 0 of the context's CURRENT model maps,
 *   KF_MAP_RAYCAST_RGB and the device-resident pose.  Allowed on z-slab contexts: after kf_set_model_maps_rays every member holds the merged maps.
 * kf_view_size: the size of the last view (KF_ERR_STATE before one).  kf_view_device: the image in HBM, valid in stream order until the next view
 *   (NULL before one).  kf_read_view: blocking copy of cols * rows * 4 bytes.
 * kf_render_view_at: kf_render_view of a window that stands ELSEWHERE (no reference counterpart: the reference's cube never moves) -- the display bytes and
 *   the optional dev_v / dev_n maps, bit for bit, that kf_render_view would produce after kf_shift_volume had moved the window to frame_origin_vox (voxels of
 *   the first cube, multiples of 8) with the brick store's bricks restored; it moves nothing.  A brick is read from the window's copy where its world brick
 *   lies in the window (the newer copy), else from the store's slot, else from one shared all-zero brick: kf_marching_cubes_at's rule.  `pose` is given in the
 *   virtual frame's coordinates, the numbers one would hand kf_render_view after that shift; NULL: the device-resident pose as that shift would have left it,
 *   t - (float)(frame - origin) * cell per axis, computed on the device (no read-back).  Asynchronous on the context's stream; the image is the context's view
 *   image (kf_view_size / kf_view_device / kf_read_view).  A bystander, strictly: volume, flags, skip tables, deferred-weight words (neither consulted nor
 *   flushed), store, device pose, model maps, KF_MAP_RAYCAST_RGB, kf_get_raycast_form's record, a pending kf_prefetch_frame, stage timers, work counters,
 *   the triangle buffer and the extraction scratch are what they were.  A context without a reserved store is no error: window or zero.
 *   KF_ERR_ARG: NULL context, frame, camera or increment, bad mode, bad camera (kf_render_view's limits), a frame component that is not a multiple of 8, a
 *   frame whose bricks fall outside the brick key range or that kf_shift_volume could not reach in one call.  KF_ERR_STATE: KF_VIEW_COLOR without a colour
 *   plane, a z-slab context.  On any error nothing is touched and the last view stays the last view. */
enum { KF_VIEW_NORMALS = 0, KF_VIEW_SHADED = 1, KF_VIEW_COLOR = 2 };
int kf_render_view(kf_ctx* ctx, int mode, const kf_mat44* pose, const kf_camera_params* view_cam, const kf_raycast_params* raycast_params,
                   float near_plane, float far_plane, float* dev_v, float* dev_n);
int kf_render_view_at(kf_ctx* ctx, int mode, const int32_t frame_origin_vox[3], const kf_mat44* pose, const kf_camera_params* view_cam,
                      const kf_raycast_params* raycast_params, float near_plane, float far_plane, float* dev_v, float* dev_n);
int kf_view_model_maps(kf_ctx* ctx, int mode);
int kf_view_size(kf_ctx* ctx, uint32_t* cols, uint32_t* rows);
const uint8_t* kf_view_device(kf_ctx* ctx);
int kf_read_view(kf_ctx* ctx, uint8_t* dst, size_t dst_bytes);
/* A MERGED VIEW over z-slabs: the ray-form merge (kf_raycast_volume_slab_cross_spec ... kf_set_model_maps_rays above) for the CALLER's camera, ending
 * in display bytes.  The three per-member steps; the caller runs the two all-reduces between them (kf_group_render_view does all five).  All take
 * view_cam with kf_render_view's limits (1 .. 4096 each way, any size whatever the context's), `pose` (NULL: the device-resident pose), are asynchronous
 * on the context's stream, are accepted on z-slab contexts and on a whole-volume context (which owns every layer), and are bystanders to tracking
 * exactly as kf_render_view is: the model maps, KF_MAP_RAYCAST_RGB, kf_get_raycast_form's record, a pending kf_prefetch_frame, the stage timers and
 * the work counters are left as they are.  Buffers are caller-owned device memory of view_cam's pixel count.
 *   kf_view_slab_cross    the march of kf_raycast_volume_slab_cross_spec (color != 0: of ..._spec_color, dev_spec 4 words per pixel) for view_cam: the
 *                         same words, second copy and speculation, bit for bit, whenever view_cam is the context's camera.  KF_ERR_ARG: a halo thinner
 *                         than ceil(ray_increment / voxel) + 2 layers, a bad camera, a NULL buffer.  KF_ERR_STATE: color without a colour plane.
 *   kf_view_slab_normals  kf_slab_ray_normals_spec / kf_slab_ray_normals_color (color != 0: dev_spec, dev_cand 4 words per pixel) for view_cam.
 *                         dev_ta_own and dev_spec may both be NULL: then every owned vertex is evaluated.
 *   kf_view_from_rays     vertices from alpha, normals and (words = 4) colours from the summed candidates, through the pixel function above into the
 *                         context's view image: kf_view_size / kf_view_device / kf_read_view follow as after any other view.  The eye is the pose's
 *                         translation.  The colour bytes are kept whether or not a normal was found; byte 3 is 255 only where the candidate normal has
 *                         a set bit.  dev_v / dev_n: optional float4 maps that receive what kf_raycast_volume would have written on the whole volume.
 *                         Every pixel of the image and of the maps is written.  words: 3 or 4; KF_VIEW_COLOR needs 4 (KF_ERR_ARG otherwise). */
int kf_view_slab_cross(kf_ctx* ctx, int color, const kf_mat44* pose, const kf_camera_params* view_cam, const kf_raycast_params* raycast_params,
                       float near_plane, float far_plane, uint64_t* dev_ta, uint64_t* dev_ta_own, float* dev_spec);
int kf_view_slab_normals(kf_ctx* ctx, int color, const kf_mat44* pose, const kf_camera_params* view_cam, const kf_raycast_params* raycast_params,
                         float near_plane, float far_plane, const uint64_t* dev_ta_min, const uint64_t* dev_ta_own, const float* dev_spec, float* dev_cand);
int kf_view_from_rays(kf_ctx* ctx, int mode, const kf_mat44* pose, const kf_camera_params* view_cam, const uint64_t* dev_ta_min, const float* dev_cand,
                      uint32_t words, float* dev_v, float* dev_n);

/* CudaMap2D::clone(CPU) / copyDataFrom on the singleton's maps (debug + parity; blocking) */
int kf_download_map(kf_ctx* ctx, int map_id, uint32_t level, void* dst, size_t dst_bytes);
int kf_upload_map(kf_ctx* ctx, int map_id, uint32_t level, const void* src, size_t src_bytes);
/* volume in the reference's index order (z*R+y)*R+x for stored layers [z_begin, z_end): tsdf, weight (float) and
 * colour (3 bytes/voxel, may be NULL).  Blocking. */
int kf_download_volume(kf_ctx* ctx, uint32_t z_begin, uint32_t z_end, float* tsdf, float* weight, uint8_t* color);
int kf_upload_volume(kf_ctx* ctx, uint32_t z_begin, uint32_t z_end, const float* tsdf, const float* weight, const uint8_t* color);
int kf_get_volume_stats(kf_ctx* ctx, kf_volume_stats* out);                /* blocking.  weight_gt0 -- the count the reference prints per frame,
                                                                              integrateVolume.cu:91-94 -- comes from a sweep of the volume for a host that asks now
                                                                              and then; asked twice within 8 fused frames, the fusion launches keep it as a running
                                                                              count (+3.6 us per frame at 512^3) and the call is a read-back until 64 frames pass
                                                                              without a question (KF_OBSERVED_COUNT=0 / 1: always sweep / always count) */
int kf_get_fusion_counters(kf_ctx* ctx, kf_volume_stats* out);             /* the same read-back WITHOUT the observed-voxel count (weight_gt0 = 0): never sweeps, and does
                                                                              not count as a question for that count -- what a measurement harness brackets its regions with */
int kf_count_observed_voxels(kf_ctx* ctx, uint64_t* out);                  /* the same number by a sweep of the owned layers (blocking): the tests' cross-check
                                                                              of the running count; src/cuda/integrateVolume.cu:78-96 counts the same way */
int kf_stored_z_range(kf_ctx* ctx, uint32_t* z_begin, uint32_t* z_end);

/* z-slab re-balancing (BASELINE.json north_star "xGMI ... exchange of boundary slabs").  No reference counterpart: the reference
 * holds one whole volume (src/cuda/tsdfVolume.h:29-37).
 * kf_download_volume_device / kf_upload_volume_device: kf_download_volume / kf_upload_volume with caller-owned DEVICE buffers, asynchronous on the
 *   context's stream -- the planes two ranks exchange (torch.distributed send / recv: RCCL point-to-point) when a brick layer changes its owner.
 * kf_resize_slab: the context now owns [z_begin, z_end) (+ halo): layers stored before and after keep their voxels, new layers read as never observed
 *   until uploaded, the rest is dropped; pose, tracker state, frame maps and counters stay.  Blocking.
 * kf_count_layer_work / kf_read_layer_work: per brick layer (resolution / 8 entries) the voxels of queued bricks the next `frames` integrate calls update:
 *   the work measure the boundaries are balanced on. */
int kf_download_volume_device(kf_ctx* ctx, uint32_t z_begin, uint32_t z_end, float* dev_tsdf, float* dev_weight, uint8_t* dev_color);
int kf_upload_volume_device(kf_ctx* ctx, uint32_t z_begin, uint32_t z_end, const float* dev_tsdf, const float* dev_weight, const uint8_t* dev_color);
int kf_resize_slab(kf_ctx* ctx, uint32_t z_begin, uint32_t z_end, uint32_t halo);
int kf_count_layer_work(kf_ctx* ctx, int frames);
int kf_read_layer_work(kf_ctx* ctx, uint64_t* out, int reset);                /* blocking */

/* The moving volume (no reference counterpart: the reference's cube stays where HybKinectfu::init put it, src/HybKinectfu.cpp:51-54).
 * kf_shift_volume: the window moves by +d voxels, each component a multiple of 8 (whole bricks).  Afterwards voxel (x, y, z) holds what voxel
 *   (x + dx, y + dy, z + dz) held before wherever that lies inside the volume -- (tsdf, weight), colour and the brick's deferred-weight state
 *   (kf_set_defer stays in force) --, and everything else reads as after kf_reset_volume unless the brick store holds the brick (below).
 *   |d| >= resolution on an axis leaves an empty volume;
 *   d = (0, 0, 0) returns 0 without enqueuing anything.  The device-resident pose moves with the contents, on the device:
 *   t <- t - (float)d * cell (cell = size_m / resolution, the fp32 quotient) and its inverse is recomputed; the tracked / lost verdict stays.
 *   In place (no second volume), asynchronous on the context's stream, no allocation and no synchronisation: it may sit between two frames
 *   of a streamed run.  Brick flags, skip tables and the observed-voxel count follow as after kf_upload_volume.
 *   THE MODEL MAPS ARE STALE AFTERWARDS: they are not translated.  Call kf_raycast_volume(transform = NULL) before the next kf_icp_track /
 *   kf_sdf_track; then "shifted here" equals "uploaded there" bit for bit.
 *   KF_ERR_ARG, with nothing touched and nothing enqueued: a component that is no multiple of 8; any non-zero shift on a z-slab context
 *   (one that does not store the whole volume: a z shift needs a layer exchange between the members -- slab groups cannot shift yet);
 *   a sum of shifts beyond 32 bits; with a brick store, a brick of the old or the new window outside [-2^20, 2^20) (below).
 * kf_volume_origin: the sum of all shifts since kf_create / kf_reset_volume, in voxels: where voxel (0, 0, 0) of the window lies in the first
 *   cube.  World position = volume position + origin * cell.  Host bookkeeping: never blocks.  Zero on a context that never shifts. */
int kf_shift_volume(kf_ctx* ctx, int32_t dx, int32_t dy, int32_t dz);
int kf_volume_origin(kf_ctx* ctx, int32_t origin_vox[3]);

/* The moving volume on z-slab contexts (shift.hip): what a slab group runs on its members (hybkf_group.h: kf_group_shift_volume).  kf_shift_volume
 * itself keeps refusing a z-slab context.  A context stores brick layers [bz0, bz1) = kf_stored_z_range / 8.
 * THE RULE: stored destination brick (bx, by, p) takes source brick (bx + dx/8, by + dy/8, p + dz/8) -- from the context's own copy where that layer is
 *   stored here (owned or halo: a halo layer holds its owner's bits), else from the feed buffer where the layer lies in the feed range, else it reads
 *   as never observed; a source whose x or y lies outside the volume reads as never observed too.  So halo layers become owned layers and back.
 * THE TRANSIT LAYOUT of one brick layer, kf_slab_layer_bytes(ctx) bytes (n = (resolution / 8)^2 bricks, brick (bx, by) at index by * (resolution / 8) + bx):
 *   n x 4 KiB of (tsdf, weight), brick after brick as they lie in the volume (voxel (x, y, z) of a brick at ((z & 7) << 6 | (y & 7) << 3 | (x & 7)));
 *   then, on a context with a colour plane, n x 2 KiB of colour (4 bytes per voxel, same order); then n 8-byte deferred-weight words, padded to a
 *   multiple of 16 bytes.  The layers of a range follow each other at that pitch.  It is what two members exchange.  0 for a NULL context.
 * kf_slab_shift_needs: host bookkeeping, never blocks.  The half-open range of GLOBAL brick layers this context must be fed for a z shift of dz: the
 *   source layers p + dz/8 of its stored layers p that lie in [0, resolution / 8) and are not stored here.  Always one range; (0, 0) when empty
 *   (dz = 0, a whole-volume context, a shift out of the volume).  KF_ERR_ARG for a dz that is no multiple of 8.
 *   kf_slab_needs: the same rule without a context, for stored voxel layers [stored_z_begin, stored_z_end) (kf_stored_z_range's) of a volume of
 *   `resolution` -- what a planner uses (kf_group_shift_plan); no HIP call.  KF_ERR_ARG for a range that is empty, not brick-aligned or outside.
 * kf_slab_pack_layers: asynchronous on the context's stream.  The stored brick layers [bz_begin, bz_end) into the caller's device buffer dev_dst
 *   ((bz_end - bz_begin) * kf_slab_layer_bytes bytes, 16-byte aligned) in the transit layout, x and y as they lie.  The deferred weights are
 *   flushed first, so the bytes do not depend on how a brick's weights were split between voxels and word: the words are states that travel
 *   verbatim.  KF_ERR_ARG for an empty range or one not stored here.
 * kf_shift_slab: kf_shift_volume's move under the rule above, in place, the planes walked in the safe order; the same pass rebuilds flags,
 *   has-negative bits and the context's skip tables; the deferred-weight words travel with their bricks.  The bookkeeping is kf_shift_volume's: the
 *   device-resident pose moves (every member of a group gets the same bits), kf_volume_origin advances, the observed-voxel count is re-based, and
 *   THE MODEL MAPS ARE STALE afterwards.  The owned and stored ranges do not change: they are window coordinates.  dev_feed holds the layers
 *   [feed_bz_begin, feed_bz_end) in the transit layout and is read in stream order.  Asynchronous: no allocation, no synchronisation.
 *   On a whole-volume context the need is empty and the call is kf_shift_volume without brick store or stream-out, bit for bit.
 *   A z shift wider than the slab is legal: the whole destination then comes from the feed or reads as never observed.
 *   Refused with nothing touched -- KF_ERR_ARG: a component that is no multiple of 8; a feed range that is not exactly kf_slab_shift_needs' (an empty
 *   need takes any empty range); a NULL feed with a non-empty need; a sum of shifts beyond 32 bits.  KF_ERR_STATE: a brick store reserved or
 *   stream-out on -- those stay whole-volume features of kf_shift_volume; a slab's window forgets what leaves it. */
size_t kf_slab_layer_bytes(kf_ctx* ctx);
int kf_slab_shift_needs(kf_ctx* ctx, int32_t dz, uint32_t* bz_begin, uint32_t* bz_end);
int kf_slab_needs(uint32_t resolution, uint32_t stored_z_begin, uint32_t stored_z_end, int32_t dz, uint32_t* bz_begin, uint32_t* bz_end);
int kf_slab_pack_layers(kf_ctx* ctx, uint32_t bz_begin, uint32_t bz_end, void* dev_dst);
int kf_shift_slab(kf_ctx* ctx, int32_t dx, int32_t dy, int32_t dz, const void* dev_feed, uint32_t feed_bz_begin, uint32_t feed_bz_end);

/* Streaming the departing surface into a world mesh (no reference counterpart).  kf_shift_volume overwrites what leaves the window; these
 * entry points keep its surface: a marching cubes limited to a box of cells, and a second, context-owned triangle buffer in WORLD coordinates
 * (world position = volume position + origin * cell, see kf_volume_origin) that outlives the window the triangles were extracted under.
 * kf_marching_cubes_region: exactly the triangles kf_marching_cubes emits for the cells lo <= (x, y, z) < hi (cells, half-open, any integers,
 *   clamped to [0, resolution)) -- every float and colour byte the same, in the canonical order (z, y, x, k) restricted to the box --, appended
 *   to what the destination holds and clamped at its capacity.  An empty or inverted box is a no-op that returns 0.  Its cost follows the box:
 *   only the bricks the box touches, widened by one brick, are tested and classified, and the 256-cell blocks are numbered inside the box.
 *   flags: KF_MC_WORLD -- every position component i becomes p + (float)origin[i] * cell (one fp32 multiply, one add: hkf_world_positions'
 *   expression; a zero origin leaves every bit); KF_MC_TO_WORLD_SOUP -- the destination is the world soup instead of the triangle buffer
 *   (KF_ERR_ARG without KF_MC_WORLD, KF_ERR_STATE without a reserved soup).  KF_ERR_ARG: NULL context or box, unknown flag bits, a z-slab
 *   context (one that does not store the whole volume).  KF_ERR_STATE: has_color without a colour plane, no destination.  Asynchronous.
 * kf_region_work: what the last kf_marching_cubes_region (or the last box of a streaming kf_shift_volume) visited -- out[0] = bricks whose voxels
 *   its class pass read, out[1] = 256-cell blocks listed.  Zeros after a no-op.  Blocking.
 * kf_world_soup_reserve: (re)allocates the world soup for max_triangles and clears it; 0 frees it (and switches stream-out off).  Blocking.
 * kf_world_soup_count: triangles held, and (dropped, may be NULL) the triangles that did not fit, summed since the last clear (saturating).
 *   Zeros without a soup.  Blocking.  kf_read_world_soup: as kf_read_triangles.  kf_clear_world_soup: both counts to zero (KF_ERR_STATE
 *   without a soup); kf_reset_volume does the same.
 * kf_append_world_soup: device to device, the world soup behind what the triangle buffer holds, clamped at max_triangles.  Asynchronous.
 * kf_set_stream_out: on != 0 -- from now on kf_shift_volume first extracts, with these marching-cubes parameters, into the world soup every
 *   cell whose 27 voxels include a voxel that is about to leave: along one axis with shift d > 0 the cells [0, d + 1), with d < 0 the cells
 *   [resolution + d - 1, resolution); over several axes the union as disjoint boxes in this order -- the x strip in full, the y strip without
 *   the x strip, the z strip without both --, each in canonical order.  Exactly these cells can never be extracted again (cell d becomes cell 0,
 *   whose lookups need voxel -1; cell d + 1 keeps its 27 voxels and is left for later), so a run of shifts in one direction loses nothing and
 *   emits nothing twice.  A window that comes back over old ground re-fuses it (or, with a brick store, gets it back: below) and streams it again
 *   when it leaves again: the soup then holds that surface twice.
 *   The volume, the pose and every later frame are what they are without stream-out, bit for bit.  KF_ERR_STATE without a reserved soup or
 *   with has_color on a context without a colour plane; KF_ERR_ARG on a z-slab context. */
enum { KF_MC_WORLD = 1, KF_MC_TO_WORLD_SOUP = 2 };
int kf_marching_cubes_region(kf_ctx* ctx, int has_color, float threshold_marchingcube, const int32_t lo[3], const int32_t hi[3], int flags);
int kf_region_work(kf_ctx* ctx, uint64_t out[2]);
int kf_world_soup_reserve(kf_ctx* ctx, uint32_t max_triangles);
int kf_world_soup_count(kf_ctx* ctx, uint32_t* count, uint32_t* dropped);
int kf_read_world_soup(kf_ctx* ctx, kf_triangle* dst, uint32_t first, uint32_t count);
int kf_clear_world_soup(kf_ctx* ctx);
int kf_append_world_soup(kf_ctx* ctx);
int kf_set_stream_out(kf_ctx* ctx, int on, int has_color, float threshold_marchingcube);

/* The brick store: the moving volume keeps what leaves and restores it on return (no reference counterpart: the reference's cube never moves, so
 * nothing ever leaves it).  A device-resident, sparse archive of bricks keyed by WORLD BRICK COORDINATE = origin / 8 + brick index (see
 * kf_volume_origin; the origin is always a multiple of 8), each component in [-2^20, 2^20).  Absent until reserved: a context that never reserves
 * one enqueues the launches and produces the bits it always did.
 * kf_shift_volume with a store: after the deferred weights are flushed and the departing cells are streamed out (kf_set_stream_out), and before
 *   anything moves, every brick that is about to leave (source brick q with q - d / 8 outside [0, resolution / 8) on some axis) and has a voxel of
 *   weight > 0 is copied into the store: its 512 (tsdf, weight) pairs, its colour on a context with a colour plane, its deferred-weight word.  A key
 *   the store already holds keeps its entry and is overwritten (the window's copy is the newer one); a new key takes the next free entry; when none
 *   is free the brick is counted as dropped and a later look-up of its key misses.  A brick never observed takes no entry.  After the move every
 *   brick that has entered (destination brick b with b + d / 8 outside) is looked up, read-only: on a hit the entry is copied back -- tsdf, weight,
 *   colour and deferred-weight word, bit for bit -- and the brick's flags, its has-negative bit and the skip tables follow as for a moved brick, so
 *   a shift away and back is lossless and "shifted here" still equals "uploaded there".  A restored brick stays in the store (a shift never
 *   deletes; only kf_brick_store_erase_box / _weak do); until it leaves again the window's copy is the only current one.  Still asynchronous, no allocation, no synchronisation: two more
 *   launches.  KF_ERR_ARG, with nothing touched and nothing enqueued, when a brick of the old or of the new window would have a world brick
 *   coordinate outside [-2^20, 2^20).  With stream-out on, a restored brick that leaves again is streamed again: the world soup is not de-duplicated.
 * kf_brick_store_reserve: (re)allocates the store for max_bricks bricks (4 KiB each, + 2 KiB with a colour plane, + a hash table of the next power of
 *   two >= 2 * max_bricks entries) and clears it; from then on every shift uses it.  0 frees it: shifts are what they were.  Blocking.  KF_ERR_ARG
 *   on a z-slab context or a NULL context; KF_ERR_ALLOC when the memory is not there -- the store is then absent.
 * kf_brick_store_count: bricks held, bricks dropped since the last clear, bricks restored since the last clear (cumulative).  Any pointer may be
 *   NULL.  Zeros without a store.  Blocking.
 * kf_brick_store_clear: no entries, all three counts zero (KF_ERR_STATE without a store); kf_reset_volume does the same, kf_destroy frees the store.
 * kf_read_brick_store: entries [first, first + count) as a sparse map of what the window has left behind: keys[i][3] the world brick coordinate
 *   (x, y, z); tsdf[i][512] and weight[i][512] in the in-brick order (z & 7) << 6 | (y & 7) << 3 | (x & 7) -- kf_download_volume's order restricted
 *   to the brick --, the weights being the TRUE weights kf_download_volume would have reported just before the brick left (the stored
 *   deferred-weight word applied); color[i][512][3] the colour bytes (untouched on a context without a colour plane).  Any pointer may be NULL.
 *   The order of the entries is unspecified, and stable as long as no shift, clear or reserve happens in between.  KF_ERR_ARG when
 *   first + count > held.  Blocking.
 * kf_brick_store_bounds: the box of the world brick coordinates the store holds, half-open: lo_brick <= key < hi_brick on every axis, taken over the
 *   held entries by one small reduction kernel.  lo == hi (all zeros) for an empty or absent store.  KF_ERR_ARG on a NULL pointer.  Blocking. */
int kf_brick_store_reserve(kf_ctx* ctx, uint32_t max_bricks);
int kf_brick_store_count(kf_ctx* ctx, uint32_t* held, uint64_t* dropped, uint64_t* restored);
int kf_brick_store_clear(kf_ctx* ctx);
int kf_read_brick_store(kf_ctx* ctx, uint32_t first, uint32_t count, int32_t* keys, float* tsdf, float* weight, uint8_t* color);
int kf_brick_store_bounds(kf_ctx* ctx, int32_t lo_brick[3], int32_t hi_brick[3]);

/* Saving and loading the map: the store written back, the window captured, the window placed (no reference counterpart).
 * kf_write_brick_store: kf_read_brick_store's inverse, the same layout and in-brick order.  Every entry with a weight > 0 ends up in a slot under its
 *   key -- (tsdf, weight) pairs, colour bytes (zeros when `color` is NULL on a context with a colour plane), a deferred-weight word of 0: the weights
 *   written are the true weights.  A key the store holds is overwritten in place: the caller's copy is the newer one.  An entry with no weight > 0 takes
 *   no slot; with the store full an entry is counted as dropped and claims nothing.  The window, the pose, the model maps and later frames are untouched.
 *   A written key that lies inside the current window is SHADOWED by the window's copy wherever window and store are read together (the source
 *   precedence of kf_marching_cubes_at and kf_render_view_at), and is overwritten when that brick next leaves the window.  The entries travel through a
 *   context-owned staging buffer (allocated by the first call, freed with the store) in chunks on the context's stream.  Blocking.  Refused with nothing
 *   touched -- KF_ERR_ARG: a NULL context; with count > 0, NULL keys, tsdf or weight, a key component outside [-2^20, 2^20), a key that occurs twice in
 *   the call (count == 0 writes nothing and looks at no array).
 *   KF_ERR_STATE: no store reserved; `color` on a context without a colour plane.
 * kf_brick_store_capture: every observed brick of the CURRENT window into the store, under the current origin, without a shift: pending weights are
 *   flushed as kf_shift_volume flushes them, then the eviction runs over all bricks.  Nothing moves; planes (as kf_download_volume reports them), pose,
 *   flags, tables and every later frame are bit for bit what they are without the call.  Afterwards the store alone holds the whole map (unless
 *   kf_brick_store_count's `dropped` grew).  Asynchronous.  KF_ERR_ARG on a z-slab context; KF_ERR_STATE without a store.
 * kf_place_window: stands the window at origin (ox, oy, oz), each a multiple of 8, filled from the store.  It leaves the state -- planes, flags,
 *   has-negative bits, skip tables, deferred-weight words, observed-voxel count, kf_volume_origin, the store and its counts -- that
 *   kf_brick_store_capture, a kf_shift_volume to a frame overlapping neither the old nor the new window (and no brick of the store), and a
 *   kf_shift_volume from there to (ox, oy, oz) leave, without stream-out; the device-resident pose is translated ONCE by (new - old origin), the pose
 *   kf_render_view_at(pose = NULL) uses for that frame.  The model maps are stale afterwards, as after a shift.  Blocks once (the store's counts):
 *   when the capture dropped a brick the call returns KF_ERR_ALLOC with window, origin and pose untouched (what was captured are harmless copies).
 *   Otherwise refused with nothing touched -- KF_ERR_ARG: a component that is no multiple of 8, a z-slab context, a brick of the old or the new window
 *   outside the key range.  KF_ERR_STATE: no store. */
int kf_write_brick_store(kf_ctx* ctx, uint32_t count, const int32_t* keys, const float* tsdf, const float* weight, const uint8_t* color);
int kf_brick_store_capture(kf_ctx* ctx);
int kf_place_window(kf_ctx* ctx, int32_t ox, int32_t oy, int32_t oz);

/* Merging maps: a second map fused into the store voxel by voxel, the window re-read from the store (no reference counterpart; the rule is the
 * reference's frame-into-volume running average, tsdfVolume.h:65-70, applied map to map).
 * kf_merge_brick_store: kf_write_brick_store's layout, in-brick order, staging, chunking and blocking behaviour, but a key the store already holds is
 *   MERGED with the incoming entry where a write overwrites it.  offset_brick (NULL: zero) is added to every key first: a translation by whole bricks
 *   between the two sessions' world frames; the key range [-2^20, 2^20) applies to the translated key.  A rigid transform between the maps -- a
 *   rotation, or a translation that is no whole number of bricks -- needs resampling: kf_merge_brick_store_rigid, below.  The target is the store only: a translated
 *   key inside the current window is shadowed by the window's copy exactly as a written one is (see kf_refill_window).
 *   An entry with no weight > 0 does nothing: it takes no slot and changes no held one.  A key not held claims a slot and is copied verbatim (colour
 *   zeros when `color` is NULL on a context with a colour plane), bit for bit what kf_write_brick_store writes; with the store full it is counted as
 *   dropped and claims nothing.  A key held is merged per voxel, in fp32, one rounded operation per operation written here, the division correctly
 *   rounded; a = the held voxel with its TRUE weight wa (what kf_read_brick_store reports), b = the incoming one:
 *     wb <= 0:   the voxel keeps ta and its colour; the weight stored is wa
 *     wa <= 0:   the voxel becomes (tb, wb, cb) verbatim ((tb * wb) / wb is not always tb)
 *     both > 0:  s = wa + wb;  t = (ta * wa + tb * wb) / s;  w = fminf(s, max_weight);
 *                each colour channel (unsigned char)fminf(255.f, ((float)ca * wa + (float)cb * wb) / s)
 *   With `color` NULL on a context with a colour plane the colour of a held slot stays as it is, whatever the weights.  The slot's deferred-weight
 *   word becomes 0: every weight now stored is a true weight.  fp32 add and multiply commute, so A merged with B equals B merged with A, bit for bit.
 *   Refused with nothing touched, as kf_write_brick_store -- KF_ERR_ARG: a NULL context; with count > 0, NULL keys, tsdf or weight, a translated key
 *   component out of range, a key that occurs twice in the call (count == 0 does nothing and looks at no array).  KF_ERR_STATE: no store reserved;
 *   `color` on a context without a colour plane.
 * kf_refill_window: re-reads the window from the store under its CURRENT origin -- the state kf_place_window(current origin) would leave if it did not
 *   capture the window first: the tail cull discarded, the flags serial bumped, the observed-voxel count re-based, the model maps stale, skip tables,
 *   has-negative bits, planes, flags and deferred-weight words cleared and every brick the store holds restored.  The pose and its inverse are not
 *   written at all, kf_volume_origin is unchanged, and the store is only read (its `restored` count grows by the hits).  This is how a merged store
 *   reaches the window: kf_place_window would capture the window's stale copy over the merged slots first.  A window brick the store does NOT hold
 *   reads as never observed afterwards: call kf_brick_store_capture first to keep such bricks.  Asynchronous, no allocation, no synchronisation.
 *   KF_ERR_ARG: a NULL context, a z-slab context, a brick of the window outside the key range.  KF_ERR_STATE: no store. */
int kf_merge_brick_store(kf_ctx* ctx, uint32_t count, const int32_t* keys, const float* tsdf, const float* weight, const uint8_t* color,
                         const int32_t offset_brick[3]);
int kf_refill_window(kf_ctx* ctx);

/* Merging maps under a rigid transform: the incoming (source) map is resampled at the destination's voxel centres, then merged as above.
 * Coordinates are world voxel indices: voxel g (brick key g >> 3, in-brick g & 7) has its centre at (g + 1/2) * cell.  xf is a row-major 3x4 [R | t], source
 * world -> destination world, t in voxels: destination voxel d lies at s = R^T (d + 1/2 - t) - 1/2 in the source.  A VALID transform: all 12 values finite,
 * max |R^T R - I| <= 1e-5 (a rotation stored in fp32 is orthonormal to a few 1e-7; the rest is room for a pose accumulated over a sequence), det R > 0.
 * kf_rigid_brick_keys (no context, host only): the candidate destination bricks of a source map.  For every source brick k the 8 corners p of the box
 *   [8k - 1, 8k + 8]^3 (the positions s whose corners floor(s), floor(s) + 1 can touch the brick) are mapped by
 *   d_i = (((R[i][0] (p_0 + 1/2) + R[i][1] (p_1 + 1/2)) + R[i][2] (p_2 + 1/2)) + t_i) - 1/2 in fp64; every destination brick (>> 3) that the box
 *   floor(min d) .. ceil(max d) touches is a candidate.  Unique, sorted by (z, y, x).  Returns the number of candidates and writes the first `cap` keys
 *   (three int32 each); -1: NULL keys with count > 0, NULL xf, NULL out_keys with cap > 0, an invalid transform, a candidate outside the key range
 *   [-2^20, 2^20).  A candidate too many is harmless: it resamples to nothing and takes no slot.
 * kf_merge_brick_store_rigid: kf_read_brick_store's layout for the source map (count entries: keys, tsdf, weight, colour bytes or NULL).  Blocks.
 *   Per candidate brick K, in fp64 on the host:  a = 8 K + 0.5 - t;  c_j = ((R[0][j] a_0 + R[1][j] a_1) + R[2][j] a_2) - 0.5;  ib = floor(c) (int32);
 *     fb = (float)(c - ib), and an fb that rounds to 1.0f becomes ib + 1, 0.f.
 *   Per voxel l in [0, 8)^3 of the brick, in fp32, one rounded operation per operation written here, Rf = (float)R:
 *     u_j = ((Rf[0][j] lx + Rf[1][j] ly) + Rf[2][j] lz) + fb_j;  n_j = floorf(u_j);  f_j = u_j - n_j;  base corner i_j = ib_j + (int)n_j.
 *   Corners: i + {0, 1}^3, the +1 neighbour on axis j used only when f_j > 0.  A corner is OBSERVED when the source holds its brick and its weight is > 0.
 *   One used corner unobserved: the voxel is unobserved -- tsdf 0, weight 0, colour 0 -- and takes part in nothing.  Otherwise
 *     tsdf:   lerp(a, b, f) = a + f * (b - a) along x, then y, then z; on an axis with f_j == 0 no lerp is applied: the value passes verbatim, -0.0 included
 *     weight: the minimum of the used corners' weights (exact): a resampled voxel is never trusted more than its least observed contributor
 *     colour: per channel the same lerps on the (float) bytes, then (unsigned char)fminf(255.f, v + 0.5f)
 *   Hence R = I with an integral t copies every voxel verbatim (every f is 0), a t of whole bricks is kf_merge_brick_store with that offset_brick wherever
 *   the source's unobserved voxels hold tsdf 0 and colour 0, and a signed permutation matrix with an integral t re-indexes voxels exactly.
 *   The resampled brick b then meets the held brick a under kf_merge_brick_store's rule, word for word: a brick with no resampled weight > 0 takes no slot
 *   and changes none; a key not held claims a slot and is written as kf_write_brick_store writes it (dropped when the store is full); a key held is
 *   merged per voxel with the held TRUE weight and its deferred-weight word becomes 0; with `color` NULL on a context with a colour plane a fresh slot's
 *   colour is 0 and a held one's stays; a key inside the current window is shadowed (kf_refill_window).
 *   Unlike the chunked write the whole source goes to the device at once -- the three planes, an open-addressing table over its keys (kf_brick_key_hash,
 *   the store's probe rule), key / ib / fb per candidate --, in temporary allocations freed before the call returns: a destination brick draws on up to 27
 *   source bricks, so chunks would need halos.
 *   Refused with nothing touched -- KF_ERR_ARG: a NULL context; with count > 0, NULL keys, tsdf, weight or xf, an invalid transform, a key component out of
 *   range, a key twice, a candidate brick outside the key range (count == 0 does nothing and looks at no array).  KF_ERR_STATE: no store reserved; `color`
 *   on a context without a colour plane.  KF_ERR_ALLOC: the temporaries do not fit. */
int64_t kf_rigid_brick_keys(uint32_t count, const int32_t* keys, const double xf[12], int32_t* out_keys, int64_t cap);
int kf_merge_brick_store_rigid(kf_ctx* ctx, uint32_t count, const int32_t* keys, const float* tsdf, const float* weight, const uint8_t* color,
                               const double xf[12]);

/* Halving a map's resolution: an incoming (source) map at voxel size s becomes a map at voxel size 2 s, which is merged into the store as above.  The TSDF
 * is stored normalised by the metric truncation distance, so the halved map is a valid TSDF for a context of the same size, the same truncation and half the
 * resolution; the call itself never looks at the context's resolution.  Coordinates are world voxel indices: coarse voxel g covers the eight fine voxels
 * 2 g + d, d in {0, 1}^3, and its centre (2 g + 1) s is the mean of their centres.  Hence coarse brick K draws on the source bricks 2 K + {0, 1}^3.
 * kf_halved_brick_keys (no context, host only): the coarse bricks of a source map, K_j >> 1 per component with the arithmetic shift (-1 gives -1, -3 gives
 *   -2).  Unique, sorted by (z, y, x).  Returns their number and writes the first `cap` keys (three int32 each); -1: NULL keys with count > 0, NULL out_keys
 *   with cap > 0, a key component outside [-2^20, 2^20).
 * kf_merge_brick_store_halved: kf_read_brick_store's layout for the source map (count entries: keys, tsdf, weight, colour bytes or NULL).  Blocks.
 *   Per coarse voxel, its children indexed i = dx | dy << 1 | dz << 2.  A child is OBSERVED when the source holds its brick and its weight is > 0.
 *   n = the number of observed children.  n == 0: the voxel is unobserved -- tsdf 0, weight 0, colour 0.  Otherwise, in fp32, one rounded operation per
 *   operation written here, the division correctly rounded, c_i = the child's tsdf, or 0.f when the child is unobserved:
 *     tsdf:   sum = ((c0 + c1) + (c2 + c3)) + ((c4 + c5) + (c6 + c7));  tsdf = sum / (float)n
 *     weight: the minimum of the observed children's weights (exact): a halved voxel is never trusted more than its least observed child
 *     colour: per channel (2 * S + n) / (2 * n) in integers, S = the sum of the observed children's bytes (their mean, rounded half up)
 *   Hence eight observed children of one value v give v exactly when 8 v does not overflow, -0.0 included, and eight observed values that are linear in the
 *   position, with every partial sum exact, give the same linear function at the coarse centre.
 *   The halved brick b then meets the held brick a under kf_merge_brick_store's rule, word for word: a brick with no halved weight > 0 takes no slot and
 *   changes none; a key not held claims a slot and is written as kf_write_brick_store writes it (dropped when the store is full); a key held is merged per
 *   voxel with the held TRUE weight and its deferred-weight word becomes 0; with `color` NULL on a context with a colour plane a fresh slot's colour is 0 and
 *   a held one's stays; a key inside the current window is shadowed (kf_refill_window).
 *   As the rigid merge, the whole source goes to the device at once -- the three planes, an open-addressing table over its keys, the coarse keys --, in
 *   temporary allocations freed before the call returns: a coarse brick draws on up to 8 source bricks, so the call cannot be chunked.  The window, the pose,
 *   the model maps and the triangle buffer stay bit for bit.
 *   Refused with nothing touched -- KF_ERR_ARG: a NULL context; a z-slab context; with count > 0, NULL keys, tsdf or weight, a key component out of range,
 *   a key twice (count == 0 does nothing and looks at no array).  KF_ERR_STATE: no store reserved; `color` on a context without a colour plane.
 *   KF_ERR_ALLOC: the temporaries do not fit. */
int64_t kf_halved_brick_keys(uint32_t count, const int32_t* keys, int32_t* out_keys, int64_t cap);
int kf_merge_brick_store_halved(kf_ctx* ctx, uint32_t count, const int32_t* keys, const float* tsdf, const float* weight, const uint8_t* color);

/* Erasing from the map: a box of voxels cleared in the store, or everything but the box; bricks that were hardly ever observed thrown out.  Emptied bricks
 * leave the store and their slots are handed out again (no reference counterpart).  All on the device: no brick crosses the bus.
 * Coordinates are world voxel indices: voxel g lies in the brick with key g >> 3 (arithmetic shift: negative coordinates floor) at in-brick position g & 7.
 * The box is half-open, lo_vox <= g < hi_vox on every axis, and is clamped to the key range [-2^23, 2^23] first, so any int32 box is legal.  An axis with
 * lo >= hi makes the box empty.
 * kf_brick_store_erase_box: mode KF_ERASE_INSIDE clears every voxel inside the box, KF_ERASE_OUTSIDE every voxel outside it (the map cropped to the box).
 *   A cleared voxel is (tsdf, weight) = (+0.0f, +0.0f) with colour bytes 0 0 0 0: what kf_reset_volume leaves.  Per held brick, from its key alone:
 *     no voxel to clear:   the brick stays bit for bit, its deferred-weight word included;
 *     all 512 to clear:    the brick is removed;
 *     anything in between: the voxels are cleared, the others keep their tsdf, their colour and their TRUE weight (what kf_read_brick_store reports), and
 *                          the brick's deferred-weight word becomes 0 whether or not an observed voxel was hit; a brick with no weight > 0 left is removed.
 *   *bricks_removed: the bricks removed; *voxels_cleared: the cleared voxels whose true weight was > 0, those of removed bricks included.  Either may be NULL.
 * kf_brick_store_erase_weak: removes every brick whose greatest TRUE weight is < min_weight; every other brick stays bit for bit.  min_weight <= 0
 *   removes nothing.
 * After either call the store is what it would be had it never held the removed bricks: `held` is the number of bricks kept and entries [0, held) are
 *   dense (their order is unspecified, as ever, and changes), `dropped` and `restored` are unchanged, every kept key is found and every removed key misses,
 *   a freed slot is handed out again, kf_brick_store_bounds shrinks accordingly.  The table is rebuilt, not patched: emptying an entry in place would cut the
 *   probe chains that run through it.  The capacity stays (kf_brick_store_reserve).
 *   The window is not touched: a key inside the current window is shadowed by the window's copy, as after kf_write_brick_store.  To erase from the MAP:
 *   kf_brick_store_capture, the erase, kf_refill_window -- and a raycast before the next frame is tracked.  Triangles already streamed into the world soup
 *   (kf_set_stream_out) are not taken back.
 *   Blocking: one read of the counts sizes the launches, one read at the end returns the results.  The scratch (a few 32-bit words per slot) is the
 *   context's, allocated by the first call.
 *   Refused with nothing touched -- KF_ERR_ARG: a NULL context, a NULL lo_vox or hi_vox, a mode other than the two, a NaN min_weight, a z-slab context.
 *   KF_ERR_STATE: no store reserved. */
#define KF_ERASE_INSIDE 0
#define KF_ERASE_OUTSIDE 1
int kf_brick_store_erase_box(kf_ctx* ctx, const int32_t lo_vox[3], const int32_t hi_vox[3], int mode, uint32_t* bricks_removed, uint64_t* voxels_cleared);
int kf_brick_store_erase_weak(kf_ctx* ctx, float min_weight, uint32_t* bricks_removed);

/* Querying the map: distance, gradient, weight and colour at N points; the first surface crossing of N rays (no reference counterpart for the points; the
 * march is the reference's, raycastingVolume.cu:79-117).  The map is read where it lies -- no resolve table, no window move, no copy -- and nothing of the
 * context changes: volume, store, deferred-weight words, pose, model maps, scratch and every later frame are bit for bit what they would have been.
 * The map as a function of a world voxel g (integers, any sign), which lies in world brick g >> 3: a brick inside the window (kf_volume_origin) is the
 *   window's; else, with a store reserved that holds the key, the store's; else nobody holds it.  Weights are TRUE weights (the deferred-weight word applied,
 *   what kf_download_volume and kf_read_brick_store report).  A voxel whose true weight is not > 0, or that nobody holds, reads (tsdf 0, weight 0, colour 0).
 *   Without a store the window alone is the map.
 * Positions are fp64 in WORLD VOXEL units, voxel g's centre at g + 0.5: the first cube's frame (a map mesh vertex or a world metre divided by the cell).
 *   fp64, so that a map anywhere in the key range (+-2^23 voxels) is sampled with the same bits as the same map at the origin.
 * kf_map_sample: per axis u = p - 0.5 (fp64), n = floor(u), f = (float)(u - n) (the difference is exact: one rounding).  The eight voxels n + {0, 1}^3 are
 *   read, corner k with x from bit 0, y from bit 1, z from bit 2.  One of them reads weight 0: the point is unobserved, every output for it is 0.  Otherwise,
 *   with lerp(a, b, f) = a + f * (b - a) in fp32, one rounding per operation:
 *     a0..a3 = lerp(v[2i], v[2i+1], fx);  b0 = lerp(a0, a1, fy), b1 = lerp(a2, a3, fy);  tsdf = lerp(b0, b1, fz);
 *     grad.x = lerp(lerp(v1-v0, v3-v2, fy), lerp(v5-v4, v7-v6, fy), fz);  grad.y = lerp(a1-a0, a3-a2, fz);  grad.z = b1 - b0   (tsdf units per voxel);
 *     weight = the least of the eight;  colour = kf_render_view's interpolateColor: corner j (x from bit 2, y from bit 1, z from bit 0) adds
 *     (float)c * wa * wb * wc in the order j = 0..7, wa = f or 1 - f, the sum truncated; byte 3 is 0.  Colour is 0 on a context without a colour plane.
 *   There is no |tsdf| < 1 rule: the caller sees the value.  A position that is not finite or lies outside [-2^23, 2^23] reads unobserved.
 * kf_map_cast_rays: ray i is origin (fp64, world voxels), dir (3 x fp32, used as given: t is in units of |dir| voxels), t_min and t_max.  Sample k is at
 *   t_k = t_min + (float)k * step, per axis at origin + (double)(t_k * dir): the product in fp32, the sum in fp64.  s_k = the tsdf of the voxel floor(p).
 *   last = 0; while t_k < t_max and k < max_steps: if last > 0 and s_k < 0 refine and stop, else last = s_k.  Refinement: ft, ftdt = kf_map_sample's tsdf at
 *   samples k - 1 and k (either unobserved: BROKEN); alpha = t_k - step * ftdt / (ftdt - ft), the division correctly rounded; the hit is kf_map_sample at
 *   origin + (double)(alpha * dir); len = sqrtf((gx * gx + gy * gy) + gz * gz); the hit unobserved or not len >= 1e-8f: BROKEN; else HIT with t = alpha,
 *   normal = grad / len (towards growing tsdf: out of the surface), the hit's colour and weight.  status: KF_RAY_MISS, KF_RAY_HIT or KF_RAY_BROKEN (the
 *   reference's `break` without output); a ray that is not a HIT writes zeros.
 * The _device forms take device pointers, run on the context's stream and do not block; the others take host pointers: one temporary allocation, copies, and
 *   they block.  Any output pointer may be NULL.  n == 0 does nothing.  pos / origin: 3 per item; grad / normal / dir: 3 per item; color: 4 bytes per item.
 * Refused with nothing written -- KF_ERR_ARG: a NULL context, a NULL input array, step not finite or not > 0, max_steps 0 or > 2^24.  KF_ERR_STATE: a z-slab
 *   context (slab groups have no store and hold part of a window each). */
#define KF_RAY_MISS 0
#define KF_RAY_HIT 1
#define KF_RAY_BROKEN 2
int kf_map_sample_device(kf_ctx* ctx, uint32_t n, const double* dev_pos, float* dev_tsdf, float* dev_weight, float* dev_grad, uint8_t* dev_color);
int kf_map_sample(kf_ctx* ctx, uint32_t n, const double* pos, float* tsdf, float* weight, float* grad, uint8_t* color);
int kf_map_cast_rays_device(kf_ctx* ctx, uint32_t n, const double* dev_origin, const float* dev_dir, const float* dev_tmin, const float* dev_tmax, float step, uint32_t max_steps, uint8_t* dev_status, float* dev_t, float* dev_normal, uint8_t* dev_color, float* dev_weight);
int kf_map_cast_rays(kf_ctx* ctx, uint32_t n, const double* origin, const float* dir, const float* tmin, const float* tmax, float step, uint32_t max_steps, uint8_t* status, float* t, float* normal, uint8_t* color, float* weight);

/* Relocalising a frame in the map: many candidate camera poses of one point set scored against the map, and the best few refined by Gauss-Newton on the
 * map's distance at the points (no reference counterpart: the reference blocks on a key press when the camera is lost).  The map, its weights and the sample
 * are those written above kf_map_sample; nothing of the context changes: volume, store, deferred-weight words, pose, model maps, scratch and every later
 * frame are bit for bit what they would have been.  Colour plays no part.
 * Points: 3 x fp32 per point, in the CAMERA frame, in voxel units (metres / cell), used as given.  Poses: 12 x fp64 per pose, row-major [R | t], camera ->
 *   world voxels, t at entries 3, 7 and 11 as in kf_align_step's xf.  Poses are NOT checked for being rigid.
 * Position of point (x, y, z) under a pose, per axis j, all in fp64 with one rounding per operation:
 *     w_j = ((R[j][0] * (double)x + R[j][1] * (double)y) + R[j][2] * (double)z) + t[j].
 * kf_map_score_poses: per pose five integers over the points.  The value at w is kf_map_sample's tsdf -- the same bits, the same observed rule (all eight
 *   corners with TRUE weight > 0; a w that is not finite or lies outside +-2^23 reads unobserved).  An observed point, with a = fabsf(tsdf): counts in
 *   n_obs; a < band: n_in; otherwise tsdf < 0: n_behind (the point lies inside an object); otherwise n_free (it floats in observed free space);
 *   sum_q += (uint32_t)(fminf(a, 1.f) * 65536.f) (the product is exact, the conversion truncates: at most 65536 per point).  n_obs = n_in + n_behind + n_free.
 *   Integers, because integer addition commutes: the bytes do not depend on the grid, the chunking or the order in which workgroups arrive, so no fold order
 *   has to be fixed and any pose count fills the chip.  A pose with a NaN in it scores all zeros.
 *   The _device form takes device pointers, runs on the context's stream (it zeroes dev_scores there first) and does not block; the other takes host
 *   pointers: one temporary allocation, copies, and it blocks.
 *   Refused with nothing written -- KF_ERR_ARG: a NULL context, points, poses or scores; n_points 0 or > 2^24; n_poses 0 or > 2^20; band not finite, not > 0
 *   or > 1.  KF_ERR_STATE: a z-slab context.  KF_ERR_ALLOC: the host form's temporary does not fit.
 * kf_map_pose_sums: the 29 sums of kf_align_brick_store's layout for each of n_poses (at most 4096) poses, one launch.  Point i under pose k: w as above; phi
 *   and g = kf_map_sample's tsdf and grad at w; the point takes part when it is observed and fabsf(phi) < gate, gate in (0, 1];
 *   x_j = (float)(w_j - centre_k[j]), the difference in fp64;  J = (x_1 g_2 - x_2 g_1, x_2 g_0 - x_0 g_2, x_0 g_1 - x_1 g_0, g_0, g_1, g_2), every product and
 *   difference rounded once, in fp32;  e = -phi.  Sums per pose: [0, 21) the upper triangle of sum J_a J_b row by row, [21, 27) sum J_a e, [27] sum e e,
 *   [28] the number of points that took part, counted in integers; every product is formed in fp64 from its fp32 factors, hence exact.
 *   kf_align_step(sums, centre, pose, step) applies to them unchanged: under a left twist xi = (omega, v) about the centre, pose <- T(c) exp(xi) T(-c) pose,
 *   a point moves by omega x (w - c) + v, so d phi = g . (omega x x + v) = J . xi and e' = e - J . xi: the step solves (sum J J^T) xi = sum J e.
 *   The fold is fixed, so the same inputs give the same 29 doubles bit for bit on every run and in every context: with G = min(ceil(n_points / 256), 64),
 *   point i belongs to workgroup (i / 256) % G of its pose, lane i % 256; a lane adds its points in ascending order; the wave's lanes fold by the butterfly
 *   xor 32 .. 1; the four waves as ((w0 + w1) + w2) + w3; the G rows are added in ascending order.  No atomic on a float anywhere.
 * kf_map_refine_poses: kf_align_brick_store's loop, per pose: evaluate the sums; KF_ALIGN_FEW_PAIRS when fewer than max(min_pairs, 1) points took part;
 *   KF_ALIGN_ITER_LIMIT when max_iter steps are done; a kf_align_step, KF_ALIGN_SINGULAR when it refuses; KF_ALIGN_CONVERGED when the step has |omega| <=
 *   eps_rot and |v| <= eps_trans (the stepped pose is the result; it is not evaluated again).  An eps below KF_ALIGN_EPS_ROT_MIN / KF_ALIGN_EPS_TRANS_MIN is
 *   raised to it: the sample's fraction is fp32 here too.  The stepped pose is not checked for being rigid (the poses that go in are not either).  All the
 *   poses still running are evaluated in one launch per iteration, with one read-back of 29 doubles per running pose; a pose's result does not depend on
 *   what else is in the batch.  poses is in / out.  On FEW_PAIRS and SINGULAR a pose is the last one evaluated with enough pairs (the guess, if none).
 *   max_iter == 0 evaluates the sums, reports them (KF_ALIGN_ITER_LIMIT) and leaves the poses alone.  reports: one per pose, as kf_align_brick_store's.
 *   centres: 3 x fp64 per pose, world voxels: the point rotations are taken about -- the middle of the points under the pose keeps sum J J^T well conditioned.
 *   Both calls take host pointers and block.  Refused with nothing written -- as kf_map_score_poses (n_poses > 4096; gate in place of band), and KF_ERR_ARG
 *   for a NULL centres, sums, params or reports, an eps that is negative or not finite, a centre or pose entry that is not finite. */
typedef struct kf_pose_score { uint32_t n_obs, n_in, n_behind, n_free; uint64_t sum_q; } kf_pose_score;   /* 24 bytes */
typedef struct kf_refine_params { uint32_t max_iter, min_pairs; double eps_rot, eps_trans; float gate; } kf_refine_params;
struct kf_align_report;
int kf_map_score_poses_device(kf_ctx* ctx, uint32_t n_points, const float* dev_points, uint32_t n_poses, const double* dev_poses, float band, kf_pose_score* dev_scores);
int kf_map_score_poses(kf_ctx* ctx, uint32_t n_points, const float* points, uint32_t n_poses, const double* poses, float band, kf_pose_score* scores);
int kf_map_pose_sums(kf_ctx* ctx, uint32_t n_points, const float* points, uint32_t n_poses, const double* poses, const double* centres, float gate, double* sums);
int kf_map_refine_poses(kf_ctx* ctx, uint32_t n_points, const float* points, uint32_t n_poses, double* poses, const double* centres, const kf_refine_params* params, struct kf_align_report* reports);

/* The distance field of the map: for every voxel of a box the exact squared Euclidean distance, in voxels, to the nearest SITE of the map, up to a radius --
 * the clearance a planner asks for beyond the truncation band (no reference counterpart).
 * The map as a function of a world voxel g is the one written above kf_map_sample: the window's copy where the voxel's brick is inside the window, else the
 *   store's, else nobody holds it; weights are TRUE weights; without a store the window alone is the map.  A voxel whose brick coordinate lies outside the
 *   key range [-2^20, 2^20) is held by nobody.
 * The class of a voxel, one byte: KF_VOX_UNKNOWN -- the true weight is not > 0, or nobody holds the voxel; KF_VOX_FREE -- observed and tsdf > level;
 *   KF_VOX_OCCUPIED -- observed and tsdf <= level.  level is in tsdf units: 0 means at or behind the surface, a small positive level inflates obstacles.
 * The sites are the voxels whose class has its bit set in site_mask (bit c = class c, the mask in 1 .. 7): 1 << KF_VOX_OCCUPIED is the obstacle field; or-ing
 *   in 1 << KF_VOX_UNKNOWN treats unknown space as an obstacle; (1 << KF_VOX_FREE) | (1 << KF_VOX_UNKNOWN) is the depth inside obstacles -- a signed field is
 *   two calls.
 * The field: for every voxel g of the box, d2(g) = the minimum of |s - g|^2 over ALL sites s of the map, not only those in the box.  Coordinates are integer
 *   voxel indices, the squared distance is an integer.  The output is d2 where d2 <= radius^2, else KF_EDT_FAR.  radius is in voxels, 1 .. 255 (255^2 = 65025
 *   fits 16 bits below the sentinel).  A site reads 0.  Two guarantees follow:
 *   - the field of a box is the same bytes as the corresponding part of the field of any box that encloses it (so a caller may tile);
 *   - the field does not depend on where the window stands or on which of window and store holds a brick, once captured.
 * The box: lo_vox (world voxels, any sign, need not be brick-aligned) and dims (each >= 1); the outputs are indexed (z * ny + y) * nx + x.  The box itself must
 *   lie inside [-2^23, 2^23) on every axis; the `radius` voxels around it that are searched may reach outside, where they read unknown.
 * dist2: 16 bits per voxel; cls: the class byte per voxel.  Either may be NULL, independently (both NULL: nothing is done).  lo_vox and dims are host pointers
 *   in both forms.  The _device form takes device output pointers, runs on the context's stream and does not block -- except that a call whose box needs more
 *   scratch than any before it waits for the stream before it frees the smaller one; the other form takes host pointers: one temporary allocation, copies, and
 *   it blocks.  The scratch (one site bit per voxel of the box widened by radius, rounded out to bricks, and 16 bits for each of nx (ny + 2 radius) (nz + 2 radius)
 *   + nx ny (nz + 2 radius) voxels) is the context's own, allocated or grown by the first call that needs it and freed with the context; it is not the extraction
 *   scratch.  The classes alone (dist2 NULL) need none.
 * Nothing of the context changes: volume, store, deferred-weight words, pose, model maps, extraction scratch and every later frame are bit for bit what they
 *   would have been.
 * Refused with nothing written -- KF_ERR_ARG: a NULL context, lo_vox or dims; a zero dimension; a box that does not lie inside [-2^23, 2^23); radius 0 or > 255;
 *   site_mask 0 or > 7; a NaN level; nx * (ny + 2 radius) * (nz + 2 radius) > 2^29 (the bound on the two 16-bit buffers, 2 GiB together at the most: a larger
 *   box is tiled by the caller, which the first guarantee makes exact).  KF_ERR_STATE: a z-slab context.  KF_ERR_ALLOC: no memory for the scratch.  The cap does
 *   NOT bound the bit volume, which is widened in x too: about (nx + 2 radius) / 8 bytes per row of (ny + 2 radius) (nz + 2 radius) -- a sixteenth of the x pass's
 *   buffer for a box much wider than its radius, but 511 / 8 bytes per row, some 34 GB at the cap, for nx = 1 at radius 255.  KF_ERR_ALLOC is the only guard
 *   there: keep a box's x edge at least comparable to the radius (lanes run along x in every pass, so a narrow box is slow as well). */
#define KF_VOX_UNKNOWN 0
#define KF_VOX_FREE 1
#define KF_VOX_OCCUPIED 2
#define KF_EDT_FAR 0xFFFFu
int kf_map_distance_field_device(kf_ctx* ctx, const int32_t lo_vox[3], const uint32_t dims[3], uint32_t radius, float level, uint32_t site_mask, uint16_t* dev_dist2, uint8_t* dev_cls);
int kf_map_distance_field(kf_ctx* ctx, const int32_t lo_vox[3], const uint32_t dims[3], uint32_t radius, float level, uint32_t site_mask, uint16_t* dist2, uint8_t* cls);

/* Aligning two maps: the rigid transform kf_merge_brick_store_rigid needs, found by Gauss-Newton on the SDF-to-SDF error between the store and an incoming
 * map (no reference counterpart).  A REFINEMENT, not a global search: its basin is about the truncation band -- on an analytic box with a band of four
 * voxels a start 10 degrees and about 5 voxels off still converges; a start much further off finds too few pairs or a wrong minimum.  Coarse-to-fine search
 * and global alignment of two maps are not offered (for a depth FRAME against the map, see kf_map_score_poses: a lattice of poses scored, the best refined).
 * The destination is the brick store as held (read only): a key inside the current window is shadowed by the window's copy, so call
 * kf_brick_store_capture first.  The source is an incoming map in kf_read_brick_store's layout (count entries: keys, tsdf, weight).  xf is the rigid
 * merge's [R | t]: row-major 3x4, source world -> destination world, t in voxels, VALID as defined above.  Colour plays no part.
 * One evaluation: for every held slot with key K and every voxel l in [0, 8)^3 of it --
 *   Held side: with the STORED pair (td, wd) the voxel takes part only when wd > 0 and fabsf(td) < 1.f.  The slot's deferred-weight word is not looked
 *     at: a quarter of a brick whose weights are still deferred holds tsdf 1.0 throughout, which the band excludes.
 *   Source position, the rigid merge's arithmetic: ib, fb per brick by its fp64 formula (a = 8 K + 0.5 - t; c_j = ((R[0][j] a_0 + R[1][j] a_1) +
 *     R[2][j] a_2) - 0.5; ib = floor(c); fb = (float)(c - ib), an fb of 1.0f becoming ib + 1, 0.f; a brick whose ib does not fit 31 bits takes no part);
 *     in fp32, Rf = (float)R, one rounded operation per operation written here:
 *     u_j = ((Rf[0][j] lx + Rf[1][j] ly) + Rf[2][j] lz) + fb_j;  n_j = floorf(u_j);  f_j = u_j - n_j;  base corner i_j = ib_j + (int)n_j.
 *   Corners: all eight i + {0, 1}^3 are read, whatever f is.  Each must be held by the source with weight > 0 and fabsf(tsdf) < 1.f, otherwise the voxel
 *     takes no part: a corner at the truncation value has no gradient to give.  v[dx | dy << 1 | dz << 2] their tsdf values.
 *   Value, lerp(a, b, f) = a + f * (b - a) always applied:  a_k = lerp(v[2k], v[2k+1], f_x), k = 0..3;  b_0 = lerp(a_0, a_1, f_y), b_1 = lerp(a_2, a_3, f_y);
 *     phi = lerp(b_0, b_1, f_z).
 *   Gradient in source voxels, from the same eight values:  dx_k = v[2k+1] - v[2k];  gx = lerp(lerp(dx_0, dx_1, f_y), lerp(dx_2, dx_3, f_y), f_z);
 *     gy = lerp(a_1 - a_0, a_3 - a_2, f_z);  gz = b_1 - b_0.
 *   Row:  gd_i = (Rf[i][0] gx + Rf[i][1] gy) + Rf[i][2] gz;  x_j = (float)(8 K_j + 0.5 - centre_j) + l_j, the bracket in fp64;
 *     J = (x_1 gd_2 - x_2 gd_1, x_2 gd_0 - x_0 gd_2, x_0 gd_1 - x_1 gd_0, gd_0, gd_1, gd_2), every product and difference rounded once;  e = phi - td.
 *   Sums, 29 doubles:  [0, 21) the upper triangle of sum J_a J_b row by row ((0,0), (0,1) .. (0,5), (1,1) .. (5,5));  [21, 27) sum J_a e;  [27] sum e e;
 *     [28] the number of voxels that took part, counted in integers.  Every product is formed in fp64 from its fp32 factors, hence exact, and added in fp64
 *     in an order that depends on the keys held alone (the slots are visited by ascending packed key, whichever slot a brick claimed): no atomic on a
 *     float, so the same map in the store and the same source give the same 29 doubles bit for bit on every run and in every context.
 * kf_align_step (no context, host only): one step from the sums.  Solves (sum J J^T) xi = sum J e by Cholesky, xi = (omega, v): omega a rotation vector
 *   in radians about `centre`, v in voxels.  Updates xf <- T(centre) exp(xi) T(-centre) xf: with E = exp(omega^) and V = I + (1 - cos th) / th^2 omega^ +
 *   (th - sin th) / th^3 omega^2, th = |omega|,  R <- E R and t <- E (t - centre) + centre + V v.  All in fp64.  Returns 0 and writes xf and step[6] = xi;
 *   non-zero with both untouched for a NULL pointer, a pivot <= 0 (the sums do not determine all six unknowns) or a result that is not finite.
 * kf_align_brick_store: uploads the source once (the two planes and an open-addressing table over its keys, in temporary allocations freed before the
 *   call returns), then repeats: evaluate the sums at xf; stop with KF_ALIGN_FEW_PAIRS when fewer than max(min_pairs, 1) voxels took part; stop with
 *   KF_ALIGN_ITER_LIMIT when max_iter steps are done; take a kf_align_step, stopping with KF_ALIGN_SINGULAR when it refuses; stop with KF_ALIGN_CONVERGED
 *   when the step has |omega| <= eps_rot and |v| <= eps_trans (the stepped transform is the result; it is not evaluated again).  An eps_rot below
 *   KF_ALIGN_EPS_ROT_MIN (2^-23 rad: one unit in the last place of an entry of Rf) or an eps_trans below KF_ALIGN_EPS_TRANS_MIN (2^-18 voxels: the
 *   granularity of a position u, a few units in the last place of a value in [8, 16)) is raised to it.  The rule evaluates Rf and fb, not R and t: below
 *   that resolution the sums change by rounding alone, and the steps of an fp64 Gauss-Newton loop, which would fall to 1e-13, here stay at some 1e-9 rad
 *   and 1e-8 voxels for ever (measured on the analytic box of the tests), four to five orders below the error of the result itself.  xf is in / out: the guess
 *   goes in, the result comes out.  On FEW_PAIRS and SINGULAR xf is the last transform that was evaluated with enough pairs (the guess, if none).
 *   max_iter == 0 evaluates the sums at xf, reports them (KF_ALIGN_ITER_LIMIT) and leaves xf alone.  centre, in voxels (voxel g has its centre at g + 1/2), is
 *   the point rotations are taken about: the middle of the map keeps sum J J^T well conditioned.  The report: the steps taken, the verdict, the LAST
 *   evaluation's sums and rms = sqrt(sums[27] / sums[28]) (0 without a pair), the last step taken (zeros if none).  Blocks.
 *   The call changes nothing: the store (slots, table, counts, deferred-weight words), the window, the pose, the model maps and the triangle buffer stay
 *   bit for bit.  Refused with nothing touched, xf and the report included -- KF_ERR_ARG: a NULL context, xf, params or report; with count > 0, NULL keys,
 *   tsdf or weight; an invalid transform; a key component out of range, a key twice; an eps that is negative or not finite, a centre that is not finite; a
 *   z-slab context.  KF_ERR_STATE: no store reserved.  KF_ERR_ALLOC: the temporaries do not fit. */
#define KF_ALIGN_EPS_ROT_MIN 1.1920928955078125e-07     /* 2^-23 rad */
#define KF_ALIGN_EPS_TRANS_MIN 3.814697265625e-06       /* 2^-18 voxels */
#define KF_ALIGN_CONVERGED 0
#define KF_ALIGN_ITER_LIMIT 1
#define KF_ALIGN_FEW_PAIRS 2
#define KF_ALIGN_SINGULAR 3
typedef struct kf_align_params { uint32_t max_iter, min_pairs; double eps_rot, eps_trans; double centre[3]; } kf_align_params;
typedef struct kf_align_report { uint32_t iterations, verdict; double sums[29]; double rms; double step[6]; } kf_align_report;
int kf_align_step(const double sums[29], const double centre[3], double xf[12], double step[6]);
int kf_align_brick_store(kf_ctx* ctx, uint32_t count, const int32_t* keys, const float* tsdf, const float* weight, double xf[12],
                         const kf_align_params* params, kf_align_report* report);

/* The map mesh: marching cubes over the brick store and the window together (no reference counterpart: the reference's one cube is its map).
 * kf_marching_cubes_at: kf_marching_cubes_region in a VIRTUAL window.  Emits exactly the triangles -- the same bytes in the same order, appended to the
 *   triangle buffer and clamped the same way -- that kf_marching_cubes_region(ctx, has_color, threshold, lo, hi, flags) would emit after
 *   kf_shift_volume(frame_origin_vox - current origin) on this context, the store's bricks restored, WITHOUT moving anything: volume, flags, skip tables,
 *   pose, model maps, store, deferred-weight words and every later frame are bit for bit what they are without the call.  lo / hi are cell indices in the
 *   virtual window, [0, resolution), clamped, with the region call's rim rule; an empty or inverted box is a no-op.  flags: KF_MC_WORLD or 0; with
 *   KF_MC_WORLD every position component i gets + (float)frame_origin_vox[i] * cell (the region call's world rule with the frame's origin in place of the
 *   window's).  Where a brick of the virtual window comes from: world brick frame_origin_vox / 8 + b reads the WINDOW's copy if it lies inside the current
 *   window (the newer one: a restored brick stays in the store as a stale copy, which must not win), otherwise the STORE's entry if its key is held
 *   (read-only), otherwise it was never observed.  With frame_origin_vox == the current origin the call is kf_marching_cubes_region.  No store reserved
 *   is not an error: bricks outside the window read as never observed.  Asynchronous on the context's stream: no synchronisation, no read-back; the first
 *   call allocates one indirection table (16 bytes per brick of the window, plus one 4 KiB zero brick) with the extraction scratch.  kf_region_work
 *   reports the call's work: out[0] bricks whose voxels were classified, out[1] blocks listed.
 *   KF_ERR_ARG, with nothing touched: a NULL context, origin or box; a frame origin component that is no multiple of 8; flag bits other than KF_MC_WORLD;
 *   a z-slab context; a frame any of whose bricks has a world brick coordinate outside [-2^20, 2^20).  KF_ERR_STATE: no triangle buffer, or has_color
 *   without a colour plane.
 * kf_marching_cubes_map: one mesh of everything ever fused, in world coordinates (KF_MC_WORLD is forced on; flags takes KF_MC_WORLD or 0), appended to the
 *   triangle buffer.  Space is tiled on a lattice fixed in the WORLD: with T = resolution - 16, tile k of an axis is the frame F_k = k * T - 8 voxels and owns
 *   the frame's local cells [8, resolution - 8), i.e. the world cells [k * T, (k + 1) * T).  Owned boxes are disjoint and cover space, and every owned
 *   cell lies eight cells inside its frame, so no cell is lost to the rim rule and none is emitted twice.  The tiles visited are those whose frame meets
 *   kf_brick_store_bounds' box or the window's bricks, in z, then y, then x order, ascending; each is one kf_marching_cubes_at over its owned box.
 *   *n_tiles (may be NULL): tiles visited.  Because the lattice does not depend on where the window stands, the map mesh is the same bytes wherever the
 *   window is, as long as no frame was fused in between and the store dropped nothing (kf_brick_store_count's `dropped`: a dropped brick is a hole).
 *   Blocks once (the store's bounds), then enqueues.  Refusals as for kf_marching_cubes_at, and KF_ERR_ARG for a resolution below 32.
 * kf_map_tile_frames: the lattice alone, on the host (no context): the frames (three voxel coordinates per tile, in visiting order) for a store box
 *   (bricks, half-open; lo == hi: none), a window origin and a resolution.  Writes the first `cap` tiles to `frames` (may be NULL with cap 0) and returns
 *   the number of tiles, or -1 for a NULL pointer or a resolution below 32 or no multiple of 8. */
int kf_marching_cubes_at(kf_ctx* ctx, int has_color, float threshold_marchingcube, const int32_t frame_origin_vox[3], const int32_t lo[3], const int32_t hi[3],
                         int flags);
int kf_marching_cubes_map(kf_ctx* ctx, int has_color, float threshold_marchingcube, int flags, uint32_t* n_tiles);
int64_t kf_map_tile_frames(const int32_t store_lo_brick[3], const int32_t store_hi_brick[3], const int32_t origin_vox[3], int32_t resolution, int32_t* frames,
                           int64_t cap);

/* test hook: counts fp32 quotients where the kernels' split exact-division helper differs from the compiler's `/` (must be 0) */
int kf_selftest_div(kf_ctx* ctx, unsigned n, unsigned seed, int mode, unsigned* mismatches);

/* Per-stage device timers (hipEvent pairs on the context's stream).  `stage_mask` bit s enables stage s:
 * 0 depth upload/convert, 1 preprocess, 2 track, 3 integrate (all passes), 4 raycast, 5 integrate fusion kernel only,
 * 6 marching cubes, 7 raycast kernel only.  Bits 8-15 of `stage_mask`, when > 1, are a sampling period N: only every N-th
 * interval of a stage is timed (fewer event records in a benchmark's timed region).  kf_stage_timers resets the accumulators; kf_read_stage_ms blocks and returns
 * accumulated milliseconds and the number of timed intervals per stage. */
int kf_stage_timers(kf_ctx* ctx, int stage_mask);
int kf_read_stage_ms(kf_ctx* ctx, float out_ms[8], uint32_t counts[8]);
/* Work counters for roofline accounting, maintained only while bit 16 of `stage_mask` is set (they cost a
 * few atomics per wave) and reset by kf_stage_timers: out[0] = voxel samples the reference's ray march takes (per ray from t_min
 * to its first crossing or t_max, src/cuda/raycastingVolume.cu:65-119), out[1] = rays whose crossing was evaluated,
 * out[2] = 4-KiB bricks the marching-cubes extractions read (those with a negative voxel in their 3x3x3 brick neighbourhood),
 * out[3] = triangles in the buffer.  Blocking. */
int kf_read_work_counters(kf_ctx* ctx, uint64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* HYBKF_H_ */
