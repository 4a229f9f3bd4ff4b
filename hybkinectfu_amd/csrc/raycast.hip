// raycast.hip -- surface prediction for the next frame's ICP (reference: raycastKernel / raySample / gradientForPoint /
// getMinTime / getMaxTime, src/cuda/raycastingVolume.cu:16-176; tsdfvolume::getVoxel(world), interpolateSDF,
// interpolateColor, src/cuda/tsdfVolume.h:81-172).
//
// gfx950 design (gather / latency bound):
//   * one lane per pixel, a wave covers an 8x8 pixel patch so its 64 rays stay spatially coherent through the volume;
//   * the reference gathers one 12-byte voxel per step (~106 dependent gathers per ray).  Here a step first reads the
//     1-byte flag of the 8^3 brick it lands in (a 256 KiB table at 512^3: L2 resident).  A brick that never held a
//     negative tsdf cannot contain the `sdf < 0` sample of a +/- crossing, so the voxel gather is skipped; the tsdf of
//     the previous sample is fetched lazily only when a negative sample is actually met.  The parameter t is still
//     advanced by the same repeated fp32 addition, so every sample position, the first crossing and all the
//     interpolation inputs are bit-identical to the reference march;
//   * bricks are 4 KiB contiguous, so the trilinear taps at the hit (2 + 6 lookups x 8 voxels) touch 1-2 bricks.
#include "kf_internal.h"
#include "bilateral_tile.h"
#include "grad_shared.h"
#include "view_pixel.h"
#include <string.h>
// the march of one ray tile and the placement of its LDS tables (RaycastArgs, rc_march, rc_tile_bounds, raycast_tile, raycast_args ...), with the default
// addressing hooks: the window's own voxels.  viewat.hip compiles the same file over a virtual window.
#include "raycast_tile.h"

__global__ void __launch_bounds__(RAYCAST_THREADS) k_raycast(RaycastArgs a) {
  extern __shared__ unsigned s_dyn[];
  raycast_tile<false>(a, (int)blockIdx.x, (int)blockIdx.y, s_dyn);
}
// kf_raycast_volume_slab_cross_spec_color: the crossing words, their second copy and 4 speculative words per pixel (normal, colour)
__global__ void __launch_bounds__(RAYCAST_THREADS) k_raycast_slab_color(RaycastArgs a) {
  extern __shared__ unsigned s_dyn[];
  raycast_tile<true>(a, (int)blockIdx.x, (int)blockIdx.y, s_dyn);
}

// kf_render_view: the caller's camera, one display word per pixel (mode = KF_VIEW_*: the epilogue is chosen at compile time)
template <int MODE>
__global__ void __launch_bounds__(RAYCAST_THREADS) k_raycast_view(RaycastArgs a, unsigned* img) {
  extern __shared__ unsigned s_dyn[];
  raycast_tile<false, MODE + 1>(a, (int)blockIdx.x, (int)blockIdx.y, s_dyn, img);
}

// kf_view_slab_cross: the z-slab march for the caller's camera (RC_VIEW_CROSS); COLOR: 4 speculative words per pixel
template <bool COLOR>
__global__ void __launch_bounds__(RAYCAST_THREADS) k_raycast_view_cross(RaycastArgs a) {
  extern __shared__ unsigned s_dyn[];
  raycast_tile<COLOR, RC_VIEW_CROSS>(a, (int)blockIdx.x, (int)blockIdx.y, s_dyn);
}

// The raycast with the NEXT frame's depth conversion + gate + bilateral filter riding along (kf_prefetch_frame, fused form).  The raycast
// lasts as long as its slowest waves while the average SIMD is busy for less than half of that; the filter of the frame that comes next
// depends on nothing this frame computes.  Workgroups [0, n_rc) are the raycast's tiles (dispatched first, higher wave priority), the rest
// filter two 64x4 tiles each (bilateral_tile.h) and fill the chip as the raycast drains -- no second stream, no events.
// behind == 1: the filter itself has run already (riders of the tracking launch, track.hip); what is left are the integrate tile tables, which
// may only be written now that the fusion pass has cleared them (one gated-depth read per pixel; b.acc.tile null: not wanted), and the frame's
// vertices + normals (out_v non-null), which then need no launch of their own.
// ... and with them levels 1 and 2 of their pyramids (pyr.v1 non-null): a 64x4 tile holds whole 2x2 and 4x4 blocks, so the riders need nothing
// from each other and the tracker's pyramid launch finds the new maps' pyramids done.
struct KfFrontTail { int behind; float4* out_v; float4* out_n; KfCam cam; KfPyrOut pyr; };
#define RIDER_LDS_BYTES (2 * (BIL_TX * BIL_TY + BIL_TX * BIL_TY / 4) * 2 * (int)sizeof(float4))      // per half: the tile's vertices + normals and their level 1
// (six waves per SIMD = three 8-wave workgroups per CU: all 600 ray tiles of a VGA frame resident at once, as in k_raycast -- the filter code would
// otherwise take 90 registers and push the last 88 tiles into a second round)
template <bool FAST>
__global__ void __launch_bounds__(RAYCAST_THREADS) __attribute__((amdgpu_waves_per_eu(6, 6))) k_raycast_prefetch(RaycastArgs a, KfBilateralArgs b, KfFrontTail ft, int rc_gx, int n_rc, int bil_gx, int bil_tiles) {
  extern __shared__ unsigned s_dyn[];
  if ((int)blockIdx.x < n_rc) {
    __builtin_amdgcn_s_setprio(2);
    raycast_tile<false>(a, (int)blockIdx.x % rc_gx, (int)blockIdx.x / rc_gx, s_dyn);
  } else {
    const int half = (int)(threadIdx.x >> 8), t = ((int)blockIdx.x - n_rc) * 2 + half, tid = (int)(threadIdx.x & 255);
    // a tile index past the last one names a row below the image: its threads touch nothing but still meet the barrier
    const int tt = t < bil_tiles ? t : bil_tiles;
    if (ft.behind) {
      kf_tiles_from_gated(b, tt % bil_gx, tt / bil_gx, tid);
      const int x0 = (tt % bil_gx) * BIL_TX, y0 = (tt / bil_gx) * BIL_TY, x = x0 + (tid & 63), y = y0 + (tid >> 6);
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f), n = v;
      if (ft.out_v && x < ft.cam.cols && y < ft.cam.rows) kf_vertex_normal_pixel(b.filtered, ft.out_v, ft.out_n, ft.cam, x, y, &v, &n);
      if (ft.pyr.v1) {                                                       // uniform
        float4* s_v = reinterpret_cast<float4*>(s_dyn) + half * (RIDER_LDS_BYTES / 2 / (int)sizeof(float4));
        float4* s_n = s_v + BIL_TX * BIL_TY, *s1_v = s_n + BIL_TX * BIL_TY, *s1_n = s1_v + BIL_TX * BIL_TY / 4;
        s_v[tid] = v; s_n[tid] = n;
        kf_tile_pyramid<BIL_TX, BIL_TY>(ft.pyr, x0, y0, tid, s_v, s_n, s1_v, s1_n, [] { __syncthreads(); });
      }
    } else kf_bilateral_tile<4, FAST>(b, tt % bil_gx, tt / bil_gx, tid, reinterpret_cast<float*>(s_dyn) + half * ((BIL_TX + 8) * (BIL_TY + 8)));
  }
}


// kf_prefetch_frame left a note: the next frame's u16 -> f32 + gate + bilateral rides in this launch (k_raycast_prefetch), its vertices /
// normals follow; the set lands in the alternate buffers and kf_preprocess adopts it when it is asked for exactly that frame
struct RaycastRiders { KfBilateralArgs b; KfFrontTail ft; bool fast, build_tiles; int bil_gx, bil_tiles; size_t lds; };
static void raycast_riders(kf_ctx* c, RaycastRiders& r) {
  c->fp_pending = 0;
  const int behind = c->fp_filtered; c->fp_filtered = 0;                 // the filter rode in the tracking launch: the tile tables and the vertices / normals are left
  r.build_tiles = c->tiles_clear && c->fuse_max_dist > 0.f;               // the fusion pass of this frame has cleared the tables: they can be built for the next depth map
  kf_bilateral_args(c, c->fp_src, nullptr, c->alt_raw, c->alt_trunced, c->alt_filtered, c->fp_params[0], c->fp_params[1], c->fp_params[2], c->fp_params[3],
                    r.build_tiles, &r.b, &r.fast);
  memset(&r.ft, 0, sizeof(r.ft));
  r.ft.behind = behind;
  if (behind) {
    r.ft.out_v = c->alt_v0; r.ft.out_n = c->alt_n0;
    if (c->levels == 3 && c->alt_v12[0]) kf_pyr_arg(r.ft.pyr, c->alt_v12, c->alt_n12, c->cols, c->rows);
    r.ft.cam = kf_to_cam(&c->fp_cam);
  }
  r.bil_gx = kf_div_up(c->cols, BIL_TX); r.bil_tiles = r.bil_gx * kf_div_up(c->rows, BIL_TY);
  r.lds = behind ? (size_t)RIDER_LDS_BYTES : 2 * (BIL_TX + 8) * (BIL_TY + 8) * sizeof(float);
}

static int raycast_launch(kf_ctx* c, int has_color, const kf_mat44* transform, const kf_raycast_params* rp, const kf_camera_params* cam,
                          float near_plane, float far_plane, const RaycastOut& out) {
  if (!c || !rp || !cam) return KF_ERR_ARG;
  if ((int)cam->cols != c->cols || (int)cam->rows != c->rows) return KF_ERR_ARG;
  if (has_color && (!c->vol.color || !c->raycast_rgb)) return KF_ERR_STATE;
  if (out.color && !c->vol.color) return KF_ERR_STATE;
  if (out.output == KF_RC_OUT_MAPS) c->model_pyr_ok = 0;                // the model maps' level 0 is rewritten
  RaycastArgs a; kf_raycast_form form; size_t lds;
  { const int st = raycast_args(c, has_color, transform, rp, cam, near_plane, far_plane, out, a, form, lds); if (st) return st; }
  kf_evt_begin(c, KF_STAGE_RAYCAST);
  KfKernelTimer timer; timer.on = kf_evt_attach(c, KF_STAGE_RAYCAST_KERNEL, &timer.e0, &timer.e1);      // the kernel's own timer rides on its dispatch: the kernel as rocprofv3 sees it
  const dim3 grid(kf_div_up(c->cols, 32), kf_div_up(c->rows, 16)), block(RAYCAST_THREADS);
  // the colour form of the z-slab speculation: a kernel of its own, no riders (a pending kf_prefetch_frame note stays where it is and is void at
  // the next kf_preprocess: the frame is then preprocessed by its own launches, same bits)
  RaycastRiders r; const bool riding = !out.color && c->fp_pending && c->alt_raw;
  form.kernel = KF_RC_PLAIN; form.grid = grid.x * grid.y;
  if (out.color) kf_launch(timer, k_raycast_slab_color, grid, block, lds, c->stream, a);
  else if (riding) {
    raycast_riders(c, r);
    const int n_rc = (int)(grid.x * grid.y), n_bil = (r.bil_tiles + 1) / 2;
    const dim3 g2((unsigned)(n_rc + n_bil)); const size_t lds2 = lds > r.lds ? lds : r.lds;
    form.kernel = r.ft.behind ? KF_RC_BEHIND : KF_RC_FILTER; form.fast = r.fast ? 1 : 0; form.grid = g2.x;
    if (r.fast) kf_launch(timer, k_raycast_prefetch<true>, g2, block, lds2, c->stream, a, r.b, r.ft, (int)grid.x, n_rc, r.bil_gx, r.bil_tiles);
    else kf_launch(timer, k_raycast_prefetch<false>, g2, block, lds2, c->stream, a, r.b, r.ft, (int)grid.x, n_rc, r.bil_gx, r.bil_tiles);
  } else kf_launch(timer, k_raycast, grid, block, lds, c->stream, a);
  if (timer.on) kf_evt_attached_done(c, KF_STAGE_RAYCAST_KERNEL);
  if (riding) {
    if (!r.ft.behind) {
      const int st = kf_launch_vertices_normals(c, c->stream, c->alt_filtered, c->alt_v0, c->alt_n0, &c->fp_cam);
      if (st) return st;
    }
    c->alt_pyr_ok = (r.ft.behind && r.ft.pyr.v1) ? 1 : 0;
    c->prefetch_src = c->fp_src; memcpy(c->prefetch_params, c->fp_params, sizeof(c->prefetch_params));
    c->prefetch_cam = c->fp_cam; c->prefetch_valid = 1; c->fp_done = 1;
    c->fp_tiles = r.build_tiles ? 1 : 0; c->fp_tiles_dist = c->fuse_max_dist; c->fp_tiles_min = (r.build_tiles && r.b.acc.n) ? 1 : 0;
    if (r.build_tiles) c->tiles_clear = 0;
  }
  kf_evt_end(c, KF_STAGE_RAYCAST);
  if (form.pyramid) c->model_pyr_ok = 1;
  c->raycast_form = form;
  return (int)hipGetLastError();
}

// ---- viewer frames: a free viewpoint through the volume, display bytes out (reference: the three DataViewer calls of src/HybKinectfu.cpp:145-158) --------
// The march of kf_raycast_volume with the caller's camera -- same bit tables, tile bounds and KF_RAYCAST_* switches (raycast_args) -- whose epilogue writes
// 4 bytes per pixel into the context's view image instead of 32 into the model maps.  It is a bystander: the model maps and model_pyr_ok, raycast_rgb,
// kf_get_raycast_form's record, a pending kf_prefetch_frame note (no riders), the stage timers and the work counters are all left alone.
extern "C" int kf_render_view(kf_ctx* c, int mode, const kf_mat44* pose, const kf_camera_params* view_cam, const kf_raycast_params* rp,
                              float near_plane, float far_plane, float* dev_v, float* dev_n) {
  if (!c || !rp) return KF_ERR_ARG;
  if (mode != KF_VIEW_NORMALS && mode != KF_VIEW_SHADED && mode != KF_VIEW_COLOR) return KF_ERR_ARG;
  if (!view_cam_ok(view_cam)) return KF_ERR_ARG;
  if (mode == KF_VIEW_COLOR && !c->vol.color) return KF_ERR_STATE;
  if (c->vol.own_z0 > 0 || c->vol.own_z1 < c->vol.res) return KF_ERR_STATE;      // a z-slab sees only its own layers
  unsigned* img = nullptr;
  { const int st = kf_view_reserve(c, view_cam->cols, view_cam->rows, &img); if (st) return st; }
  RaycastOut out = {}; out.output = -1;                                    // none of KF_RC_OUT_*: no pyramid, no crossing words
  RaycastArgs a; kf_raycast_form form; size_t lds;
  { const int st = raycast_args(c, mode == KF_VIEW_COLOR, pose, rp, view_cam, near_plane, far_plane, out, a, form, lds); if (st) return st; }
  a.out_v = (float4*)dev_v; a.out_n = (float4*)dev_n; a.out_rgb = nullptr; a.work = nullptr;
  const dim3 grid(kf_div_up((int)view_cam->cols, 32), kf_div_up((int)view_cam->rows, 16)), block(RAYCAST_THREADS);
  if (mode == KF_VIEW_NORMALS) hipLaunchKernelGGL(k_raycast_view<KF_VIEW_NORMALS>, grid, block, lds, c->stream, a, img);
  else if (mode == KF_VIEW_SHADED) hipLaunchKernelGGL(k_raycast_view<KF_VIEW_SHADED>, grid, block, lds, c->stream, a, img);
  else hipLaunchKernelGGL(k_raycast_view<KF_VIEW_COLOR>, grid, block, lds, c->stream, a, img);
  return (int)hipGetLastError();
}

static_assert(sizeof(kf_raycast_form) == 48, "lib.py RaycastForm");
extern "C" int kf_get_raycast_form(kf_ctx* c, kf_raycast_form* out) {
  if (!c || !out) return KF_ERR_ARG;
  *out = c->raycast_form;
  return 0;
}

extern "C" int kf_raycast_volume(kf_ctx* c, int has_color, const kf_mat44* transform, const kf_raycast_params* rp,
                                 const kf_camera_params* cam, float near_plane, float far_plane) {
  RaycastOut out = {}; out.output = KF_RC_OUT_MAPS;
  return raycast_launch(c, has_color, transform, rp, cam, near_plane, far_plane, out);
}

// z-slab variant, MAP FORM (the earlier protocol, kept for per-kernel tests: it evaluates the gradient in the slab that met the crossing and therefore
// drops the rare pixel whose extrapolated vertex leaves that slab's halo -- see kf_raycast_volume_slab_cross below, which SlabPipeline uses):
// this context marches every ray but reports only crossings whose negative sample lies in the voxel layers it owns.  dev_t[pixel] = ray parameter of that crossing (+inf if none), dev_v / dev_n = the vertex / normal it produced
// (zeros when the reference would have given up at that crossing).  The caller reduces over the slabs -- first crossing
// along the ray wins, exactly the reference's sequential march -- and hands the result back with kf_set_model_maps_device.
// The previous sample of the first owned one lies up to x = inc/cell layers outside the owned range and the trilinear +
// gradient taps around a vertex next to it reach ceil(x) + 2 layers: a thinner halo would silently lose crossings at the
// slab faces (those reads fail), so it is refused.  Layers clipped by the volume's own faces do not count.
static int slab_halo_check(const kf_ctx* c, const kf_raycast_params* rp) {
  const int need = (int)ceilf(rp->ray_increment / c->vol.cell) + 2;
  const int lo = c->vol.own_z0 - c->vol.bz0 * KF_BRICK, hi = c->vol.bz1 * KF_BRICK - c->vol.own_z1;
  return ((c->vol.own_z0 > 0 && lo < need) || (c->vol.own_z1 < c->vol.res && hi < need)) ? KF_ERR_ARG : 0;
}
extern "C" int kf_raycast_volume_slab(kf_ctx* c, int has_color, const kf_mat44* transform, const kf_raycast_params* rp,
                                      const kf_camera_params* cam, float near_plane, float far_plane,
                                      float* dev_t, float* dev_v, float* dev_n) {
  if (!c || !rp || !dev_t || !dev_v || !dev_n) return KF_ERR_ARG;
  const int st = slab_halo_check(c, rp);
  if (st) return st;
  RaycastOut out = {}; out.output = KF_RC_OUT_T; out.t = dev_t; out.v = (float4*)dev_v; out.n = (float4*)dev_n;
  return raycast_launch(c, has_color, transform, rp, cam, near_plane, far_plane, out);
}

// after the MIN reduction of the crossing parameters over the slabs: keep this context's candidate where it IS the first
// crossing (t == tmin, finite), zero it elsewhere -- the integer SUM reduction that follows then returns the winner's bits
__global__ void __launch_bounds__(256) k_slab_mask(const float* __restrict__ t, const float* __restrict__ tmin, float4* __restrict__ v, float4* __restrict__ n, int npx) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= npx) return;
  const float ti = t[i];
  if (!(ti == tmin[i] && ti < __builtin_huge_valf())) { const float4 z = make_float4(0.f, 0.f, 0.f, 0.f); v[i] = z; n[i] = z; }
}
extern "C" int kf_slab_mask_candidates(kf_ctx* c, const float* dev_t, const float* dev_tmin, float* dev_v, float* dev_n) {
  if (!c || !dev_t || !dev_tmin || !dev_v || !dev_n) return KF_ERR_ARG;
  const int npx = c->cols * c->rows;
  hipLaunchKernelGGL(k_slab_mask, dim3(kf_div_up(npx, 256)), dim3(256), 0, c->stream, dev_t, dev_tmin, (float4*)dev_v, (float4*)dev_n, npx);
  return (int)hipGetLastError();
}

// ---- the merge SlabPipeline runs: crossings first, normals by the vertex's owner -----------------------------------------------------------------------
// A crossing's vertex is org + dir * alpha with alpha = t - inc * f(t) / (f(t) - f(t - inc)) (raycastingVolume.cu:89-90): an EXTRAPOLATION whenever the two
// interpolated values have the same sign -- an isolated negative voxel at a silhouette does that -- and then the vertex lies anywhere along the ray, far
// outside the halo of the slab that met the crossing (found in round 4: one pixel every few frames on a moving camera; the slab could not read the
// gradient taps and dropped a pixel the single-GPU march keeps).  So the work is split where the data is:
//   1. kf_raycast_volume_slab_cross: every slab marches every ray and reports, per pixel, ONE 64-bit word (crossing parameter << 32 | alpha), what it can
//      decide alone (the two interpolations at the crossing lie within its halo);
//   2. the caller's MIN all-reduce over those words: positive floats order like their bit patterns, so the first crossing along the ray wins and brings its
//      alpha along (alpha 0: the reference gave up at that crossing -- the pixel stays empty, as in the sequential march);
//   3. kf_slab_ray_normals: every rank rebuilds the winners' vertices from the rays (a pure function of pose and camera, which all ranks hold bit for bit);
//      the rank that OWNS the vertex's voxel layer evaluates gradientForPoint (:16-42) -- its taps reach two layers, inside any halo -- and contributes
//      the normal (three words; all-zero bits = none), everybody else zeros; the previous sample's position, whose voxel the function bounds-tests, is found by replaying the chain of additions
//      from t_min (:116), exactly as the march walked it;
//   4. the caller's integer SUM all-reduce (exactly one contributor per pixel: the winner's bits, -0.0 included) and kf_set_model_maps_rays, which writes
//      the model maps and levels 1 and 2 of their pyramids.
// Two collectives and three launches per frame; 8 + 12 bytes per pixel on the wire (round 4: 8 + 16 -- the fourth word only said "valid", which a unit normal says itself).
static int raycast_slab_cross(kf_ctx* c, const kf_mat44* transform, const kf_raycast_params* rp, const kf_camera_params* cam, float near_plane, float far_plane,
                              uint64_t* dev_ta, uint64_t* dev_ta_own, float* dev_spec, bool spec, bool color) {
  if (!c || !rp || !dev_ta || (spec && (!dev_ta_own || !dev_spec))) return KF_ERR_ARG;
  const int st = slab_halo_check(c, rp);
  if (st) return st;
  RaycastOut out = {}; out.output = spec ? KF_RC_OUT_TA_SPEC : KF_RC_OUT_TA; out.color = color;
  out.ta = (unsigned long long*)dev_ta; out.own_ta = (unsigned long long*)dev_ta_own; out.spec = dev_spec;
  return raycast_launch(c, 0, transform, rp, cam, near_plane, far_plane, out);
}
extern "C" int kf_raycast_volume_slab_cross(kf_ctx* c, const kf_mat44* transform, const kf_raycast_params* rp, const kf_camera_params* cam,
                                            float near_plane, float far_plane, uint64_t* dev_ta) {
  return raycast_slab_cross(c, transform, rp, cam, near_plane, far_plane, dev_ta, nullptr, nullptr, false, false);
}
extern "C" int kf_raycast_volume_slab_cross_spec(kf_ctx* c, const kf_mat44* transform, const kf_raycast_params* rp, const kf_camera_params* cam,
                                                 float near_plane, float far_plane, uint64_t* dev_ta, uint64_t* dev_ta_own, float* dev_spec) {
  return raycast_slab_cross(c, transform, rp, cam, near_plane, far_plane, dev_ta, dev_ta_own, dev_spec, true, false);
}
// The colour forms of the three calls (a context with a colour plane): the candidate is 4 words per pixel, the normal's three and the uchar4 colour
// word of interpolateColor at the VERTEX (raycastingVolume.cu:91-92, tsdfVolume.h:123-148) -- evaluated by the vertex's owner like the gradient, before
// and independently of it, so a pixel without a normal can carry a colour, as in the whole-volume march.  All-zero bits: no colour.
extern "C" int kf_raycast_volume_slab_cross_spec_color(kf_ctx* c, const kf_mat44* transform, const kf_raycast_params* rp, const kf_camera_params* cam,
                                                       float near_plane, float far_plane, uint64_t* dev_ta, uint64_t* dev_ta_own, float* dev_spec) {
  return raycast_slab_cross(c, transform, rp, cam, near_plane, far_plane, dev_ta, dev_ta_own, dev_spec, true, true);
}
struct SlabNormalArgs { KfVolume vol; KfCam cam; const float* pose; KfMat pose_val; const unsigned long long* ta; float* cand; float inc, near_plane, far_plane; int shared_grad;
                        const unsigned long long* own_ta; const float* spec; };   // own_ta / spec: kf_raycast_volume_slab_cross_spec's second outputs, or null   // cand, spec: 3 floats per pixel (the colour forms: 4)
// COLOR (compile time; kf_slab_ray_normals_color): spec and cand have 4 words per pixel, the fourth the colour at the vertex
template <bool COLOR>
__device__ __forceinline__ void slab_ray_normals_body(SlabNormalArgs a) {
  // (a workgroup is a 32x8 pixel tile, a wave an 8x8 patch of it: its 64 vertices stay inside a few bricks -- fewer cache lines per gather instruction)
  const int x = (int)blockIdx.x * 32 + (int)(threadIdx.x >> 6) * 8 + (int)(threadIdx.x & 7), y = (int)blockIdx.y * 8 + (int)((threadIdx.x >> 3) & 7);
  if (x >= a.cam.cols || y >= a.cam.rows) return;
  const KfVolume& v = a.vol;
  const int i = y * a.cam.cols + x;
  const unsigned long long w = a.ta[i];
  const float t_cross = __uint_as_float((unsigned)(w >> 32));
  const unsigned alpha_bits = (unsigned)w;
  float3 out = kf3(0.f, 0.f, 0.f);                                             // all-zero bits: not this rank's vertex, or no gradient (a found gradient is a unit vector)
  unsigned out_c = 0u;                                                         // (COLOR) all-zero bits: not this rank's vertex, or no colour there
  constexpr int W = COLOR ? 4 : 3;
  if (t_cross < __builtin_huge_valf() && alpha_bits != 0u && a.own_ta && a.own_ta[i] == w) {
    // this context's own crossing won: its march has evaluated the vertex already, if the vertex is this context's (zeros otherwise: the owner's
    // own crossing word differs from the winner's, so the owner takes the branch below)
    out = kf3(a.spec[W * i], a.spec[W * i + 1], a.spec[W * i + 2]);
    if (COLOR) out_c = __float_as_uint(a.spec[W * i + 3]);
  } else if (t_cross < __builtin_huge_valf() && alpha_bits != 0u) {
    float3 org, dir, cam_dir;
    rc_pixel_ray(a.cam, a.pose ? a.pose : a.pose_val.m, x, y, org, dir, cam_dir);
    const float3 vtx = kf_add(org, kf_scale(dir, __uint_as_float(alpha_bits)));
    const KfRecip rS = kf_recip(v.size), rcell = kf_recip(v.cell);
    int gz = kf_f2i(kf_div(vtx.z * (float)v.res, rS));                       // the vertex's voxel layer (tsdfVolume.h:50-56), clamped: exactly one owner
    gz = max(0, min(gz, v.res - 1));
    if (gz >= v.own_z0 && gz < v.own_z1) {
      if (COLOR) { uchar4 c = make_uchar4(0, 0, 0, 0); kf_interpolate_color(v, vtx, c); out_c = rc_color_word(c); }     // before the gradient, whatever it finds
      float tmin, tmax;
      rc_ray_interval(v.size, a.near_plane, a.far_plane, org, dir, cam_dir, tmin, tmax);
      float t = tmin, t_prev = tmin;
      if (t < t_cross) kf_ray_advance(t, t_prev, a.inc, t_cross);            // the march's own chain of additions (its closed form, exact: kf_selftest_div mode 12): t ends ON t_cross, t_prev on the sample before it
      const float3 last_pos = kf_add(org, kf_scale(dir, t_prev));
      float3 grad;
      if (gradient_for_point_either<6, RC_SLAB_GRAD_ROUNDS>(a.shared_grad, ((blockIdx.x + blockIdx.y + (threadIdx.x >> 6)) & 1u) != 0u, v, last_pos, vtx, rS, rcell, grad)) out = grad;                  // (the six taps' 48 gathers in one batch: this kernel has the registers)
    }
  }
  a.cand[W * i] = out.x; a.cand[W * i + 1] = out.y; a.cand[W * i + 2] = out.z;
  if (COLOR) a.cand[W * i + 3] = __uint_as_float(out_c);
}
__global__ void __launch_bounds__(256) k_slab_ray_normals(SlabNormalArgs a) { slab_ray_normals_body<false>(a); }
__global__ void __launch_bounds__(256) k_slab_ray_normals_color(SlabNormalArgs a) { slab_ray_normals_body<true>(a); }
static int slab_ray_normals(kf_ctx* c, const kf_mat44* transform, const kf_raycast_params* rp, const kf_camera_params* cam,
                            float near_plane, float far_plane, const uint64_t* dev_ta_min, const uint64_t* dev_ta_own, const float* dev_spec, float* dev_cand,
                            bool color = false, bool view = false) {
  if (!c || !rp || !cam || !dev_ta_min || !dev_cand) return KF_ERR_ARG;
  // (the kernels follow a.cam alone -- the pixel, its ray and the buffers' index -- so a view's camera needs only a grid of its own size)
  if (view ? !view_cam_ok(cam) : ((int)cam->cols != c->cols || (int)cam->rows != c->rows)) return KF_ERR_ARG;
  if (color && !c->vol.color) return KF_ERR_STATE;
  SlabNormalArgs a;
  a.vol = c->vol; a.ta = (const unsigned long long*)dev_ta_min; a.cand = dev_cand;
  a.own_ta = (dev_ta_own && dev_spec) ? (const unsigned long long*)dev_ta_own : nullptr; a.spec = dev_spec;
  a.cam = kf_to_cam(cam);
  a.inc = rp->ray_increment; a.near_plane = near_plane; a.far_plane = far_plane;
  a.shared_grad = rc_shared_grad_for(c->vol);
  kf_pose_arg(c, transform, a.pose, a.pose_val);
  const dim3 grid(kf_div_up(a.cam.cols, 32), kf_div_up(a.cam.rows, 8));
  if (color) hipLaunchKernelGGL(k_slab_ray_normals_color, grid, dim3(256), 0, c->stream, a);
  else hipLaunchKernelGGL(k_slab_ray_normals, grid, dim3(256), 0, c->stream, a);
  return (int)hipGetLastError();
}
// dev_ta_own and dev_spec (4 words per pixel) may both be NULL: then every owned vertex is evaluated here
extern "C" int kf_slab_ray_normals_color(kf_ctx* c, const kf_mat44* transform, const kf_raycast_params* rp, const kf_camera_params* cam,
                                         float near_plane, float far_plane, const uint64_t* dev_ta_min, const uint64_t* dev_ta_own, const float* dev_spec, float* dev_cand) {
  if ((dev_ta_own == nullptr) != (dev_spec == nullptr)) return KF_ERR_ARG;
  return slab_ray_normals(c, transform, rp, cam, near_plane, far_plane, dev_ta_min, dev_ta_own, dev_spec, dev_cand, true);
}
extern "C" int kf_slab_ray_normals(kf_ctx* c, const kf_mat44* transform, const kf_raycast_params* rp, const kf_camera_params* cam,
                                   float near_plane, float far_plane, const uint64_t* dev_ta_min, float* dev_cand) {
  return slab_ray_normals(c, transform, rp, cam, near_plane, far_plane, dev_ta_min, nullptr, nullptr, dev_cand);
}
extern "C" int kf_slab_ray_normals_spec(kf_ctx* c, const kf_mat44* transform, const kf_raycast_params* rp, const kf_camera_params* cam,
                                        float near_plane, float far_plane, const uint64_t* dev_ta_min, const uint64_t* dev_ta_own, const float* dev_spec, float* dev_cand) {
  if (!dev_ta_own || !dev_spec) return KF_ERR_ARG;
  return slab_ray_normals(c, transform, rp, cam, near_plane, far_plane, dev_ta_min, dev_ta_own, dev_spec, dev_cand);
}
struct SlabUnpackArgs { const unsigned long long* ta; const float* cand; float4* v; float4* n; KfCam cam; const float* pose; KfMat pose_val; KfPyrOut pyr; };   // cand: 3 floats per pixel (the colour form: 4)
// one 32x8 pixel tile per workgroup: the tile's whole 2x2 and 4x4 blocks also give levels 1 and 2 of the model maps' pyramids (kf_tile_pyramid),
// so the tracker that follows finds them done, as after a single-GPU raycast
// COLOR (compile time; kf_set_model_maps_rays_color): cand has 4 words per pixel and the fourth goes to rgb (KF_MAP_RAYCAST_RGB), normal or not
template <bool COLOR>
__device__ __forceinline__ void slab_rays_unpack_body(SlabUnpackArgs a, uchar4* rgb) {
  __shared__ float4 s_v[32 * 8], s_n[32 * 8], s1_v[16 * 4], s1_n[16 * 4];
  const int x = (int)blockIdx.x * 32 + (int)(threadIdx.x & 31), y = (int)blockIdx.y * 8 + (int)(threadIdx.x >> 5);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f), n = v;
  if (x < a.cam.cols && y < a.cam.rows) {
    const int i = y * a.cam.cols + x;
    constexpr int W = COLOR ? 4 : 3;
    const float3 cd = kf3(a.cand[W * i], a.cand[W * i + 1], a.cand[W * i + 2]);
    if (COLOR) rgb[i] = rc_word_color(__float_as_uint(a.cand[W * i + 3]));
    if ((__float_as_uint(cd.x) | __float_as_uint(cd.y) | __float_as_uint(cd.z)) != 0u) {     // the vertex's owner found a gradient (a unit vector: some bit is set): vertex = org + dir * alpha (raycastingVolume.cu:90), w = 1
      float3 org, dir, cam_dir;
      rc_pixel_ray(a.cam, a.pose ? a.pose : a.pose_val.m, x, y, org, dir, cam_dir);
      const float3 vtx = kf_add(org, kf_scale(dir, __uint_as_float((unsigned)a.ta[i])));
      v = make_float4(vtx.x, vtx.y, vtx.z, 1.0f);
      n = make_float4(cd.x, cd.y, cd.z, 0.f);
    }
    a.v[i] = v; a.n[i] = n;
  }
  if (a.pyr.v1) {                                                            // uniform
    s_v[threadIdx.x] = v; s_n[threadIdx.x] = n;
    kf_tile_pyramid<32, 8>(a.pyr, (int)blockIdx.x * 32, (int)blockIdx.y * 8, (int)threadIdx.x, s_v, s_n, s1_v, s1_n, [] { __syncthreads(); });
  }
}
__global__ void __launch_bounds__(256) k_slab_rays_unpack(SlabUnpackArgs a) { slab_rays_unpack_body<false>(a, nullptr); }
__global__ void __launch_bounds__(256) k_slab_rays_unpack_color(SlabUnpackArgs a, uchar4* rgb) { slab_rays_unpack_body<true>(a, rgb); }
static int set_model_maps_rays(kf_ctx* c, const kf_mat44* transform, const kf_camera_params* cam, const uint64_t* dev_ta_min, const float* dev_cand, bool color) {
  if (!c || !cam || !dev_ta_min || !dev_cand) return KF_ERR_ARG;
  if ((int)cam->cols != c->cols || (int)cam->rows != c->rows) return KF_ERR_ARG;
  if (color && !c->raycast_rgb) return KF_ERR_STATE;
  SlabUnpackArgs a;
  c->model_pyr_ok = 0;
  memset(&a.pyr, 0, sizeof(a.pyr));
  if (c->levels == 3) kf_pyr_arg(a.pyr, c->model_v + 1, c->model_n + 1, c->cols, c->rows);
  a.ta = (const unsigned long long*)dev_ta_min; a.cand = dev_cand; a.v = c->model_v[0]; a.n = c->model_n[0];
  a.cam = kf_to_cam(cam);
  kf_pose_arg(c, transform, a.pose, a.pose_val);      // the pose the raycast used: nothing moves it between the raycast and this call
  if (color) hipLaunchKernelGGL(k_slab_rays_unpack_color, dim3(kf_div_up(c->cols, 32), kf_div_up(c->rows, 8)), dim3(256), 0, c->stream, a, c->raycast_rgb);
  else hipLaunchKernelGGL(k_slab_rays_unpack, dim3(kf_div_up(c->cols, 32), kf_div_up(c->rows, 8)), dim3(256), 0, c->stream, a);
  if (a.pyr.v1) c->model_pyr_ok = 1;
  return (int)hipGetLastError();
}
extern "C" int kf_set_model_maps_rays(kf_ctx* c, const kf_mat44* transform, const kf_camera_params* cam, const uint64_t* dev_ta_min, const float* dev_cand) {
  return set_model_maps_rays(c, transform, cam, dev_ta_min, dev_cand, false);
}
extern "C" int kf_set_model_maps_rays_color(kf_ctx* c, const kf_mat44* transform, const kf_camera_params* cam, const uint64_t* dev_ta_min, const float* dev_cand) {
  return set_model_maps_rays(c, transform, cam, dev_ta_min, dev_cand, true);
}

// ---- a merged view over z-slabs: the three per-member steps (what kf_group_render_view enqueues) ----------------------------------------------------
// The ray-form merge above for the CALLER's camera, ending in display bytes instead of model maps: kf_view_slab_cross on every member, the MIN
// all-reduce, kf_view_slab_normals on every member, the integer SUM all-reduce, kf_view_from_rays on one.  All three are bystanders exactly as
// kf_render_view is: the model maps and model_pyr_ok, raycast_rgb, kf_get_raycast_form's record, a pending kf_prefetch_frame note (no riders), the
// stage timers and the work counters are left alone.  A whole-volume context owns every layer and is accepted too.
extern "C" int kf_view_slab_cross(kf_ctx* c, int color, const kf_mat44* pose, const kf_camera_params* view_cam, const kf_raycast_params* rp,
                                  float near_plane, float far_plane, uint64_t* dev_ta, uint64_t* dev_ta_own, float* dev_spec) {
  if (!c || !rp || !dev_ta || !dev_ta_own || !dev_spec) return KF_ERR_ARG;
  if (!view_cam_ok(view_cam)) return KF_ERR_ARG;
  { const int st = slab_halo_check(c, rp); if (st) return st; }
  if (color && !c->vol.color) return KF_ERR_STATE;
  RaycastOut out = {}; out.output = KF_RC_OUT_TA_SPEC; out.color = color != 0;       // (not the model maps: raycast_args arms no pyramid)
  out.ta = (unsigned long long*)dev_ta; out.own_ta = (unsigned long long*)dev_ta_own; out.spec = dev_spec;
  RaycastArgs a; kf_raycast_form form; size_t lds;
  { const int st = raycast_args(c, 0, pose, rp, view_cam, near_plane, far_plane, out, a, form, lds); if (st) return st; }
  a.out_v = nullptr; a.out_n = nullptr; a.out_rgb = nullptr; a.work = nullptr;
  const dim3 grid(kf_div_up((int)view_cam->cols, 32), kf_div_up((int)view_cam->rows, 16)), block(RAYCAST_THREADS);
  if (color) hipLaunchKernelGGL(k_raycast_view_cross<true>, grid, block, lds, c->stream, a);
  else hipLaunchKernelGGL(k_raycast_view_cross<false>, grid, block, lds, c->stream, a);
  return (int)hipGetLastError();
}
extern "C" int kf_view_slab_normals(kf_ctx* c, int color, const kf_mat44* pose, const kf_camera_params* view_cam, const kf_raycast_params* rp,
                                    float near_plane, float far_plane, const uint64_t* dev_ta_min, const uint64_t* dev_ta_own, const float* dev_spec,
                                    float* dev_cand) {
  if ((dev_ta_own == nullptr) != (dev_spec == nullptr)) return KF_ERR_ARG;
  return slab_ray_normals(c, pose, rp, view_cam, near_plane, far_plane, dev_ta_min, dev_ta_own, dev_spec, dev_cand, color != 0, true);
}
// one pixel per lane: what slab_rays_unpack_body does for the model maps -- the vertex org + dir * alpha where the candidate normal has a set bit, the
// colour from the fourth word whatever the normal -- pushed through the pixel function; the eye is the pose's translation, the ray's origin
struct ViewRaysArgs { const unsigned long long* ta; const float* cand; unsigned* img; float4* v; float4* n; KfCam cam; const float* pose; KfMat pose_val; };
template <int MODE, int W>
__global__ void __launch_bounds__(256) k_view_from_rays(ViewRaysArgs a) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= a.cam.cols * a.cam.rows) return;
  const int y = i / a.cam.cols, x = i - y * a.cam.cols;
  const float3 cd = kf3(a.cand[W * i], a.cand[W * i + 1], a.cand[W * i + 2]);
  const uchar4 col = W == 4 ? rc_word_color(__float_as_uint(a.cand[W * i + 3])) : make_uchar4(0, 0, 0, 0);
  float3 org, dir, cam_dir;
  rc_pixel_ray(a.cam, a.pose ? a.pose : a.pose_val.m, x, y, org, dir, cam_dir);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f), n = v;
  if ((__float_as_uint(cd.x) | __float_as_uint(cd.y) | __float_as_uint(cd.z)) != 0u) {
    const float3 vtx = kf_add(org, kf_scale(dir, __uint_as_float((unsigned)a.ta[i])));
    v = make_float4(vtx.x, vtx.y, vtx.z, 1.0f);
    n = make_float4(cd.x, cd.y, cd.z, 0.f);
  }
  if (a.v) a.v[i] = v;
  if (a.n) a.n[i] = n;
  a.img[i] = kf_view_pixel<MODE>(v, n, col, org);
}
extern "C" int kf_view_from_rays(kf_ctx* c, int mode, const kf_mat44* pose, const kf_camera_params* view_cam, const uint64_t* dev_ta_min,
                                 const float* dev_cand, uint32_t words, float* dev_v, float* dev_n) {
  if (!c || !dev_ta_min || !dev_cand) return KF_ERR_ARG;
  if (mode != KF_VIEW_NORMALS && mode != KF_VIEW_SHADED && mode != KF_VIEW_COLOR) return KF_ERR_ARG;
  if (!view_cam_ok(view_cam)) return KF_ERR_ARG;
  if ((words != 3 && words != 4) || (mode == KF_VIEW_COLOR && words != 4)) return KF_ERR_ARG;
  ViewRaysArgs a;
  { const int st = kf_view_reserve(c, view_cam->cols, view_cam->rows, &a.img); if (st) return st; }
  a.ta = (const unsigned long long*)dev_ta_min; a.cand = dev_cand; a.v = (float4*)dev_v; a.n = (float4*)dev_n;
  a.cam = kf_to_cam(view_cam);
  kf_pose_arg(c, pose, a.pose, a.pose_val);
  const dim3 grid(kf_div_up(a.cam.cols * a.cam.rows, 256)), block(256);
  if (mode == KF_VIEW_COLOR) hipLaunchKernelGGL((k_view_from_rays<KF_VIEW_COLOR, 4>), grid, block, 0, c->stream, a);
  else if (mode == KF_VIEW_NORMALS && words == 3) hipLaunchKernelGGL((k_view_from_rays<KF_VIEW_NORMALS, 3>), grid, block, 0, c->stream, a);
  else if (mode == KF_VIEW_NORMALS) hipLaunchKernelGGL((k_view_from_rays<KF_VIEW_NORMALS, 4>), grid, block, 0, c->stream, a);
  else if (words == 3) hipLaunchKernelGGL((k_view_from_rays<KF_VIEW_SHADED, 3>), grid, block, 0, c->stream, a);
  else hipLaunchKernelGGL((k_view_from_rays<KF_VIEW_SHADED, 4>), grid, block, 0, c->stream, a);
  return (int)hipGetLastError();
}

extern "C" int kf_set_model_maps_device(kf_ctx* c, const float* dev_v, const float* dev_n) {
  if (!c || !dev_v || !dev_n) return KF_ERR_ARG;
  const size_t bytes = (size_t)c->cols * c->rows * sizeof(float4);
  c->model_pyr_ok = 0;
  KF_CHECK(hipMemcpyAsync(c->model_v[0], dev_v, bytes, hipMemcpyDeviceToDevice, c->stream));
  KF_CHECK(hipMemcpyAsync(c->model_n[0], dev_n, bytes, hipMemcpyDeviceToDevice, c->stream));
  return 0;
}
