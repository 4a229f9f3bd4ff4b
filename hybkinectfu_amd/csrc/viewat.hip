// viewat.hip -- viewer frames of the whole map: kf_render_view_at renders a window that stands elsewhere (no reference counterpart: the reference's cube
// never moves, src/HybKinectfu.cpp:51-54, and its viewer looks at that one cube, :145-158).
//
// The call gives the bytes kf_render_view would give after kf_shift_volume had moved the window to another origin, the store's bricks restored, and moves
// nothing: the viewer's half of mapmesh.hip's virtual window (vwindow.h).
//   resolve : map_resolve_brick over ALL nb^3 bricks of the virtual window, a wave per brick -- the window's copy, else the store's slot, else the zero
//             brick -- into the call's own indirection table; a brick with a negative voxel sets its bit in the virtual has-negative bits and marks its
//             macro, super and meso cell in the virtual skip tables (kf_mark_macro's indexing).  All tables are cleared on the stream first.
//   pose    : for pose == NULL, t - (float)d * cell per axis (kf_shift_translation, shared with k_shift_pose) from the device-resident pose into the scratch: no read-back.
//   march   : raycast_tile<false, VIEW> of raycast_tile.h, compiled a second time here with the addressing hooks redefined: the sample's voxel, the lazily
//             fetched previous sample, the trilinear taps, the colour taps go through the table, the has-negative flag is the virtual bit.  LDS placement,
//             KF_RAYCAST_* switches, tile bounds, tile and workgroup shape follow raycast_args exactly as for kf_render_view.  The shared-neighbourhood
//             gradient (grad_shared.h) addresses v.tw through a buffer descriptor and cannot go through a table: this form takes the six separate lookups,
//             which give the same bits (tests/test_gpu_raycast_forms.py).
// Why the bytes are the shift's: every skip level is conservative by construction -- a set bit costs a read and changes no result -- so the image depends on
// the voxels alone, and those are the ones the shift would assemble (precedence above = what k_shift_bricks keeps + what k_store_restore brings back).
// The deferred-weight words are neither consulted nor flushed, by mapmesh.hip's argument: the march and the interpolations ask of a weight only whether it is
// zero, and a quarter brick with a pending count holds stored weights >= 1.
// (A file of its own: a kernel added to raycast.hip would renumber the local labels of its neighbours, whose listings are to stay what they were.)
#include "kf_internal.h"
#include "bilateral_tile.h"
#include "grad_shared.h"
#include "view_pixel.h"
#include "brick_key.h"
#include "brick_find.h"
#include "vwindow.h"
#include <stdint.h>
#include <string.h>

namespace viewat {

using mapmesh::McVBrick;
using mapmesh::McResolve;

// RaycastArgs::vol here: the window's KfVolume for its shape (res, nb, nm .. cell, size), `macrobits` and `negbits` pointing at the VIRTUAL tables, plus the
// indirection table.  Its voxel, colour and flag pointers are not read by any kernel compiled here.
struct VVolume : KfVolume { const McVBrick* vtab; };
#define RC_VOL VVolume
#define RC_VOL_ASSIGN(dst, src) (static_cast<KfVolume&>(dst) = (src))
#define RC_TSDF_IN_SLOT(v, slot, off) ((v).vtab[slot].tw[off].x)
#define RC_TSDF_AT(v, gx_, gy_, gz_) (mapmesh::v_voxel((v).vtab, v, gx_, gy_, gz_).x)
#define RC_BRICK_HASNEG(v, slot) ((((v).negbits[(slot) >> 5] >> ((slot) & 31u)) & 1u) != 0u)
#define RC_INTERP_LOAD(v, it, q) mapmesh::v_interp_load((v).vtab, v, it, q)
#define RC_INTERP_LOAD_NB(v, it, q) mapmesh::v_interp_load_nb((v).vtab, v, it, q)
#define RC_INTERP_SDF_PAIR(v, p1, p2, rS, rcell, ok1, d1, ok2, d2) mapmesh::v_interpolate_sdf_pair((v).vtab, v, p1, p2, rS, rcell, ok1, d1, ok2, d2)
#define RC_INTERP_COLOR(v, pos, out) mapmesh::v_interp_color((v).vtab, v, pos, out)
#define RC_SHARED_GRAD(shared) 0
#include "raycast_tile.h"

// the march of kf_render_view (k_raycast_view) over the virtual window
template <int MODE>
__global__ void __launch_bounds__(RAYCAST_THREADS) k_view_at(RaycastArgs a, unsigned* img) {
  extern __shared__ unsigned s_dyn[];
  raycast_tile<false, MODE + 1>(a, (int)blockIdx.x, (int)blockIdx.y, s_dyn, img);
}

// resolve over the whole virtual window; vv: the window's shape with `macrobits` = the virtual skip tables [macro | super | meso]
__global__ void __launch_bounds__(256) k_view_resolve(KfVolume v, KfVolume vv, KfBrickStore st, McResolve g, McVBrick* __restrict__ vtab, const float2* __restrict__ zero,
                                                      unsigned* __restrict__ vneg) {
  const unsigned nb = (unsigned)v.nb, n = nb * nb * nb;
  const unsigned lane = threadIdx.x & 63u;
  for (unsigned i = blockIdx.x * 4u + (threadIdx.x >> 6); i < n; i += gridDim.x * 4u) {            // a wave per brick; i IS the virtual slot (x fastest)
    const int bx = (int)(i % nb), by = (int)((i / nb) % nb), bz = (int)(i / (nb * nb));
    bool neg;
    const McVBrick e = mapmesh::map_resolve_brick(v, st, g, bx, by, bz, zero, lane, neg);
    if (lane == 0) {
      vtab[i] = e;
      if (neg) {
        atomicOr(&vneg[i >> 5], 1u << (i & 31u));
        kf_mark_macro(vv, bx, by, bz);
      }
    }
  }
}

// the device-resident pose as kf_shift_volume(d) would leave it (kf_shift_translation, as in k_shift_pose)
__global__ void k_view_pose(const KfTrackState* __restrict__ st, float* __restrict__ out, int dx, int dy, int dz, float cell) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  for (int i = 0; i < 16; ++i) out[i] = st->pose[i];
  kf_shift_translation(st->pose, out, dx, dy, dz, cell);
}

// the scratch: [zero brick | table | skip tables | has-negative bits | pose]; every part a multiple of 16 bytes
struct Scratch { const float2* zero; McVBrick* vtab; unsigned* skip; unsigned* neg; float* pose; size_t table_bytes, bytes; };
static Scratch scratch_parts(const kf_ctx* c, void* base) {
  const size_t zero_b = (size_t)KF_BRICK_VOX * sizeof(float2), vtab_b = c->n_stored_bricks * sizeof(McVBrick), skip_b = kf_skip_table_words(c->vol) * sizeof(unsigned),
               neg_b = kf_negbit_words(c->n_stored_bricks) * sizeof(unsigned);
  Scratch s;
  char* p = reinterpret_cast<char*>(base);
  s.zero = reinterpret_cast<const float2*>(p);
  s.vtab = reinterpret_cast<McVBrick*>(p + zero_b);
  s.skip = reinterpret_cast<unsigned*>(p + zero_b + vtab_b);
  s.neg = reinterpret_cast<unsigned*>(p + zero_b + vtab_b + skip_b);
  s.pose = reinterpret_cast<float*>(p + zero_b + vtab_b + skip_b + neg_b);
  s.table_bytes = skip_b + neg_b;
  s.bytes = zero_b + vtab_b + skip_b + neg_b + 16 * sizeof(float);
  return s;
}
static int scratch(kf_ctx* c) {
  if (c->view_at_scratch) return 0;
  static_assert(sizeof(McVBrick) == 16, "16 bytes per brick slot");
  char probe[1];
  const size_t bytes = scratch_parts(c, probe).bytes;
  void* p = nullptr;
  const hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) { (void)hipGetLastError(); return KF_ERR_ALLOC; }
  const hipError_t m = hipMemsetAsync(p, 0, (size_t)KF_BRICK_VOX * sizeof(float2), c->stream);       // the zero brick; everything else is written before it is read
  if (m != hipSuccess) { hipFree(p); return (int)m; }
  c->view_at_scratch = p;
  return 0;
}

}  // namespace viewat

extern "C" int kf_render_view_at(kf_ctx* c, int mode, const int32_t frame_origin_vox[3], const kf_mat44* pose, const kf_camera_params* view_cam,
                                 const kf_raycast_params* rp, float near_plane, float far_plane, float* dev_v, float* dev_n) {
  using namespace viewat;
  if (!c || !frame_origin_vox || !rp) return KF_ERR_ARG;
  if (mode != KF_VIEW_NORMALS && mode != KF_VIEW_SHADED && mode != KF_VIEW_COLOR) return KF_ERR_ARG;
  if (!view_cam_ok(view_cam)) return KF_ERR_ARG;
  for (int k = 0; k < 3; ++k) if (frame_origin_vox[k] % KF_BRICK) return KF_ERR_ARG;
  if (mode == KF_VIEW_COLOR && !c->vol.color) return KF_ERR_STATE;
  const KfVolume& v = c->vol;
  if (v.own_z0 > 0 || v.own_z1 < v.res || !kf_whole_volume(c)) return KF_ERR_STATE;      // a z-slab context, kf_render_view's code
  if (!kf_window_in_key_range(frame_origin_vox, v.nb)) return KF_ERR_ARG;
  int d[3];
  for (int k = 0; k < 3; ++k) {                                            // the shift that would bring the window there: kf_shift_volume takes 32-bit components
    const int64_t dd = (int64_t)frame_origin_vox[k] - (int64_t)c->origin_vox[k];
    if (dd > INT32_MAX || dd < INT32_MIN) return KF_ERR_ARG;
    d[k] = (int)dd;
  }
  RaycastOut out = {}; out.output = -1;                                    // none of KF_RC_OUT_*: no pyramid, no crossing words
  RaycastArgs a; kf_raycast_form form; size_t lds;
  { const int st = raycast_args(c, mode == KF_VIEW_COLOR, pose, rp, view_cam, near_plane, far_plane, out, a, form, lds); if (st) return st; }   // (touches nothing)
  KF_CHECK(hipSetDevice(c->cfg.device));
  { const int st = scratch(c); if (st) return st; }
  unsigned* img = nullptr;
  { const int st = kf_view_reserve(c, view_cam->cols, view_cam->rows, &img); if (st) return st; }
  const Scratch s = scratch_parts(c, c->view_at_scratch);
  a.vol.macrobits = s.skip; a.vol.negbits = s.neg; a.vol.vtab = s.vtab;
  a.shared_grad = 0;
  a.out_v = (float4*)dev_v; a.out_n = (float4*)dev_n; a.out_rgb = nullptr; a.work = nullptr;
  if (!pose) a.pose = s.pose;
  McResolve r;
  for (int k = 0; k < 3; ++k) { r.wlo[k] = 0; r.wn[k] = v.nb; r.fb[k] = frame_origin_vox[k] / KF_BRICK; r.ob[k] = c->origin_vox[k] / KF_BRICK; }   // exact: multiples of 8 both
  KfVolume vv = v; vv.macrobits = s.skip;
  KF_CHECK(hipMemsetAsync(s.skip, 0, s.table_bytes, c->stream));           // the skip tables and the has-negative bits lie next to each other
  const unsigned n_b = (unsigned)c->n_stored_bricks, walk_all = (unsigned)c->num_cus * 8u, walk = (n_b + 3) / 4 < walk_all ? (n_b + 3) / 4 : walk_all;
  hipLaunchKernelGGL(k_view_resolve, dim3(walk), dim3(256), 0, c->stream, v, vv, c->bstore, r, s.vtab, s.zero, s.neg);
  if (!pose) hipLaunchKernelGGL(k_view_pose, dim3(1), dim3(64), 0, c->stream, c->track, s.pose, d[0], d[1], d[2], v.cell);
  const dim3 grid(kf_div_up((int)view_cam->cols, 32), kf_div_up((int)view_cam->rows, 16)), block(RAYCAST_THREADS);
  if (mode == KF_VIEW_NORMALS) hipLaunchKernelGGL(k_view_at<KF_VIEW_NORMALS>, grid, block, lds, c->stream, a, img);
  else if (mode == KF_VIEW_SHADED) hipLaunchKernelGGL(k_view_at<KF_VIEW_SHADED>, grid, block, lds, c->stream, a, img);
  else hipLaunchKernelGGL(k_view_at<KF_VIEW_COLOR>, grid, block, lds, c->stream, a, img);
  return (int)hipGetLastError();
}
