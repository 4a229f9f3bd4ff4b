// shift.hip -- the moving volume: kf_shift_volume slides the TSDF window by whole bricks, in place, on the context's stream.
// No reference counterpart: the reference's cube stays where HybKinectfu::init put it (src/HybKinectfu.cpp:51-54, src/cuda/tsdfVolume.h:29-37).
//
// A brick is one contiguous 4 KiB block of (tsdf, weight) plus 2 KiB of colour and one 8-byte deferred-weight word, so a shift by whole
// bricks moves every brick by a constant slot offset.  The move runs in place, one launch per brick plane perpendicular to the first axis
// (z, y, x) with a non-zero shift: destination plane p takes source plane p + s, and the planes are walked so that a plane is read before it
// is overwritten (ascending for s > 0, descending for s < 0).  Inside one launch source and destination plane differ, so no workgroup reads
// what another writes; stream order does the rest.  The pass that moves a brick also sees all of its voxels, so it rebuilds the brick's
// flags, its has-negative bit and the skip tables on the way: no second sweep of the volume.
//
// With a brick store reserved (brickstore.hip) the observed bricks that leave are copied into the store before anything moves, and the bricks that
// enter are looked up in it after the move: two more launches around the ones above, which stay as they are.
#include "kf_internal.h"
#include "brick_key.h"
#include <stdint.h>

// One workgroup iteration moves one brick of brick plane `plane` (perpendicular to `axis`: 0 x, 1 y, 2 z): 256 lanes x one float4 (two voxels),
// for colour one uint2 each.  A source brick outside the volume reads as never observed (all-zero bits, zero colour, zero deferred-weight word).
// negbits and the skip tables were cleared up front: only atomicOr here.  Whole-volume contexts only (bz0 == 0: slot == brick index).
template <bool COLOR>
__global__ void __launch_bounds__(256) k_shift_bricks(KfVolume v, int axis, int plane, int sx, int sy, int sz) {
  __shared__ unsigned s_f[2][4];                         // the four waves' flags, double-buffered by iteration: one barrier per brick
  const unsigned nb = (unsigned)v.nb, n = nb * nb;
  const unsigned wave = threadIdx.x >> 6;
  unsigned par = 0;
  for (unsigned i = blockIdx.x; i < n; i += gridDim.x, par ^= 1u) {
    const int u = (int)(i / nb), w = (int)(i % nb);
    const int bx = axis == 0 ? plane : w, by = axis == 1 ? plane : (axis == 0 ? w : u), bz = axis == 2 ? plane : u;
    const int qx = bx + sx, qy = by + sy, qz = bz + sz;
    const bool in = (unsigned)qx < nb && (unsigned)qy < nb && (unsigned)qz < nb;          // (workgroup-uniform)
    const size_t dst = ((size_t)bz * nb + (size_t)by) * nb + (size_t)bx;
    const size_t src = in ? ((size_t)qz * nb + (size_t)qy) * nb + (size_t)qx : dst;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    uint2 cc = make_uint2(0u, 0u);
    if (in) {
      q = reinterpret_cast<const float4*>(v.tw + src * KF_BRICK_VOX)[threadIdx.x];
      if (COLOR) cc = reinterpret_cast<const uint2*>(v.color + src * KF_BRICK_VOX)[threadIdx.x];
    }
    reinterpret_cast<float4*>(v.tw + dst * KF_BRICK_VOX)[threadIdx.x] = q;
    if (COLOR) reinterpret_cast<uint2*>(v.color + dst * KF_BRICK_VOX)[threadIdx.x] = cc;
    const unsigned f = (__ballot(q.y > 0.f || q.w > 0.f) ? KF_FLAG_OBSERVED : 0u) | (__ballot(q.x < 0.f || q.z < 0.f) ? KF_FLAG_HASNEG : 0u);
    if ((threadIdx.x & 63u) == 0u) s_f[par][wave] = f;
    __syncthreads();
    if (threadIdx.x == 0) {
      const unsigned fl = s_f[par][0] | s_f[par][1] | s_f[par][2] | s_f[par][3];
      v.pend[dst] = in ? v.pend[src] : 0ull;             // the deferred-weight word travels with its brick (flushed: 0, 1 or KF_PEND_SAT per quarter)
      v.flags[dst] = (uint8_t)fl;
      if (fl & KF_FLAG_HASNEG) {
        atomicOr(&v.negbits[dst >> 5], 1u << (dst & 31));
        kf_mark_macro(v, bx, by, bz);
      }
    }
  }
}

// The device-resident pose moves with the contents: t <- t - (float)d * cell, one rounded fp32 operation each (the library is built without
// contraction), and the inverse is recomputed as every other committer of the pose does.  cur[0] and last_inv are rebuilt from the pose at the
// start of every tracking call; they are restated here so that nothing in KfTrackState describes the old window.  The verdict is left alone.
__global__ void k_shift_pose(KfTrackState* st, int dx, int dy, int dz, float cell) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  st->pose[3] = st->pose[3] - (float)dx * cell;
  st->pose[7] = st->pose[7] - (float)dy * cell;
  st->pose[11] = st->pose[11] - (float)dz * cell;
  kf_mat44_inverse(st->pose, st->pose_inv);
  for (int i = 0; i < 16; ++i) { st->cur[0][i] = st->pose[i]; st->last_inv[i] = st->pose_inv[i]; }
}

// Stream-out (kf_set_stream_out): the cells whose 27 voxels include a voxel that is about to leave, as up to three disjoint boxes -- the x strip
// in full, the y strip without the x strip, the z strip without both.  Along one axis with d > 0 voxels < d leave: cells [0, d + 1); with d < 0
// cells [res + d - 1, res).  The same few lines as hkf_departing_boxes of the host library (this library does not link it).
static int departing_boxes(const int32_t d[3], int res, int32_t lo[3][3], int32_t hi[3][3]) {
  int32_t slo[3], shi[3], klo[3], khi[3];                  // per axis: the strip, and what is left of the axis without it
  for (int k = 0; k < 3; ++k) {
    const int64_t dd = d[k];
    if (dd > 0) { slo[k] = 0; shi[k] = (int32_t)(dd + 1 > res ? res : dd + 1); klo[k] = shi[k]; khi[k] = res; }
    else if (dd < 0) { shi[k] = res; slo[k] = (int32_t)(res + dd - 1 < 0 ? 0 : res + dd - 1); klo[k] = 0; khi[k] = slo[k]; }
    else { slo[k] = shi[k] = 0; klo[k] = 0; khi[k] = res; }
  }
  int n = 0;
  for (int k = 0; k < 3; ++k) {
    if (slo[k] >= shi[k]) continue;
    bool empty = false;
    for (int j = 0; j < 3; ++j) {
      lo[n][j] = j < k ? klo[j] : (j == k ? slo[j] : 0);
      hi[n][j] = j < k ? khi[j] : (j == k ? shi[j] : res);
      if (lo[n][j] >= hi[n][j]) empty = true;
    }
    if (!empty) ++n;
  }
  return n;
}

extern "C" int kf_shift_volume(kf_ctx* c, int32_t dx, int32_t dy, int32_t dz) {
  if (!c) return KF_ERR_ARG;
  if ((dx % KF_BRICK) || (dy % KF_BRICK) || (dz % KF_BRICK)) return KF_ERR_ARG;
  if (dx == 0 && dy == 0 && dz == 0) return 0;
  KfVolume& v = c->vol;
  if (v.bz0 != 0 || v.bz1 != v.nb) return KF_ERR_ARG;     // a z-slab context: a z shift needs a layer exchange between the members of a group
  const int32_t d[3] = {dx, dy, dz};
  int64_t org[3];
  for (int k = 0; k < 3; ++k) { org[k] = (int64_t)c->origin_vox[k] + d[k]; if (org[k] > INT32_MAX || org[k] < INT32_MIN) return KF_ERR_ARG; }
  const bool store = c->bstore.max_bricks != 0;
  if (store) {                                                    // every brick of the old and of the new window needs a key (brick_key.h): refused before anything is touched
    for (int k = 0; k < 3; ++k) {
      const int64_t b_old = c->origin_vox[k] / KF_BRICK, b_new = org[k] / KF_BRICK;
      if (!kf_brick_key_in_range(b_old) || !kf_brick_key_in_range(b_old + v.nb - 1) || !kf_brick_key_in_range(b_new) || !kf_brick_key_in_range(b_new + v.nb - 1)) return KF_ERR_ARG;
    }
  }
  KF_CHECK(hipSetDevice(c->cfg.device));
  // the bookkeeping of a wholesale change, in kf_resize_slab's order
  { const int ds = kf_tail_cull_discard(c); if (ds) return ds; }
  { const int fs = kf_flush_pending(c); if (fs) return fs; }      // the words become 0, 1 or KF_PEND_SAT: they describe voxels that move verbatim
  if (c->stream_on && c->soup) {                                  // before anything moves: the surface that can never be extracted again -> the world soup
    int32_t lo[3][3], hi[3][3];
    const int nbox = departing_boxes(d, v.res, lo, hi);
    for (int b = 0; b < nbox; ++b) {
      const int rs = kf_mc_region_enqueue(c, c->stream_color, c->stream_thr, lo[b], hi[b], KF_MC_WORLD | KF_MC_TO_WORLD_SOUP);
      if (rs) return rs;
    }
  }
  const int sb[3] = {d[0] / KF_BRICK, d[1] / KF_BRICK, d[2] / KF_BRICK};   // the shift in bricks, not clamped: the store's passes clamp their boxes themselves
  if (store) { const int es = kf_brick_store_evict(c, sb, c->origin_vox); if (es) return es; }   // the flushed voxels and words of what leaves, keyed under the OLD origin
  ++c->vol_flags_serial;
  c->wgt0_valid = 0;
  c->model_pyr_ok = 0;                                            // the model maps show the old window: the caller raycasts before the next kf_*_track
  KF_CHECK(hipMemsetAsync(v.macrobits, 0, kf_skip_table_words(v) * sizeof(unsigned), c->stream));
  KF_CHECK(hipMemsetAsync(v.negbits, 0, kf_negbit_words(c->n_stored_bricks) * sizeof(unsigned), c->stream));
  hipLaunchKernelGGL(k_shift_pose, dim3(1), dim3(64), 0, c->stream, c->track, (int)dx, (int)dy, (int)dz, v.cell);
  // brick shifts, clamped to the volume (anything beyond leaves it empty all the same)
  int s[3];
  for (int k = 0; k < 3; ++k) { const int b = d[k] / KF_BRICK; s[k] = b > v.nb ? v.nb : (b < -v.nb ? -v.nb : b); }
  const int axis = s[2] ? 2 : (s[1] ? 1 : 0);
  const unsigned per_plane = (unsigned)v.nb * (unsigned)v.nb;
  const dim3 grid(per_plane > 2048u ? 2048u : per_plane), block(256);
  for (int k = 0; k < v.nb; ++k) {
    const int plane = s[axis] > 0 ? k : v.nb - 1 - k;
    if (v.color) hipLaunchKernelGGL(k_shift_bricks<true>, grid, block, 0, c->stream, v, axis, plane, s[0], s[1], s[2]);
    else hipLaunchKernelGGL(k_shift_bricks<false>, grid, block, 0, c->stream, v, axis, plane, s[0], s[1], s[2]);
  }
  for (int k = 0; k < 3; ++k) c->origin_vox[k] = (int32_t)org[k];
  if (store) { const int rs = kf_brick_store_restore(c, sb, c->origin_vox); if (rs) return rs; }   // what enters, looked up under the NEW origin
  return (int)hipGetLastError();
}

// kf_place_window: the window at any origin, filled from the store.  kf_shift_volume restores only what ENTERS, so a window moved by less than its width onto
// a filled store stays empty where it overlaps its old place.  This call leaves what capture, a shift to a frame that overlaps neither window, and a
// shift from there to (ox, oy, oz) leave: after the capture the store alone is the whole map, the first hop empties the window (everything leaves, already
// captured), the second restores all nb^3 bricks.  Done directly: capture, the shift's clears plus the planes themselves, the pose moved once, the restore
// over one box of all bricks.  No stream-out: the bricks are kept, not lost.
extern "C" int kf_place_window(kf_ctx* c, int32_t ox, int32_t oy, int32_t oz) {
  if (!c) return KF_ERR_ARG;
  if ((ox % KF_BRICK) || (oy % KF_BRICK) || (oz % KF_BRICK)) return KF_ERR_ARG;
  KfVolume& v = c->vol;
  if (v.bz0 != 0 || v.bz1 != v.nb) return KF_ERR_ARG;
  if (!c->bstore.max_bricks) return KF_ERR_STATE;
  const int32_t org[3] = {ox, oy, oz};
  for (int k = 0; k < 3; ++k) {
    const int64_t b_old = c->origin_vox[k] / KF_BRICK, b_new = org[k] / KF_BRICK;
    if (!kf_brick_key_in_range(b_old) || !kf_brick_key_in_range(b_old + v.nb - 1) || !kf_brick_key_in_range(b_new) || !kf_brick_key_in_range(b_new + v.nb - 1)) return KF_ERR_ARG;
  }
  KF_CHECK(hipSetDevice(c->cfg.device));
  // the counts before and after the capture, one blocking read: a brick the capture dropped exists in the window only, so the window stays
  KfBrickStoreCounts* h = (KfBrickStoreCounts*)c->host_pinned;
  KF_CHECK(hipMemcpyAsync(&h[0], c->bstore.cnt, sizeof(KfBrickStoreCounts), hipMemcpyDeviceToHost, c->stream));
  { const int cs = kf_brick_store_capture_enqueue(c); if (cs) return cs; }
  KF_CHECK(hipMemcpyAsync(&h[1], c->bstore.cnt, sizeof(KfBrickStoreCounts), hipMemcpyDeviceToHost, c->stream));
  KF_CHECK(hipStreamSynchronize(c->stream));
  if (h[1].dropped != h[0].dropped) return KF_ERR_ALLOC;         // (the bricks that were captured are harmless copies)
  // kf_shift_volume's bookkeeping and clears; the planes, flags and deferred-weight words as k_shift_bricks leaves a window everything has left
  { const int ds = kf_tail_cull_discard(c); if (ds) return ds; }
  ++c->vol_flags_serial;
  c->wgt0_valid = 0;
  c->model_pyr_ok = 0;
  KF_CHECK(hipMemsetAsync(v.macrobits, 0, kf_skip_table_words(v) * sizeof(unsigned), c->stream));
  KF_CHECK(hipMemsetAsync(v.negbits, 0, kf_negbit_words(c->n_stored_bricks) * sizeof(unsigned), c->stream));
  KF_CHECK(hipMemsetAsync(v.tw, 0, c->n_stored_vox * sizeof(float2), c->stream));
  if (v.color) KF_CHECK(hipMemsetAsync(v.color, 0, c->n_stored_vox * sizeof(uchar4), c->stream));
  KF_CHECK(hipMemsetAsync(v.flags, 0, c->n_stored_bricks, c->stream));
  KF_CHECK(hipMemsetAsync(v.pend, 0, c->n_stored_bricks * sizeof(unsigned long long), c->stream));
  hipLaunchKernelGGL(k_shift_pose, dim3(1), dim3(64), 0, c->stream, c->track, (int)(ox - c->origin_vox[0]), (int)(oy - c->origin_vox[1]), (int)(oz - c->origin_vox[2]), v.cell);
  for (int k = 0; k < 3; ++k) c->origin_vox[k] = org[k];
  const int all[3] = {v.nb, 0, 0};                                // what enters when everything has left: one box of all bricks
  { const int rs = kf_brick_store_restore(c, all, c->origin_vox); if (rs) return rs; }
  return (int)hipGetLastError();
}

extern "C" int kf_volume_origin(kf_ctx* c, int32_t origin_vox[3]) {
  if (!c || !origin_vox) return KF_ERR_ARG;
  for (int k = 0; k < 3; ++k) origin_vox[k] = c->origin_vox[k];
  return 0;
}
