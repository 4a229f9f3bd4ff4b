// shift.hip -- the moving volume: kf_shift_volume slides the TSDF window by whole bricks, in place, on the context's stream; kf_shift_slab is the same move
// for a context that stores brick layers [bz0, bz1) only, with the layers it does not store fed in by their owners; kf_place_window stands the window anywhere.
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
// enter are looked up in it after the move: two more launches around the ones above.
//
// Slab contexts.  A slab group (group.hip: kf_group_shift_volume) packs on every owner (kf_slab_pack_layers), exchanges, then moves on every member
// (kf_shift_slab).  The transit layout of one brick layer (kf_slab_layer_bytes, n = nb * nb bricks, brick (bx, by) at index by * nb + bx):
//   [n x 4 KiB (tsdf, weight)] [n x 2 KiB colour, on a context with a colour plane] [n x 8 B deferred-weight words, padded to 16 B]
// every brick verbatim as it lies in the volume, so a pack and a move are streaming copies of whole bricks.  Layers follow each other at that pitch.
// The rule of the move: stored destination brick (bx, by, p) takes source brick (bx + sx, by + sy, p + sz) -- from this context's own copy where layer
// p + sz is stored here (halo layers hold their owner's bits, which kf_resize_slab already relies on), else from the feed where the layer lies in the
// feed range, else it reads as never observed; so does a source whose x or y lies outside.  The feed is a buffer of its own, so only the context's own
// planes need the safe order.  A whole-volume context is the case bz0 == 0, bz1 == nb, no feed, which the move's body knows at compile time.
#include "kf_internal.h"
#include "brick_key.h"
#include "strip_boxes.h"
#include <stdint.h>

struct KfSlabFeed {
  const unsigned char* base;   // the feed / pack buffer (layer f0 first)
  int f0, f1;                  // brick layers it holds
  size_t pitch, color_off, pend_off;   // bytes of one layer; where the colours and the words of a layer begin
};

static inline size_t slab_pend_bytes(size_t n) { return (n * sizeof(unsigned long long) + 15) & ~(size_t)15; }
static KfSlabFeed slab_feed(const KfVolume& v, const void* base, int f0, int f1) {
  const size_t n = (size_t)v.nb * v.nb;
  KfSlabFeed f;
  f.base = (const unsigned char*)base; f.f0 = f0; f.f1 = f1;
  f.color_off = n * KF_BRICK_VOX * sizeof(float2);
  f.pend_off = f.color_off + (v.color ? n * KF_BRICK_VOX * sizeof(uchar4) : 0);
  f.pitch = f.pend_off + slab_pend_bytes(n);
  return f;
}

// stored layers [b0, b0 + layers) into the transit layout: one workgroup iteration per brick, 256 lanes x one float4 (colour: one uint2)
template <bool COLOR>
__global__ void __launch_bounds__(256) k_slab_pack(KfVolume v, KfSlabFeed f, int b0, unsigned layers) {
  const unsigned n = (unsigned)v.nb * (unsigned)v.nb, total = layers * n;
  for (unsigned i = blockIdx.x; i < total; i += gridDim.x) {
    const unsigned l = i / n, k = i % n;
    const size_t src = (size_t)(b0 - v.bz0 + (int)l) * n + k;
    unsigned char* lay = const_cast<unsigned char*>(f.base) + (size_t)l * f.pitch;
    reinterpret_cast<float4*>(lay + (size_t)k * (KF_BRICK_VOX * sizeof(float2)))[threadIdx.x] = reinterpret_cast<const float4*>(v.tw + src * KF_BRICK_VOX)[threadIdx.x];
    if (COLOR)
      reinterpret_cast<uint2*>(lay + f.color_off + (size_t)k * (KF_BRICK_VOX * sizeof(uchar4)))[threadIdx.x] = reinterpret_cast<const uint2*>(v.color + src * KF_BRICK_VOX)[threadIdx.x];
    if (threadIdx.x == 0) reinterpret_cast<unsigned long long*>(lay + f.pend_off)[k] = v.pend[src];
  }
}

// The brick move.  One workgroup iteration moves one brick of brick plane `plane` (perpendicular to `axis`: 0 x, 1 y, 2 z): 256 lanes x one float4 (two
// voxels), for colour one uint2 each; a z plane has nb x nb bricks, an x or y plane nb x (stored layers).  The source is workgroup-uniform: the own volume,
// the feed, or nothing -- a brick that reads as never observed (all-zero bits, zero colour, zero deferred-weight word).  SLAB == false: the stored layers are
// [0, nb) and there is no feed, both known to the compiler (f is not read).
template <bool COLOR, bool SLAB>
__device__ __forceinline__ void shift_bricks(const KfVolume& v, const KfSlabFeed& f, int axis, int plane, int sx, int sy, int sz) {
  __shared__ unsigned s_f[2][4];                         // the four waves' flags, double-buffered by iteration: one barrier per brick
  const unsigned nb = (unsigned)v.nb;
  const int bz0 = SLAB ? v.bz0 : 0, bz1 = SLAB ? v.bz1 : (int)nb;
  const unsigned n = nb * (axis == 2 ? nb : (unsigned)(bz1 - bz0));
  const unsigned wave = threadIdx.x >> 6;
  unsigned par = 0;
  for (unsigned i = blockIdx.x; i < n; i += gridDim.x, par ^= 1u) {
    const int u = (int)(i / nb), w = (int)(i % nb);      // u: y of a z plane, else the stored layer
    const int bx = axis == 0 ? plane : w, by = axis == 1 ? plane : (axis == 0 ? w : u), bz = axis == 2 ? plane : u + bz0;
    const int qx = bx + sx, qy = by + sy, qz = bz + sz;
    const bool in_xy = (unsigned)qx < nb && (unsigned)qy < nb;
    const bool own = in_xy && (unsigned)(qz - bz0) < (unsigned)(bz1 - bz0), fed = SLAB && in_xy && !own && qz >= f.f0 && qz < f.f1;          // (workgroup-uniform)
    const size_t dst = ((size_t)(bz - bz0) * nb + (size_t)by) * nb + (size_t)bx;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    uint2 cc = make_uint2(0u, 0u);
    const unsigned long long* pp = nullptr;              // the deferred-weight word travels with its brick (flushed: 0, 1 or KF_PEND_SAT per quarter)
    if (own) {
      const size_t src = ((size_t)(qz - bz0) * nb + (size_t)qy) * nb + (size_t)qx;
      q = reinterpret_cast<const float4*>(v.tw + src * KF_BRICK_VOX)[threadIdx.x];
      if (COLOR) cc = reinterpret_cast<const uint2*>(v.color + src * KF_BRICK_VOX)[threadIdx.x];
      pp = v.pend + src;
    } else if (fed) {
      const unsigned char* lay = f.base + (size_t)(qz - f.f0) * f.pitch;
      const size_t qi = (size_t)qy * nb + (size_t)qx;    // the source brick inside its layer
      q = reinterpret_cast<const float4*>(lay + qi * (KF_BRICK_VOX * sizeof(float2)))[threadIdx.x];
      if (COLOR) cc = reinterpret_cast<const uint2*>(lay + f.color_off + qi * (KF_BRICK_VOX * sizeof(uchar4)))[threadIdx.x];
      pp = reinterpret_cast<const unsigned long long*>(lay + f.pend_off) + qi;
    }
    // When thread 0 loads the word is the one thing the forms do not share: the slab form with the voxels (after the barrier an x walk over a slab's few
    // layers measured 6 % slower), the whole-volume form after the barrier, as it always did (before it the word costs the kernel two more VGPRs).
    unsigned long long pw = 0ull;
    if (SLAB && threadIdx.x == 0 && pp) pw = *pp;
    reinterpret_cast<float4*>(v.tw + dst * KF_BRICK_VOX)[threadIdx.x] = q;
    if (COLOR) reinterpret_cast<uint2*>(v.color + dst * KF_BRICK_VOX)[threadIdx.x] = cc;
    const unsigned fw = (__ballot(q.y > 0.f || q.w > 0.f) ? KF_FLAG_OBSERVED : 0u) | (__ballot(q.x < 0.f || q.z < 0.f) ? KF_FLAG_HASNEG : 0u);
    if ((threadIdx.x & 63u) == 0u) s_f[par][wave] = fw;
    __syncthreads();
    if (threadIdx.x == 0) {
      const unsigned fl = s_f[par][0] | s_f[par][1] | s_f[par][2] | s_f[par][3];
      if (!SLAB && own) pw = *pp;
      kf_restate_brick(v, dst, bx, by, bz, pw, fl);
    }
  }
}
// the two launch forms: a whole-volume context passes no feed (kf_shift_volume's speed rests on this form), a slab context its stored range and the feed
template <bool COLOR>
__global__ void __launch_bounds__(256) k_shift_bricks(KfVolume v, int axis, int plane, int sx, int sy, int sz) {
  shift_bricks<COLOR, false>(v, KfSlabFeed{}, axis, plane, sx, sy, sz);
}
template <bool COLOR>
__global__ void __launch_bounds__(256) k_shift_slab_bricks(KfVolume v, KfSlabFeed f, int axis, int plane, int sx, int sy, int sz) {
  shift_bricks<COLOR, true>(v, f, axis, plane, sx, sy, sz);
}

// The device-resident pose moves with the contents (kf_shift_translation), and the inverse is recomputed as every other committer of the pose does.
// cur[0] and last_inv are rebuilt from the pose at the start of every tracking call; they are restated here so that nothing in KfTrackState describes
// the old window.  The verdict is left alone.
__global__ void k_shift_pose(KfTrackState* st, int dx, int dy, int dz, float cell) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  kf_shift_translation(st->pose, st->pose, dx, dy, dz, cell);
  kf_mat44_inverse(st->pose, st->pose_inv);
  for (int i = 0; i < 16; ++i) { st->cur[0][i] = st->pose[i]; st->last_inv[i] = st->pose_inv[i]; }
}

// ---- the host path of "the window's contents change", shared by kf_shift_volume, kf_shift_slab and kf_place_window ---------------------------------------
// the origin after a move by d, or false where it leaves 32 bits
static bool moved_origin(const kf_ctx* c, const int32_t d[3], int32_t org[3]) {
  for (int k = 0; k < 3; ++k) {
    const int64_t o = (int64_t)c->origin_vox[k] + d[k];
    if (o > INT32_MAX || o < INT32_MIN) return false;
    org[k] = (int32_t)o;
  }
  return true;
}

// The bookkeeping of a wholesale change, in kf_resize_slab's order, past the caller's tail-cull discard and flush: the serial, the tables cleared for the
// atomicOrs to come, the pose moved by d.  `empty`: the window itself is cleared too, to what the move leaves of a window everything has left (kf_place_window).
// d == nullptr: the window stays where it is (kf_refill_window) -- no pose move, not even by zero: the pose and its inverse are not written at all.
static int window_change(kf_ctx* c, const int32_t* d, bool empty) {
  KfVolume& v = c->vol;
  ++c->vol_flags_serial;
  c->wgt0_valid = 0;
  c->model_pyr_ok = 0;                                            // the model maps show the old window: the caller raycasts before the next kf_*_track
  KF_CHECK(hipMemsetAsync(v.macrobits, 0, kf_skip_table_words(v) * sizeof(unsigned), c->stream));
  KF_CHECK(hipMemsetAsync(v.negbits, 0, kf_negbit_words(c->n_stored_bricks) * sizeof(unsigned), c->stream));
  if (empty) {
    KF_CHECK(hipMemsetAsync(v.tw, 0, c->n_stored_vox * sizeof(float2), c->stream));
    if (v.color) KF_CHECK(hipMemsetAsync(v.color, 0, c->n_stored_vox * sizeof(uchar4), c->stream));
    KF_CHECK(hipMemsetAsync(v.flags, 0, c->n_stored_bricks, c->stream));
    KF_CHECK(hipMemsetAsync(v.pend, 0, c->n_stored_bricks * sizeof(unsigned long long), c->stream));
  }
  if (d) hipLaunchKernelGGL(k_shift_pose, dim3(1), dim3(64), 0, c->stream, c->track, (int)d[0], (int)d[1], (int)d[2], v.cell);
  return 0;
}

// The plane walk of a move by d voxels: the brick shift clamped to the volume (anything beyond leaves it empty all the same), the planes perpendicular to
// the first non-zero axis among z, y, x in the safe order -- the stored planes for a z walk, else all nb.  f == nullptr: a whole-volume context moved by
// kf_shift_volume, the form without a feed; kf_shift_slab always brings a feed (empty on a context that stores every layer) and launches the slab form.
static void walk_planes(kf_ctx* c, const int32_t d[3], const KfSlabFeed* f) {
  const KfVolume& v = c->vol;
  int s[3];
  for (int k = 0; k < 3; ++k) { const int b = d[k] / KF_BRICK; s[k] = b > v.nb ? v.nb : (b < -v.nb ? -v.nb : b); }
  const int axis = s[2] ? 2 : (s[1] ? 1 : 0);
  const int lo = axis == 2 ? v.bz0 : 0, hi = axis == 2 ? v.bz1 : v.nb;
  const unsigned per_plane = (unsigned)v.nb * (unsigned)(axis == 2 ? v.nb : v.bz1 - v.bz0);
  const dim3 grid(per_plane > 2048u ? 2048u : per_plane), block(256);
  for (int k = 0; k < hi - lo; ++k) {
    const int plane = s[axis] > 0 ? lo + k : hi - 1 - k;
    if (!f) {
      if (v.color) hipLaunchKernelGGL(k_shift_bricks<true>, grid, block, 0, c->stream, v, axis, plane, s[0], s[1], s[2]);
      else hipLaunchKernelGGL(k_shift_bricks<false>, grid, block, 0, c->stream, v, axis, plane, s[0], s[1], s[2]);
    } else {
      if (v.color) hipLaunchKernelGGL(k_shift_slab_bricks<true>, grid, block, 0, c->stream, v, *f, axis, plane, s[0], s[1], s[2]);
      else hipLaunchKernelGGL(k_shift_slab_bricks<false>, grid, block, 0, c->stream, v, *f, axis, plane, s[0], s[1], s[2]);
    }
  }
}

extern "C" int kf_shift_volume(kf_ctx* c, int32_t dx, int32_t dy, int32_t dz) {
  if (!c) return KF_ERR_ARG;
  if ((dx % KF_BRICK) || (dy % KF_BRICK) || (dz % KF_BRICK)) return KF_ERR_ARG;
  if (dx == 0 && dy == 0 && dz == 0) return 0;
  KfVolume& v = c->vol;
  if (!kf_whole_volume(c)) return KF_ERR_ARG;     // a z-slab context: a z shift needs a layer exchange between the members of a group
  const int32_t d[3] = {dx, dy, dz};
  int32_t org[3];
  if (!moved_origin(c, d, org)) return KF_ERR_ARG;
  const bool store = c->bstore.max_bricks != 0;                   // every brick of the old and of the new window needs a key: refused before anything is touched
  if (store && (!kf_window_in_key_range(c->origin_vox, v.nb) || !kf_window_in_key_range(org, v.nb))) return KF_ERR_ARG;
  KF_CHECK(hipSetDevice(c->cfg.device));
  { const int ds = kf_tail_cull_discard(c); if (ds) return ds; }
  { const int fs = kf_flush_pending(c); if (fs) return fs; }      // the words become 0, 1 or KF_PEND_SAT: they describe voxels that move verbatim
  if (c->stream_on && c->soup) {                                  // before anything moves: the surface that can never be extracted again -> the world soup
    int32_t lo[3][3], hi[3][3];                                   // the cells whose 27 voxels include a voxel that is about to leave (hkf_departing_boxes' boxes)
    const int nbox = kf_strip_boxes(dx, dy, dz, v.res, 1, lo, hi);
    for (int b = 0; b < nbox; ++b) {
      const int rs = kf_mc_region_enqueue(c, c->stream_color, c->stream_thr, lo[b], hi[b], KF_MC_WORLD | KF_MC_TO_WORLD_SOUP);
      if (rs) return rs;
    }
  }
  const int sb[3] = {d[0] / KF_BRICK, d[1] / KF_BRICK, d[2] / KF_BRICK};   // the shift in bricks, not clamped: the store's passes clamp their boxes themselves
  if (store) { const int es = kf_brick_store_evict(c, sb, c->origin_vox); if (es) return es; }   // the flushed voxels and words of what leaves, keyed under the OLD origin
  { const int ws = window_change(c, d, false); if (ws) return ws; }
  walk_planes(c, d, nullptr);
  for (int k = 0; k < 3; ++k) c->origin_vox[k] = org[k];
  if (store) { const int rs = kf_brick_store_restore(c, sb, c->origin_vox); if (rs) return rs; }   // what enters, looked up under the NEW origin
  return (int)hipGetLastError();
}

// kf_place_window: the window at any origin, filled from the store.  kf_shift_volume restores only what ENTERS, so a window moved by less than its width onto
// a filled store stays empty where it overlaps its old place.  This call leaves what capture, a shift to a frame that overlaps neither window, and a
// shift from there to (ox, oy, oz) leave: after the capture the store alone is the whole map, the first hop empties the window (everything leaves, already
// captured), the second restores all nb^3 bricks.  Done directly: capture, the window's change to an empty one with the pose moved once, the restore
// over one box of all bricks.  No stream-out: the bricks are kept, not lost.
extern "C" int kf_place_window(kf_ctx* c, int32_t ox, int32_t oy, int32_t oz) {
  if (!c) return KF_ERR_ARG;
  if ((ox % KF_BRICK) || (oy % KF_BRICK) || (oz % KF_BRICK)) return KF_ERR_ARG;
  KfVolume& v = c->vol;
  if (!kf_whole_volume(c)) return KF_ERR_ARG;
  if (!c->bstore.max_bricks) return KF_ERR_STATE;
  const int32_t org[3] = {ox, oy, oz};
  if (!kf_window_in_key_range(c->origin_vox, v.nb) || !kf_window_in_key_range(org, v.nb)) return KF_ERR_ARG;
  KF_CHECK(hipSetDevice(c->cfg.device));
  // the counts before and after the capture, one blocking read: a brick the capture dropped exists in the window only, so the window stays
  KfBrickStoreCounts* h = (KfBrickStoreCounts*)c->host_pinned;
  KF_CHECK(hipMemcpyAsync(&h[0], c->bstore.cnt, sizeof(KfBrickStoreCounts), hipMemcpyDeviceToHost, c->stream));
  { const int cs = kf_brick_store_capture_enqueue(c); if (cs) return cs; }   // (flushes the pending weights)
  KF_CHECK(hipMemcpyAsync(&h[1], c->bstore.cnt, sizeof(KfBrickStoreCounts), hipMemcpyDeviceToHost, c->stream));
  KF_CHECK(hipStreamSynchronize(c->stream));
  if (h[1].dropped != h[0].dropped) return KF_ERR_ALLOC;         // (the bricks that were captured are harmless copies)
  { const int ds = kf_tail_cull_discard(c); if (ds) return ds; }
  const int32_t d[3] = {ox - c->origin_vox[0], oy - c->origin_vox[1], oz - c->origin_vox[2]};   // (both inside the key range: no overflow)
  { const int ws = window_change(c, d, true); if (ws) return ws; }
  for (int k = 0; k < 3; ++k) c->origin_vox[k] = org[k];
  const int all[3] = {v.nb, 0, 0};                                // what enters when everything has left: one box of all bricks
  { const int rs = kf_brick_store_restore(c, all, c->origin_vox); if (rs) return rs; }
  return (int)hipGetLastError();
}

// kf_refill_window: kf_place_window at the current origin with the capture left out -- the window is re-read from the store as the store is NOW.  That is
// what a merge into the store needs (kf_merge_brick_store): a key inside the window is shadowed by the window's copy, and kf_place_window would capture
// that stale copy over the merged slot before it refills.  The window does not move, so the pose is not touched; a brick the store does not hold reads as
// never observed afterwards.  Asynchronous: no allocation, no synchronisation, no read-back.
extern "C" int kf_refill_window(kf_ctx* c) {
  if (!c) return KF_ERR_ARG;
  KfVolume& v = c->vol;
  if (!kf_whole_volume(c)) return KF_ERR_ARG;
  if (!c->bstore.max_bricks) return KF_ERR_STATE;
  if (!kf_window_in_key_range(c->origin_vox, v.nb)) return KF_ERR_ARG;
  KF_CHECK(hipSetDevice(c->cfg.device));
  { const int ds = kf_tail_cull_discard(c); if (ds) return ds; }
  { const int ws = window_change(c, nullptr, true); if (ws) return ws; }   // (the deferred-weight words are cleared with the planes: nothing to flush)
  const int all[3] = {v.nb, 0, 0};
  { const int rs = kf_brick_store_restore(c, all, c->origin_vox); if (rs) return rs; }
  return (int)hipGetLastError();
}

extern "C" int kf_volume_origin(kf_ctx* c, int32_t origin_vox[3]) {
  if (!c || !origin_vox) return KF_ERR_ARG;
  for (int k = 0; k < 3; ++k) origin_vox[k] = c->origin_vox[k];
  return 0;
}

// ---- slab contexts -------------------------------------------------------------------------------------------------------------------------------------
// the source layers p + sz of the stored destination layers p in [b0, b1) that lie in the volume and are not stored there: one range, possibly empty (0, 0)
static void slab_needs(int nb, int b0, int b1, int32_t dz, int* n0, int* n1) {
  int sz = dz / KF_BRICK;
  sz = sz > nb ? nb : (sz < -nb ? -nb : sz);
  int lo = b0 + sz, hi = b1 + sz;
  if (sz > 0) lo = lo > b1 ? lo : b1;                    // what overlaps the stored range is read there
  if (sz < 0) hi = hi < b0 ? hi : b0;
  lo = lo < 0 ? 0 : lo; hi = hi > nb ? nb : hi;
  if (sz == 0 || lo >= hi) lo = hi = 0;
  *n0 = lo; *n1 = hi;
}

extern "C" int kf_slab_needs(uint32_t resolution, uint32_t stored_z_begin, uint32_t stored_z_end, int32_t dz, uint32_t* bz_begin, uint32_t* bz_end) {
  if (!bz_begin || !bz_end || resolution == 0 || (resolution % KF_BRICK) || (dz % KF_BRICK)) return KF_ERR_ARG;
  if ((stored_z_begin % KF_BRICK) || (stored_z_end % KF_BRICK) || stored_z_begin >= stored_z_end || stored_z_end > resolution) return KF_ERR_ARG;
  int b0, b1;
  slab_needs((int)(resolution / KF_BRICK), (int)(stored_z_begin / KF_BRICK), (int)(stored_z_end / KF_BRICK), dz, &b0, &b1);
  *bz_begin = (uint32_t)b0; *bz_end = (uint32_t)b1;
  return 0;
}

extern "C" size_t kf_slab_layer_bytes(kf_ctx* c) {
  if (!c) return 0;
  return slab_feed(c->vol, nullptr, 0, 0).pitch;
}

extern "C" int kf_slab_shift_needs(kf_ctx* c, int32_t dz, uint32_t* bz_begin, uint32_t* bz_end) {
  if (!c || !bz_begin || !bz_end || (dz % KF_BRICK)) return KF_ERR_ARG;
  int b0, b1;
  slab_needs(c->vol.nb, c->vol.bz0, c->vol.bz1, dz, &b0, &b1);
  *bz_begin = (uint32_t)b0; *bz_end = (uint32_t)b1;
  return 0;
}

extern "C" int kf_slab_pack_layers(kf_ctx* c, uint32_t bz_begin, uint32_t bz_end, void* dev_dst) {
  if (!c || !dev_dst) return KF_ERR_ARG;
  const KfVolume& v = c->vol;
  if (bz_begin >= bz_end || (int64_t)bz_begin < v.bz0 || (int64_t)bz_end > v.bz1) return KF_ERR_ARG;
  KF_CHECK(hipSetDevice(c->cfg.device));
  { const int fs = kf_flush_pending(c); if (fs) return fs; }      // the words become states: the bytes do not depend on how the weights were split
  const KfSlabFeed f = slab_feed(v, dev_dst, (int)bz_begin, (int)bz_end);
  const unsigned layers = bz_end - bz_begin;
  const size_t total = (size_t)layers * v.nb * v.nb;
  const dim3 grid((unsigned)(total > 2048 ? 2048 : total)), block(256);
  if (v.color) hipLaunchKernelGGL(k_slab_pack<true>, grid, block, 0, c->stream, v, f, (int)bz_begin, layers);
  else hipLaunchKernelGGL(k_slab_pack<false>, grid, block, 0, c->stream, v, f, (int)bz_begin, layers);
  return (int)hipGetLastError();
}

extern "C" int kf_shift_slab(kf_ctx* c, int32_t dx, int32_t dy, int32_t dz, const void* dev_feed, uint32_t feed_bz_begin, uint32_t feed_bz_end) {
  if (!c) return KF_ERR_ARG;
  if ((dx % KF_BRICK) || (dy % KF_BRICK) || (dz % KF_BRICK)) return KF_ERR_ARG;
  KfVolume& v = c->vol;
  int need0, need1;
  slab_needs(v.nb, v.bz0, v.bz1, dz, &need0, &need1);
  if (need0 < need1 ? ((int64_t)feed_bz_begin != need0 || (int64_t)feed_bz_end != need1 || !dev_feed) : feed_bz_begin != feed_bz_end) return KF_ERR_ARG;
  const int32_t d[3] = {dx, dy, dz};
  int32_t org[3];
  if (!moved_origin(c, d, org)) return KF_ERR_ARG;
  if (c->bstore.max_bricks != 0 || c->stream_on) return KF_ERR_STATE;   // brick store and stream-out stay whole-volume features (kf_shift_volume)
  if (dx == 0 && dy == 0 && dz == 0) return 0;
  KF_CHECK(hipSetDevice(c->cfg.device));
  { const int ds = kf_tail_cull_discard(c); if (ds) return ds; }
  { const int fs = kf_flush_pending(c); if (fs) return fs; }      // the words become 0, 1 or KF_PEND_SAT: they describe voxels that move verbatim
  { const int ws = window_change(c, d, false); if (ws) return ws; }
  const KfSlabFeed f = slab_feed(v, need0 < need1 ? dev_feed : nullptr, need0, need1);
  walk_planes(c, d, &f);
  for (int k = 0; k < 3; ++k) c->origin_vox[k] = org[k];
  if (need0 < need1) c->pend_live = 1;                            // the fed bricks brought their owner's words: they may be set, whatever ran here
  return (int)hipGetLastError();
}
