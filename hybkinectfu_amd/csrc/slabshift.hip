// slabshift.hip -- the moving volume on z-slab contexts: kf_shift_slab is kf_shift_volume's move for a context that stores brick layers [bz0, bz1), with
// the brick layers it does not store fed in by their owners (kf_slab_pack_layers on the owner, kf_shift_slab's feed buffer here).  A slab group
// (group.hip: kf_group_shift_volume) packs on every owner, exchanges, then moves on every member.  No reference counterpart, as for shift.hip.
//
// The transit layout of one brick layer (kf_slab_layer_bytes, n = nb * nb bricks, brick (bx, by) at index by * nb + bx):
//   [n x 4 KiB (tsdf, weight)] [n x 2 KiB colour, on a context with a colour plane] [n x 8 B deferred-weight words, padded to 16 B]
// every brick verbatim as it lies in the volume, so a pack and a move are streaming copies of whole bricks.  Layers follow each other at that pitch.
//
// The rule of the move: stored destination brick (bx, by, p) takes source brick (bx + sx, by + sy, p + sz) -- from this context's own copy where layer
// p + sz is stored here (halo layers hold their owner's bits, which kf_resize_slab already relies on), else from the feed where the layer lies in the
// feed range, else it reads as never observed; so does a source whose x or y lies outside.  In place and plane by plane in the safe order, as in
// shift.hip; the feed is a buffer of its own, so only the context's own planes need the order.
// shift.hip and its kernels stay as they are: this file has its own kernels.
#include "kf_internal.h"
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

// k_shift_bricks (shift.hip) for stored layers [bz0, bz1): one workgroup iteration moves one brick of brick plane `plane` perpendicular to `axis`;
// a z plane has nb x nb bricks, an x or y plane nb x (bz1 - bz0).  The source is workgroup-uniform: own volume, feed, or nothing.
template <bool COLOR>
__global__ void __launch_bounds__(256) k_shift_slab_bricks(KfVolume v, KfSlabFeed f, int axis, int plane, int sx, int sy, int sz) {
  __shared__ unsigned s_f[2][4];                         // the four waves' flags, double-buffered by iteration: one barrier per brick
  const unsigned nb = (unsigned)v.nb, n = nb * (axis == 2 ? nb : (unsigned)(v.bz1 - v.bz0));
  const unsigned wave = threadIdx.x >> 6;
  unsigned par = 0;
  for (unsigned i = blockIdx.x; i < n; i += gridDim.x, par ^= 1u) {
    const int u = (int)(i / nb), w = (int)(i % nb);      // u: y of a z plane, else the stored layer
    const int bx = axis == 0 ? plane : w, by = axis == 1 ? plane : (axis == 0 ? w : u), bz = axis == 2 ? plane : u + v.bz0;
    const int qx = bx + sx, qy = by + sy, qz = bz + sz;
    const bool in_xy = (unsigned)qx < nb && (unsigned)qy < nb;
    const bool own = in_xy && qz >= v.bz0 && qz < v.bz1, fed = in_xy && !own && qz >= f.f0 && qz < f.f1;          // (workgroup-uniform)
    const size_t dst = ((size_t)(bz - v.bz0) * nb + (size_t)by) * nb + (size_t)bx;
    const size_t qi = (size_t)qy * nb + (size_t)qx;      // the source brick inside its layer
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    uint2 cc = make_uint2(0u, 0u);
    unsigned long long pw = 0ull;
    if (own) {
      const size_t src = (size_t)(qz - v.bz0) * nb * nb + qi;
      q = reinterpret_cast<const float4*>(v.tw + src * KF_BRICK_VOX)[threadIdx.x];
      if (COLOR) cc = reinterpret_cast<const uint2*>(v.color + src * KF_BRICK_VOX)[threadIdx.x];
      if (threadIdx.x == 0) pw = v.pend[src];
    } else if (fed) {
      const unsigned char* lay = f.base + (size_t)(qz - f.f0) * f.pitch;
      q = reinterpret_cast<const float4*>(lay + qi * (KF_BRICK_VOX * sizeof(float2)))[threadIdx.x];
      if (COLOR) cc = reinterpret_cast<const uint2*>(lay + f.color_off + qi * (KF_BRICK_VOX * sizeof(uchar4)))[threadIdx.x];
      if (threadIdx.x == 0) pw = reinterpret_cast<const unsigned long long*>(lay + f.pend_off)[qi];
    }
    reinterpret_cast<float4*>(v.tw + dst * KF_BRICK_VOX)[threadIdx.x] = q;
    if (COLOR) reinterpret_cast<uint2*>(v.color + dst * KF_BRICK_VOX)[threadIdx.x] = cc;
    const unsigned fw = (__ballot(q.y > 0.f || q.w > 0.f) ? KF_FLAG_OBSERVED : 0u) | (__ballot(q.x < 0.f || q.z < 0.f) ? KF_FLAG_HASNEG : 0u);
    if ((threadIdx.x & 63u) == 0u) s_f[par][wave] = fw;
    __syncthreads();
    if (threadIdx.x == 0) {
      const unsigned fl = s_f[par][0] | s_f[par][1] | s_f[par][2] | s_f[par][3];
      v.pend[dst] = pw;                                  // the deferred-weight word travels with its brick (flushed: a state, not a count)
      v.flags[dst] = (uint8_t)fl;
      if (fl & KF_FLAG_HASNEG) {
        atomicOr(&v.negbits[dst >> 5], 1u << (dst & 31));
        kf_mark_macro(v, bx, by, bz);
      }
    }
  }
}

// k_shift_pose of shift.hip, restated (a kernel cannot be launched across translation units): the same operations, so the same pose bits
__global__ void k_slab_shift_pose(KfTrackState* st, int dx, int dy, int dz, float cell) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  st->pose[3] = st->pose[3] - (float)dx * cell;
  st->pose[7] = st->pose[7] - (float)dy * cell;
  st->pose[11] = st->pose[11] - (float)dz * cell;
  kf_mat44_inverse(st->pose, st->pose_inv);
  for (int i = 0; i < 16; ++i) { st->cur[0][i] = st->pose[i]; st->last_inv[i] = st->pose_inv[i]; }
}

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
  int64_t org[3];
  for (int k = 0; k < 3; ++k) { org[k] = (int64_t)c->origin_vox[k] + d[k]; if (org[k] > INT32_MAX || org[k] < INT32_MIN) return KF_ERR_ARG; }
  if (c->bstore.max_bricks != 0 || c->stream_on) return KF_ERR_STATE;   // brick store and stream-out stay whole-volume features (kf_shift_volume)
  if (dx == 0 && dy == 0 && dz == 0) return 0;
  KF_CHECK(hipSetDevice(c->cfg.device));
  // the bookkeeping of kf_shift_volume, in its order
  { const int ds = kf_tail_cull_discard(c); if (ds) return ds; }
  { const int fs = kf_flush_pending(c); if (fs) return fs; }      // the words become 0, 1 or KF_PEND_SAT: they describe voxels that move verbatim
  ++c->vol_flags_serial;
  c->wgt0_valid = 0;
  c->model_pyr_ok = 0;                                            // the model maps show the old window: the caller raycasts before the next kf_*_track
  KF_CHECK(hipMemsetAsync(v.macrobits, 0, kf_skip_table_words(v) * sizeof(unsigned), c->stream));
  KF_CHECK(hipMemsetAsync(v.negbits, 0, kf_negbit_words(c->n_stored_bricks) * sizeof(unsigned), c->stream));
  hipLaunchKernelGGL(k_slab_shift_pose, dim3(1), dim3(64), 0, c->stream, c->track, (int)dx, (int)dy, (int)dz, v.cell);
  int s[3];                                                       // brick shifts, clamped to the volume (anything beyond leaves it empty all the same)
  for (int k = 0; k < 3; ++k) { const int b = d[k] / KF_BRICK; s[k] = b > v.nb ? v.nb : (b < -v.nb ? -v.nb : b); }
  const int axis = s[2] ? 2 : (s[1] ? 1 : 0);
  const KfSlabFeed f = slab_feed(v, need0 < need1 ? dev_feed : nullptr, need0, need1);
  const int lo = axis == 2 ? v.bz0 : 0, hi = axis == 2 ? v.bz1 : v.nb;          // the planes of the walk
  const unsigned per_plane = (unsigned)v.nb * (unsigned)(axis == 2 ? v.nb : v.bz1 - v.bz0);
  const dim3 grid(per_plane > 2048u ? 2048u : per_plane), block(256);
  for (int k = 0; k < hi - lo; ++k) {
    const int plane = s[axis] > 0 ? lo + k : hi - 1 - k;
    if (v.color) hipLaunchKernelGGL(k_shift_slab_bricks<true>, grid, block, 0, c->stream, v, f, axis, plane, s[0], s[1], s[2]);
    else hipLaunchKernelGGL(k_shift_slab_bricks<false>, grid, block, 0, c->stream, v, f, axis, plane, s[0], s[1], s[2]);
  }
  for (int k = 0; k < 3; ++k) c->origin_vox[k] = (int32_t)org[k];
  if (need0 < need1) c->pend_live = 1;                            // the fed bricks brought their owner's words: they may be set, whatever ran here
  return (int)hipGetLastError();
}
