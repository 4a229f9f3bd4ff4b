// mapmesh.hip -- meshing the whole map: marching cubes over the brick store and the window together (no reference counterpart: the reference's
// cube never moves, src/HybKinectfu.cpp:51-54, so its one cube IS its map).
//
// kf_marching_cubes_at extracts a box of a VIRTUAL window -- the window as kf_shift_volume would have assembled it at another origin, the store's bricks
// restored -- without moving anything.  The passes are those of kf_marching_cubes_region (mcubes.hip) on the same scratch and the same brick slot numbering
// (the virtual window has the window's shape); what differs is where a brick's voxels come from:
//   resolve : a wave per brick of the box's bricks widened by one.  World brick frame / 8 + b lies in the current window -> the window's copy (the newer
//             one: a restored brick stays in the store as a stale copy); else the store's slot if the key is found; else one shared all-zero brick.  The
//             entry (voxel pointer, colour pointer: 16 bytes) goes into the indirection table, so every gather downstream is an unconditional load through
//             one table entry.  The brick's has-negative bit goes into a bit table over the virtual slots: for a window brick the window's own bit, for a
//             store brick the OR over its voxels, reduced here (what k_store_restore would compute; the store keeps no flags, and k_store_evict stays as it
//             is).  The 4 KiB the wave reads are read again by the class pass of the same call, out of the cache.
//   bricks, codes, sift, list, count, scan, emit, finish : mc_kernels.h, compiled a second time in this file with the addressing hooks redefined: the
//             class pass and the gathers of a cell's evaluation go through the table, the brick tests read the virtual has-negative bits.
// The 3x3x3 brick test sees only the has-negative bits of the widened box (the table is cleared first and only resolved bricks set a bit).  That is enough: a
// cell of the box yields a triangle only with a negative voxel among its 27, that voxel's brick N lies in the widened box, and every brick the cell touches is a
// neighbour of N -- so it is listed for the class pass.  A brick listed on the real window only because of a brick two outside the box has its classes written
// as zeros here, which is the verdict "no triangle" its cells get either way.  Hence voxels are read from resolved bricks of the widened box only.
//
// The deferred-weight words are not consulted and not flushed: the extraction asks of a weight only whether it is zero (k_mc_codes, kf_interp_finish,
// kf_interpolate_color), and a quarter brick with a pending count holds stored weights >= 1 (kf_pend_weight), so flushing -- as the shift would -- changes no answer.
#include "kf_internal.h"
#include "scan.h"
#include "brick_key.h"
#include "brick_find.h"
#include "map_tiles.h"
#include "vwindow.h"
#include <stdint.h>
#include <vector>

namespace mapmesh {

// The hooks of mc_kernels.h for the virtual window.  McArgs::vol is the window's KfVolume for its shape (res, nb, cell, size) with `negbits` pointing at the
// VIRTUAL has-negative bits; its voxel, colour and flag pointers are not used by any kernel compiled here.
#define MC_ARGS_EXTRA const McVBrick* vtab; const float2* vzero;
#define MC_BRICK_PRESENT(a, slot) ((a).vtab[slot].tw != (a).vzero)               /* a brick nobody holds reads the zero brick: its classes are zeros without a read */
#define MC_BRICK_TW(a, slot) ((a).vtab[slot].tw)
#define MC_HAS_FLAG(v, slot, mask) (((v).negbits[(slot) >> 5] >> ((slot) & 31u)) & 1u)          /* mask is KF_FLAG_HASNEG wherever the extraction asks */
#define MC_INTERP_LOAD(a, it, q) v_interp_load((a).vtab, (a).vol, it, q)
#define MC_INTERP_COLOR(a, pos, out) v_interp_color((a).vtab, (a).vol, pos, out)
#define MC_REGION_ONLY
#include "mc_kernels.h"

// ---- resolve (vwindow.h: map_resolve_brick, shared with kf_render_view_at) ------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_map_resolve(KfVolume v, KfBrickStore st, McResolve g, McVBrick* __restrict__ vtab, const float2* __restrict__ zero,
                                                     unsigned* __restrict__ vneg) {
  const unsigned n = (unsigned)g.wn[0] * (unsigned)g.wn[1] * (unsigned)g.wn[2];
  const unsigned lane = threadIdx.x & 63u;
  const int nb = v.nb;
  for (unsigned i = blockIdx.x * 4u + (threadIdx.x >> 6); i < n; i += gridDim.x * 4u) {            // a wave per brick: everything up to the reduction is wave-uniform
    const int bx = g.wlo[0] + (int)(i % (unsigned)g.wn[0]), by = g.wlo[1] + (int)((i / (unsigned)g.wn[0]) % (unsigned)g.wn[1]);
    const int bz = g.wlo[2] + (int)(i / ((unsigned)g.wn[0] * (unsigned)g.wn[1]));
    const unsigned vslot = ((unsigned)bz * (unsigned)nb + (unsigned)by) * (unsigned)nb + (unsigned)bx;
    bool neg;
    const McVBrick e = map_resolve_brick(v, st, g, bx, by, bz, zero, lane, neg);
    if (lane == 0) {
      vtab[vslot] = e;
      if (neg) atomicOr(&vneg[vslot >> 5], 1u << (vslot & 31u));
    }
  }
}

static int vtab_scratch(kf_ctx* c) {
  if (c->mc_vtab) return 0;
  void* p = nullptr;
  const hipError_t e = hipMalloc(&p, (size_t)KF_BRICK_VOX * sizeof(float2) + c->n_stored_bricks * sizeof(McVBrick));
  if (e != hipSuccess) { (void)hipGetLastError(); return KF_ERR_ALLOC; }
  const hipError_t m = hipMemsetAsync(p, 0, (size_t)KF_BRICK_VOX * sizeof(float2), c->stream);       // the zero brick; the table is written before it is read
  if (m != hipSuccess) { hipFree(p); return (int)m; }
  c->mc_vtab = p;
  return 0;
}

// kf_marching_cubes_at past its argument checks
static int enqueue_at(kf_ctx* c, int has_color, float thr, const int32_t fo[3], const int32_t lo_in[3], const int32_t hi_in[3], int flags) {
  const KfVolume& v = c->vol;
  const int R = v.res;
  int lo[3], hi[3];
  for (int k = 0; k < 3; ++k) {
    lo[k] = lo_in[k] < 0 ? 0 : (lo_in[k] > R ? R : lo_in[k]);
    hi[k] = hi_in[k] < 0 ? 0 : (hi_in[k] > R ? R : hi_in[k]);
    if (lo[k] >= hi[k]) { c->region_noop = 1; return 0; }    // empty or inverted: nothing to do
  }
  McArgs a;
  a.vol = v; a.has_color = has_color; a.thr = thr;
  a.x0 = lo[0]; a.x1 = hi[0]; a.xa = lo[0] & ~7; a.wx = ((hi[0] + 7) & ~7) - a.xa;
  a.y0 = lo[1]; a.wy = hi[1] - lo[1]; a.z0 = lo[2]; a.z1 = hi[2];
  a.world = (flags & KF_MC_WORLD) ? 1 : 0; a.spread = 1;
  a.woff = make_float3((float)fo[0] * v.cell, (float)fo[1] * v.cell, (float)fo[2] * v.cell);
  const size_t n_cells = (size_t)(a.z1 - a.z0) * (size_t)a.wy * (size_t)a.wx;
  a.n_blocks = (unsigned)((n_cells + 255) / 256);
  if (a.n_blocks > c->mc_blocks_cap) return KF_ERR_STATE;
  { const int st = kf_mc_scratch(c); if (st) return st; }
  KF_CHECK(hipSetDevice(c->cfg.device));
  { const int st = vtab_scratch(c); if (st) return st; }
  mc_scratch_args(c, a);
  const float2* zero = reinterpret_cast<const float2*>(c->mc_vtab);
  McVBrick* vtab = reinterpret_cast<McVBrick*>(reinterpret_cast<char*>(c->mc_vtab) + (size_t)KF_BRICK_VOX * sizeof(float2));
  a.vtab = vtab; a.vzero = zero;
  a.vol.negbits = c->mc_nbr_bits;                            // the virtual has-negative bits live in the whole-volume extraction's neighbourhood bits: a region call never reads those
  a.tris = c->triangles; a.max_tris = c->max_triangles; a.n_held = &c->counters->n_triangles;
  McRegionBricks g; McResolve r;
  unsigned n_w = 1;
  for (int k = 0; k < 3; ++k) {
    g.blo[k] = lo[k] >> 3; g.bhi[k] = ((hi[k] - 1) >> 3) + 1;
    g.wlo[k] = g.blo[k] > 0 ? g.blo[k] - 1 : 0;
    const int whi = g.bhi[k] < v.nb ? g.bhi[k] + 1 : v.nb;
    g.wn[k] = whi - g.wlo[k];
    n_w *= (unsigned)g.wn[k];
    r.wlo[k] = g.wlo[k]; r.wn[k] = g.wn[k];
    r.fb[k] = fo[k] / KF_BRICK; r.ob[k] = c->origin_vox[k] / KF_BRICK;                           // exact: multiples of 8 both
  }
  unsigned* sift_list = c->mc_d1_list + c->n_stored_bricks;
  kf_evt_begin(c, KF_STAGE_MCUBES);
  // the class tables now take rows of another frame: the next whole-volume extraction zeroes them first (region calls trust nothing anyway)
  c->mc_zero_serial = c->vol_flags_serial - 1;
  KF_CHECK(hipMemsetAsync(c->mc_nbr_bits, 0, (c->n_stored_bricks / 32 + 4) * sizeof(unsigned), c->stream));
  hipLaunchKernelGGL(k_mc_region_clear, dim3((a.n_blocks + 1 + 255) / 256), dim3(256), 0, c->stream, c->mc_block_counts, a.n_blocks + 1, c->mc_block_bits,
                     a.n_blocks / 32 + 1, c->mc_list);
  const unsigned walk_all = (unsigned)c->num_cus * 8u, walk = (n_w + 3) / 4 < walk_all ? (n_w + 3) / 4 : walk_all;
  hipLaunchKernelGGL(k_map_resolve, dim3(walk), dim3(256), 0, c->stream, v, c->bstore, r, vtab, zero, c->mc_nbr_bits);
  hipLaunchKernelGGL(k_mc_region_bricks, dim3((n_w + 255) / 256), dim3(256), 0, c->stream, a, g, sift_list, c->mc_list + 4);
  hipLaunchKernelGGL(k_mc_codes, dim3(walk), dim3(256), 0, c->stream, a);
  McArgs s = a; s.d1_list = sift_list; s.n_d1 = c->mc_list + 4;
  hipLaunchKernelGGL(k_mc_sift, dim3(walk), dim3(256), 0, c->stream, s);
  mc_count_and_emit(c, a, &c->counters->n_triangles, nullptr, c->mc_list + 5);
  kf_evt_end(c, KF_STAGE_MCUBES);
  c->region_noop = 0;
  return (int)hipGetLastError();
}

// what both entry points refuse, before anything is touched
static int check_common(kf_ctx* c, int has_color, int flags) {
  if (!c) return KF_ERR_ARG;
  if (flags & ~KF_MC_WORLD) return KF_ERR_ARG;
  if (!kf_whole_volume(c)) return KF_ERR_ARG;                     // a z-slab context, as for kf_shift_volume
  if (!c->triangles || c->max_triangles == 0) return KF_ERR_STATE;
  if (has_color && !c->vol.color) return KF_ERR_STATE;
  return 0;
}

}  // namespace mapmesh

// kf_brick_store_bounds: the componentwise minimum and maximum of the keys of slots [0, held), by one workgroup (the keys are 8 bytes a brick: a store of a
// million bricks is 8 MiB, read once).  out[0..2] min, out[3..5] max (inclusive), out[6] = held.
__global__ void __launch_bounds__(256) k_store_bounds(KfBrickStore st, int32_t* __restrict__ out) {
  __shared__ int32_t s_lo[3][4], s_hi[3][4];
  const unsigned held = st.cnt->held < st.max_bricks ? st.cnt->held : st.max_bricks;
  int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
  for (unsigned i = threadIdx.x; i < held; i += 256u) {
    int32_t xyz[3];
    kf_brick_key_unpack(st.key[i], xyz);
#pragma unroll
    for (int k = 0; k < 3; ++k) { lo[k] = min(lo[k], xyz[k]); hi[k] = max(hi[k], xyz[k]); }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { lo[k] = min(lo[k], __shfl_down(lo[k], off, 64)); hi[k] = max(hi[k], __shfl_down(hi[k], off, 64)); }
    if ((threadIdx.x & 63u) == 0u) { s_lo[k][threadIdx.x >> 6] = lo[k]; s_hi[k][threadIdx.x >> 6] = hi[k]; }
  }
  __syncthreads();
  if (threadIdx.x < 3u) {
    const unsigned k = threadIdx.x;
    out[k] = min(min(s_lo[k][0], s_lo[k][1]), min(s_lo[k][2], s_lo[k][3]));
    out[3 + k] = max(max(s_hi[k][0], s_hi[k][1]), max(s_hi[k][2], s_hi[k][3]));
  }
  if (threadIdx.x == 0) out[6] = (int32_t)held;
}
// (Here and not in brickstore.hip: a kernel added to that file renumbers the local labels of its template kernels, and the listings of the kernels kf_shift_volume
// launches are to stay byte for byte what they were.)
extern "C" int kf_brick_store_bounds(kf_ctx* c, int32_t lo_brick[3], int32_t hi_brick[3]) {
  if (!c || !lo_brick || !hi_brick) return KF_ERR_ARG;
  for (int k = 0; k < 3; ++k) lo_brick[k] = hi_brick[k] = 0;
  if (!c->bstore.max_bricks) return 0;
  KF_CHECK(hipSetDevice(c->cfg.device));
  int32_t* dev = nullptr;
  KF_CHECK(hipMalloc((void**)&dev, 8 * sizeof(int32_t)));
  hipLaunchKernelGGL(k_store_bounds, dim3(1), dim3(256), 0, c->stream, c->bstore, dev);
  hipError_t e = hipMemcpyAsync(c->host_pinned, dev, 8 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  hipFree(dev);
  if (e != hipSuccess) return (int)e;
  const int32_t* h = (const int32_t*)c->host_pinned;
  if (h[6] == 0) return 0;                                   // nothing held: lo == hi
  for (int k = 0; k < 3; ++k) { lo_brick[k] = h[k]; hi_brick[k] = h[3 + k] + 1; }   // half-open
  return 0;
}

extern "C" int kf_marching_cubes_at(kf_ctx* c, int has_color, float thr, const int32_t frame_origin_vox[3], const int32_t lo[3], const int32_t hi[3], int flags) {
  if (!c || !frame_origin_vox || !lo || !hi) return KF_ERR_ARG;
  for (int k = 0; k < 3; ++k) if (frame_origin_vox[k] % KF_BRICK) return KF_ERR_ARG;
  { const int cs = mapmesh::check_common(c, has_color, flags); if (cs) return cs; }
  if (!kf_window_in_key_range(frame_origin_vox, c->vol.nb)) return KF_ERR_ARG;
  return mapmesh::enqueue_at(c, has_color, thr, frame_origin_vox, lo, hi, flags);
}

extern "C" int64_t kf_map_tile_frames(const int32_t store_lo[3], const int32_t store_hi[3], const int32_t origin_vox[3], int32_t res, int32_t* frames, int64_t cap) {
  if (!store_lo || !store_hi || !origin_vox || cap < 0 || (cap > 0 && !frames)) return -1;
  return kf_map_tiles(store_lo, store_hi, origin_vox, res, frames, cap);
}

extern "C" int kf_marching_cubes_map(kf_ctx* c, int has_color, float thr, int flags, uint32_t* n_tiles) {
  if (n_tiles) *n_tiles = 0;
  { const int cs = mapmesh::check_common(c, has_color, flags); if (cs) return cs; }
  const int R = c->vol.res;
  if (R < 32) return KF_ERR_ARG;                             // a tile owns res - 16 cells per axis
  int32_t slo[3], shi[3];
  { const int bs = kf_brick_store_bounds(c, slo, shi); if (bs) return bs; }           // blocks: the one read-back of the call
  const int64_t n = kf_map_tiles(slo, shi, c->origin_vox, R, nullptr, 0);
  if (n < 0 || n > (int64_t)1 << 24) return KF_ERR_ARG;
  std::vector<int32_t> frames((size_t)n * 3);
  kf_map_tiles(slo, shi, c->origin_vox, R, frames.data(), n);
  for (int64_t t = 0; t < n; ++t) if (!kf_window_in_key_range(&frames[3 * t], c->vol.nb)) return KF_ERR_ARG;     // refused before the first tile is enqueued
  const int32_t lo[3] = {KF_MAP_TILE_MARGIN, KF_MAP_TILE_MARGIN, KF_MAP_TILE_MARGIN}, hi[3] = {R - KF_MAP_TILE_MARGIN, R - KF_MAP_TILE_MARGIN, R - KF_MAP_TILE_MARGIN};
  for (int64_t t = 0; t < n; ++t) {
    const int as = mapmesh::enqueue_at(c, has_color, thr, &frames[3 * t], lo, hi, KF_MC_WORLD);
    if (as) return as;
  }
  if (n_tiles) *n_tiles = (uint32_t)n;
  return 0;
}
