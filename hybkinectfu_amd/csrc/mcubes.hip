// mcubes.hip -- marching-cubes iso-surface extraction (reference: extractIsoSurfaceKernel & helpers,
// src/cuda/marchingcube.cu:5-164; tables src/cuda/marchingcube_table.h; MarchingcubeData src/cuda/MarchingcubeData.h).
//
// The reference appends triangles with one global atomicAdd, so its output ORDER is nondeterministic (and its
// check-then-add can overshoot the buffer, marchingcube.cu:29-32).  Here extraction is deterministic and reads voxels only where
// the surface can be:
//   dilate : the bricks with a negative voxel in their 3x3x3 brick neighbourhood (brick flags only) -> a bit per brick and a list;
//   codes  : a 2-bit class per voxel (unobserved / not negative / negative) of the listed bricks, one coalesced pass over them;
//   sift   : a cell whose 27 voxels are all of one class -- or hold an unobserved one -- cannot produce a triangle: one lane
//            decides that for the eight cells of a brick x-row from 27 cached 16-bit loads -> a bit per cell, a bit per 256-cell block;
//   list   : the 256-cell blocks (z, y, x order) that hold a surviving cell, unordered;
//   count  : the surviving cells of the listed blocks, queued into dense waves, evaluated as the reference evaluates a cell
//            (eight trilinear corner lookups) -> per-block triangle count, and a record per cell that holds triangles;
//   scan   : exclusive prefix over ALL blocks in order (three parallel steps);
//   emit   : one lane per record: the cell again, its triangles land at block prefix + offset in the block: a fixed index.
// The canonical order is (z, y, x, k) -- identical for 1 GPU and for concatenated z-slabs.
// The triangle table is packed into 256 x 64-bit words (16 nibbles per case) instead of the reference's 16 KiB int table; the
// 12-bit edge mask is derived from it.
#include "kf_internal.h"
#include "scan.h"

#include "mc_kernels.h"

// extraction scratch: allocated by the first extraction, not by every context (per 4-KiB brick: 128 B of voxel classes + 64 B of sieve bits + 12 B of lists)
// mc_list: [0] block list length, [1] records, [2] overflow, [3] class-pass bricks, [4] sieve bricks of a region, [5] [6] kf_region_work; then the block ids
int kf_mc_scratch(kf_ctx* c) {
  if (c->mc_list) return 0;
  KF_CHECK(hipSetDevice(c->cfg.device));
  // all or nothing: the pointers are committed to the context only once every allocation has succeeded (at 2048^3 the scratch is
  // ~3.3 GB next to 68.7 GB of voxels -- a failure must not leave a half-allocated set behind that the next call would trust)
  size_t recs = c->max_triangles > c->soup_cap ? c->max_triangles : c->soup_cap;
  if (recs == 0) recs = 1;
  const size_t sizes[8] = {(c->mc_blocks_cap + MC_LIST_HEAD) * sizeof(unsigned),                        // list: the head, then the block ids
                           (c->n_stored_bricks / 32 + 4) * sizeof(unsigned),                           // neighbourhood bits
                           ((c->mc_blocks_cap + MC_CHUNK - 1) / MC_CHUNK + 1) * sizeof(unsigned),       // scan partials
                           c->n_stored_bricks * 64 * sizeof(unsigned short),                            // voxel classes
                           c->n_stored_bricks * 64,                                                    // sieve survivors
                           2 * c->n_stored_bricks * sizeof(unsigned),                                  // brick list; behind it a region's sieve list
                           (c->mc_blocks_cap / 32 + 2) * sizeof(unsigned),                             // block bits
                           recs * sizeof(uint2)};                                                      // records: a recorded cell holds >= 1 triangle
  void* got[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  for (int i = 0; i < 8; ++i) {
    const hipError_t e = hipMalloc(&got[i], sizes[i]);
    if (e != hipSuccess) { for (int j = 0; j < i; ++j) hipFree(got[j]); (void)hipGetLastError(); return (int)e; }
  }
  c->mc_list = (unsigned*)got[0]; c->mc_nbr_bits = (unsigned*)got[1]; c->mc_partials = (unsigned*)got[2]; c->mc_codes = (unsigned short*)got[3];
  c->mc_surv = (unsigned char*)got[4]; c->mc_d1_list = (unsigned*)got[5]; c->mc_block_bits = (unsigned*)got[6]; c->mc_recs = (uint2*)got[7];
  c->mc_recs_cap = (uint32_t)recs;
  c->region_noop = 1;                                      // no region call on this scratch yet: kf_region_work reports zeros, not what hipMalloc left in the head
  c->mc_zero_serial = c->vol_flags_serial - 1;
  return 0;
}

extern "C" int kf_marching_cubes(kf_ctx* c, int has_color, float thr) {
  if (!c) return KF_ERR_ARG;
  if (!c->triangles || c->max_triangles == 0) return KF_ERR_STATE;
  if (has_color && !c->vol.color) return KF_ERR_STATE;
  McArgs a;
  a.vol = c->vol; a.z0 = c->vol.own_z0; a.z1 = c->vol.own_z1; a.has_color = has_color; a.thr = thr;
  a.xa = 0; a.wx = c->vol.res; a.y0 = 0; a.wy = c->vol.res; a.x0 = 0; a.x1 = c->vol.res;
  a.world = 0; a.woff = make_float3(0.f, 0.f, 0.f); a.spread = 0;
  const size_t n_cells = (size_t)(a.z1 - a.z0) * c->vol.res * c->vol.res;
  a.n_blocks = (unsigned)((n_cells + 255) / 256);
  if (a.n_blocks > c->mc_blocks_cap) return KF_ERR_STATE;
  { const int st = kf_mc_scratch(c); if (st) return st; }
  mc_scratch_args(c, a);
  a.tris = c->triangles; a.max_tris = c->max_triangles; a.n_held = &c->counters->n_triangles;
  kf_evt_begin(c, KF_STAGE_MCUBES);
  if (c->mc_zero_serial != c->vol_flags_serial) {          // bricks outside the has-negative neighbourhood set must read as class 0 / no survivor
    KF_CHECK(hipMemsetAsync(c->mc_codes, 0, c->n_stored_bricks * 64 * sizeof(unsigned short), c->stream));
    KF_CHECK(hipMemsetAsync(c->mc_surv, 0, c->n_stored_bricks * 64, c->stream));
    c->mc_zero_serial = c->vol_flags_serial;
  }
  KF_CHECK(hipMemsetAsync(c->mc_block_counts, 0, ((size_t)a.n_blocks + 1) * sizeof(unsigned), c->stream));
  KF_CHECK(hipMemsetAsync(c->mc_list, 0, 4 * sizeof(unsigned), c->stream));
  KF_CHECK(hipMemsetAsync(c->mc_block_bits, 0, ((size_t)a.n_blocks / 32 + 1) * sizeof(unsigned), c->stream));
  const unsigned n_slots = (unsigned)c->n_stored_bricks;
  if (c->vol.nb % 32 == 0)
    hipLaunchKernelGGL(k_mc_dilate_words, dim3((n_slots / 32 + 255) / 256), dim3(256), 0, c->stream, c->vol, c->mc_nbr_bits, n_slots / 32, a.d1_list, a.n_d1, c->count_work ? c->counters : nullptr);
  else
    hipLaunchKernelGGL(k_mc_dilate, dim3((n_slots + 255) / 256), dim3(256), 0, c->stream, c->vol, c->mc_nbr_bits, n_slots, a.d1_list, a.n_d1, c->count_work ? c->counters : nullptr);
  const unsigned walk = (unsigned)c->num_cus * 8u;
  hipLaunchKernelGGL(k_mc_codes, dim3(walk), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL(k_mc_sift, dim3(walk), dim3(256), 0, c->stream, a);
  mc_count_and_emit(c, a, &c->counters->n_triangles, nullptr, nullptr);
  kf_evt_end(c, KF_STAGE_MCUBES);
  return (int)hipGetLastError();
}

// ---- region extraction and the world soup ---------------------------------------------------------------------------------------------
// (kf_internal.h) the region extraction behind kf_marching_cubes_region and kf_shift_volume's stream-out: the arguments are checked by the callers
int kf_mc_region_enqueue(kf_ctx* c, int has_color, float thr, const int32_t lo_in[3], const int32_t hi_in[3], int flags) {
  const KfVolume& v = c->vol;
  const int R = v.res;
  int lo[3], hi[3];
  for (int k = 0; k < 3; ++k) {
    lo[k] = lo_in[k] < 0 ? 0 : (lo_in[k] > R ? R : lo_in[k]);
    hi[k] = hi_in[k] < 0 ? 0 : (hi_in[k] > R ? R : hi_in[k]);
    if (lo[k] >= hi[k]) { c->region_noop = 1; return 0; }    // empty or inverted: nothing to do
  }
  const bool to_soup = (flags & KF_MC_TO_WORLD_SOUP) != 0;
  McArgs a;
  a.vol = v; a.has_color = has_color; a.thr = thr;
  a.x0 = lo[0]; a.x1 = hi[0]; a.xa = lo[0] & ~7; a.wx = ((hi[0] + 7) & ~7) - a.xa;
  a.y0 = lo[1]; a.wy = hi[1] - lo[1]; a.z0 = lo[2]; a.z1 = hi[2];
  a.world = (flags & KF_MC_WORLD) ? 1 : 0; a.spread = 1;
  a.woff = make_float3((float)c->origin_vox[0] * v.cell, (float)c->origin_vox[1] * v.cell, (float)c->origin_vox[2] * v.cell);
  const size_t n_cells = (size_t)(a.z1 - a.z0) * (size_t)a.wy * (size_t)a.wx;
  a.n_blocks = (unsigned)((n_cells + 255) / 256);
  if (a.n_blocks > c->mc_blocks_cap) return KF_ERR_STATE;
  { const int st = kf_mc_scratch(c); if (st) return st; }
  mc_scratch_args(c, a);
  unsigned* n_tris; unsigned long long* dropped = nullptr;
  if (to_soup) { a.tris = c->soup; a.max_tris = c->soup_cap; n_tris = c->soup_cnt; dropped = reinterpret_cast<unsigned long long*>(c->soup_cnt + 2); }
  else { a.tris = c->triangles; a.max_tris = c->max_triangles; n_tris = &c->counters->n_triangles; }
  a.n_held = n_tris;
  McRegionBricks g;
  unsigned n_w = 1;
  for (int k = 0; k < 3; ++k) {
    g.blo[k] = lo[k] >> 3; g.bhi[k] = ((hi[k] - 1) >> 3) + 1;
    g.wlo[k] = g.blo[k] > 0 ? g.blo[k] - 1 : 0;
    const int whi = g.bhi[k] < v.nb ? g.bhi[k] + 1 : v.nb;
    g.wn[k] = whi - g.wlo[k];
    n_w *= (unsigned)g.wn[k];
  }
  unsigned* sift_list = c->mc_d1_list + c->n_stored_bricks;
  kf_evt_begin(c, KF_STAGE_MCUBES);
  hipLaunchKernelGGL(k_mc_region_clear, dim3((a.n_blocks + 1 + 255) / 256), dim3(256), 0, c->stream, c->mc_block_counts, a.n_blocks + 1, c->mc_block_bits,
                     a.n_blocks / 32 + 1, c->mc_list);
  hipLaunchKernelGGL(k_mc_region_bricks, dim3((n_w + 255) / 256), dim3(256), 0, c->stream, a, g, sift_list, c->mc_list + 4);
  // the persistent walkers, no more of them than the widened range has bricks (four per workgroup)
  const unsigned walk_all = (unsigned)c->num_cus * 8u, walk = (n_w + 3) / 4 < walk_all ? (n_w + 3) / 4 : walk_all;
  hipLaunchKernelGGL(k_mc_codes, dim3(walk), dim3(256), 0, c->stream, a);
  McArgs s = a; s.d1_list = sift_list; s.n_d1 = c->mc_list + 4;
  hipLaunchKernelGGL(k_mc_sift, dim3(walk), dim3(256), 0, c->stream, s);
  mc_count_and_emit(c, a, n_tris, dropped, c->mc_list + 5);
  kf_evt_end(c, KF_STAGE_MCUBES);
  c->region_noop = 0;
  return (int)hipGetLastError();
}

extern "C" int kf_marching_cubes_region(kf_ctx* c, int has_color, float thr, const int32_t lo[3], const int32_t hi[3], int flags) {
  if (!c || !lo || !hi) return KF_ERR_ARG;
  if (flags & ~(KF_MC_WORLD | KF_MC_TO_WORLD_SOUP)) return KF_ERR_ARG;
  if ((flags & KF_MC_TO_WORLD_SOUP) && !(flags & KF_MC_WORLD)) return KF_ERR_ARG;       // the world soup holds world coordinates only
  if (!kf_whole_volume(c)) return KF_ERR_ARG;                     // a z-slab context, as for kf_shift_volume
  if (has_color && !c->vol.color) return KF_ERR_STATE;
  if (flags & KF_MC_TO_WORLD_SOUP) { if (!c->soup) return KF_ERR_STATE; }
  else if (!c->triangles || c->max_triangles == 0) return KF_ERR_STATE;
  return kf_mc_region_enqueue(c, has_color, thr, lo, hi, flags);
}

extern "C" int kf_region_work(kf_ctx* c, uint64_t out[2]) {
  if (!c || !out) return KF_ERR_ARG;
  out[0] = out[1] = 0;
  if (!c->mc_list || c->region_noop) return 0;
  KF_CHECK(hipMemcpyAsync(c->host_pinned, c->mc_list + 5, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
  KF_CHECK(hipStreamSynchronize(c->stream));
  out[0] = ((unsigned*)c->host_pinned)[0]; out[1] = ((unsigned*)c->host_pinned)[1];
  return 0;
}

void kf_world_soup_free(kf_ctx* c) {
  if (c->soup) hipFree(c->soup);
  if (c->soup_cnt) hipFree(c->soup_cnt);
  c->soup = nullptr; c->soup_cnt = nullptr; c->soup_cap = 0; c->stream_on = 0;
}
extern "C" int kf_world_soup_reserve(kf_ctx* c, uint32_t max_triangles) {
  if (!c) return KF_ERR_ARG;
  KF_CHECK(hipSetDevice(c->cfg.device));
  KF_CHECK(hipStreamSynchronize(c->stream));                 // whatever still writes the old soup
  kf_world_soup_free(c);
  if (max_triangles == 0) return 0;
  kf_triangle* soup = nullptr; unsigned* cnt = nullptr; uint2* recs = nullptr;
  const bool grow_recs = c->mc_list && max_triangles > c->mc_recs_cap;      // the record list holds a cell per triangle of the larger destination
  hipError_t e = hipMalloc((void**)&soup, (size_t)max_triangles * sizeof(kf_triangle));
  if (e == hipSuccess) e = hipMalloc((void**)&cnt, 4 * sizeof(unsigned));
  if (e == hipSuccess && grow_recs) e = hipMalloc((void**)&recs, (size_t)max_triangles * sizeof(uint2));
  if (e != hipSuccess) { if (soup) hipFree(soup); if (cnt) hipFree(cnt); (void)hipGetLastError(); return (int)e; }
  if (grow_recs) { hipFree(c->mc_recs); c->mc_recs = recs; c->mc_recs_cap = max_triangles; }
  c->soup = soup; c->soup_cnt = cnt; c->soup_cap = max_triangles;
  KF_CHECK(hipMemsetAsync(c->soup_cnt, 0, 4 * sizeof(unsigned), c->stream));
  return 0;
}
extern "C" int kf_clear_world_soup(kf_ctx* c) {
  if (!c) return KF_ERR_ARG;
  if (!c->soup) return KF_ERR_STATE;
  KF_CHECK(hipMemsetAsync(c->soup_cnt, 0, 4 * sizeof(unsigned), c->stream));
  return 0;
}
extern "C" int kf_world_soup_count(kf_ctx* c, uint32_t* count, uint32_t* dropped) {
  if (!c || !count) return KF_ERR_ARG;
  *count = 0; if (dropped) *dropped = 0;
  if (!c->soup) return 0;
  KF_CHECK(hipMemcpyAsync(c->host_pinned, c->soup_cnt, 4 * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
  KF_CHECK(hipStreamSynchronize(c->stream));
  const unsigned* h = (const unsigned*)c->host_pinned;
  *count = h[0];
  if (dropped) { const unsigned long long d = (unsigned long long)h[2] | ((unsigned long long)h[3] << 32); *dropped = d > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)d; }
  return 0;
}
extern "C" int kf_read_world_soup(kf_ctx* c, kf_triangle* dst, uint32_t first, uint32_t count) {
  if (!c || !dst) return KF_ERR_ARG;
  if ((uint64_t)first + count > c->soup_cap) return KF_ERR_ARG;
  if (count == 0) return 0;
  KF_CHECK(hipMemcpyAsync(dst, c->soup + first, (size_t)count * sizeof(kf_triangle), hipMemcpyDeviceToHost, c->stream));
  KF_CHECK(hipStreamSynchronize(c->stream));
  return 0;
}
// the world soup behind what the triangle buffer holds, clamped at the buffer's capacity: 18 words per triangle, a lane per word
__global__ void __launch_bounds__(256) k_soup_append(const kf_triangle* __restrict__ soup, const unsigned* __restrict__ n_soup, kf_triangle* __restrict__ tris,
                                                    const unsigned* __restrict__ n_tris, unsigned max_tris) {
  const unsigned held = *n_tris, room = max_tris - held, n = *n_soup < room ? *n_soup : room;
  const size_t words = (size_t)n * 18u;
  const unsigned* src = reinterpret_cast<const unsigned*>(soup);
  unsigned* dst = reinterpret_cast<unsigned*>(tris + held);
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < words; i += (size_t)gridDim.x * 256u) dst[i] = src[i];
}
__global__ void k_soup_append_finish(const unsigned* n_soup, unsigned* n_tris, unsigned max_tris) {
  if (threadIdx.x == 0 && blockIdx.x == 0) { const unsigned long long t = (unsigned long long)*n_tris + *n_soup; *n_tris = (unsigned)(t > max_tris ? max_tris : t); }
}
extern "C" int kf_append_world_soup(kf_ctx* c) {
  if (!c) return KF_ERR_ARG;
  if (!c->soup || !c->triangles || c->max_triangles == 0) return KF_ERR_STATE;
  hipLaunchKernelGGL(k_soup_append, dim3((unsigned)c->num_cus * 8u), dim3(256), 0, c->stream, (const kf_triangle*)c->soup, (const unsigned*)c->soup_cnt, c->triangles,
                     (const unsigned*)&c->counters->n_triangles, c->max_triangles);
  hipLaunchKernelGGL(k_soup_append_finish, dim3(1), dim3(64), 0, c->stream, (const unsigned*)c->soup_cnt, &c->counters->n_triangles, c->max_triangles);
  return (int)hipGetLastError();
}
extern "C" int kf_set_stream_out(kf_ctx* c, int on, int has_color, float thr) {
  if (!c) return KF_ERR_ARG;
  if (!on) { c->stream_on = 0; return 0; }
  if (!c->soup) return KF_ERR_STATE;
  if (has_color && !c->vol.color) return KF_ERR_STATE;
  if (!kf_whole_volume(c)) return KF_ERR_ARG;
  c->stream_on = 1; c->stream_color = has_color ? 1 : 0; c->stream_thr = thr;
  return 0;
}

extern "C" int kf_clear_triangles(kf_ctx* c) {
  if (!c) return KF_ERR_ARG;
  KF_CHECK(hipMemsetAsync(&c->counters->n_triangles, 0, sizeof(unsigned), c->stream));
  return 0;
}

extern "C" int kf_triangle_count(kf_ctx* c, uint32_t* count) {
  if (!c || !count) return KF_ERR_ARG;
  KF_CHECK(hipMemcpyAsync(c->host_pinned, &c->counters->n_triangles, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
  KF_CHECK(hipStreamSynchronize(c->stream));
  *count = *(unsigned*)c->host_pinned;
  return 0;
}

extern "C" int kf_read_triangles(kf_ctx* c, kf_triangle* dst, uint32_t first, uint32_t count) {
  if (!c || !dst) return KF_ERR_ARG;
  if ((uint64_t)first + count > c->max_triangles) return KF_ERR_ARG;
  if (count == 0) return 0;
  KF_CHECK(hipMemcpyAsync(dst, c->triangles + first, (size_t)count * sizeof(kf_triangle), hipMemcpyDeviceToHost, c->stream));
  KF_CHECK(hipStreamSynchronize(c->stream));
  return 0;
}
