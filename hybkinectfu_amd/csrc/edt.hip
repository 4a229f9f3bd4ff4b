// edt.hip -- the distance field of the map: for every voxel of a box the exact squared Euclidean distance, in voxels, to the nearest SITE of the map -- a voxel
// whose class (unknown / free / occupied) is in the caller's mask -- up to a radius R, and the class bytes (kf_map_distance_field).  The map is the window's
// bricks and, outside the window, the brick store's (map_lookup.h), read where it lies.  No reference counterpart.  The contract is written out above
// kf_map_distance_field in include/hybkf.h, the argument in DESIGN.md 4e-9.
// Four kinds of launch, chained by stream order, integers only, no atomics:
//   classify  one workgroup per brick of the box widened by R: the brick resolved, each voxel classed with its TRUE weight, one site BIT per voxel written into
//             a bit volume (a brick row of 8 voxels is one byte of a ballot), the class byte written for the voxels of the box proper;
//   x pass    per voxel of nx x (ny + 2R) x (nz + 2R) the distance to the nearest set bit of its row within +-R, by count-trailing / count-leading-zeros on
//             the row's 64-bit words; stored SQUARED as 16 bits (255^2 fits below KF_EDT_FAR), so that the two passes after it are one kernel;
//   y pass, z pass   out(v) = min over j in [-R, R] of in(v + j) + j^2, FAR above R^2: j walks outwards from 0 and stops once j^2 is not below the best so
//             far (no later tap can win: every term is >= j^2).  Lanes run along x, so every tap is a coalesced row.
// The windowed passes are exact: where d2 <= R^2 every component of the offset to the nearest site is <= R and every partial sum <= R^2, so no window and no
// FAR cut drops it; where d2 > R^2 no path gives a value <= R^2.
#include "kf_internal.h"
#include "brick_key.h"
#include "brick_find.h"
#include "map_lookup.h"
#include <stdint.h>
#include <math.h>

using namespace mapq;

#define KF_EDT_MAX_RADIUS 255u
#define KF_EDT_MAX_DOMAIN (1ull << 29)   // nx * (ny + 2R) * (nz + 2R): the x pass's output, 2 bytes each -- 1 GiB of scratch at the most for it (the bit volume, widened
                                         // in x too, is not bounded by this: hipMalloc's refusal, KF_ERR_ALLOC, is its only guard -- include/hybkf.h)

// the box, and the brick-aligned region around it that the classify pass covers: the box widened by `halo` (R; 0 when only the classes are asked for)
struct EdtBox {
  int lo[3];             // the box's first voxel, world voxels
  unsigned n[3];         // its dimensions
  int b0[3];             // the region's first brick, world bricks: (lo - halo) >> 3
  unsigned nbk[3];       // the region's bricks per axis
  unsigned halo;
  unsigned row_words;    // 64-bit words of one x row of the bit volume: ceil(nbk[0] / 8); the rows are (8 nbk[2]) x (8 nbk[1])
};

// One workgroup per brick, two voxels per lane (z and z + 4): wave w holds the z slices w and w + 4, lane l of it the voxel (x = l & 7, y = l >> 3), so one
// ballot is the slice's 8 rows of 8 site bits.  A brick nobody holds costs no load; where unknown is no site it costs no store either (the bits were zeroed).
__global__ void __launch_bounds__(256) k_edt_classify(MapRef m, EdtBox e, float level, unsigned site_mask, unsigned char* __restrict__ bits,
                                                      unsigned char* __restrict__ cls) {
  const unsigned nbricks = e.nbk[0] * e.nbk[1] * e.nbk[2];
  const size_t row_bytes = (size_t)e.row_words * 8u, rows_y = (size_t)e.nbk[1] * 8u;
  for (unsigned i = blockIdx.x; i < nbricks; i += gridDim.x) {
    const unsigned kx = i % e.nbk[0], r = i / e.nbk[0], ky = r % e.nbk[1], kz = r / e.nbk[1];
    const int bx = e.b0[0] + (int)kx, by = e.b0[1] + (int)ky, bz = e.b0[2] + (int)kz;
    MapBrick b = map_brick_none();
    if (kf_brick_key_in_range(bx) && kf_brick_key_in_range(by) && kf_brick_key_in_range(bz)) map_brick_resolve(m, bx, by, bz, kf_brick_key_pack(bx, by, bz), b);
    if (!b.tw && !(site_mask & (1u << KF_VOX_UNKNOWN)) && !cls) continue;            // (the same in every lane of the workgroup)
#pragma unroll
    for (unsigned h = 0; h < 2; ++h) {
      const unsigned off = threadIdx.x + 256u * h;
      const unsigned vx = off & 7u, vy = (off >> 3) & 7u, vz = off >> 6;
      unsigned c = KF_VOX_UNKNOWN;
      if (b.tw) {
        const float2 q = b.tw[off];
        // the TRUE weight, as the definition says.  (Today a word is only set on a quarter whose stored weights are all >= 1 -- integrate.hip, DEFER -- so the
        // word cannot turn an unobserved voxel into an observed one; the class follows the definition, not that invariant.)
        const unsigned pq = (unsigned)(b.pend >> (16u * (off >> 7))) & 0xFFFFu;
        if (kf_pend_weight(q.y, pq, m.vol.max_weight) > 0.f) c = q.x > level ? KF_VOX_FREE : KF_VOX_OCCUPIED;
      }
      if (bits) {
        const unsigned long long rows = __ballot((site_mask >> c) & 1u);
        if (vx == 0u && (b.tw || (site_mask & (1u << KF_VOX_UNKNOWN))))
          bits[((size_t)(8u * kz + vz) * rows_y + (8u * ky + vy)) * row_bytes + kx] = (unsigned char)(rows >> (threadIdx.x & 56u));
      }
      if (cls) {
        const unsigned ux = (unsigned)(8 * bx + (int)vx - e.lo[0]), uy = (unsigned)(8 * by + (int)vy - e.lo[1]), uz = (unsigned)(8 * bz + (int)vz - e.lo[2]);
        if (ux < e.n[0] && uy < e.n[1] && uz < e.n[2]) cls[((size_t)uz * e.n[1] + uy) * e.n[0] + ux] = (unsigned char)c;
      }
    }
  }
}

// the distance from bit b of word wi to the nearest set bit at or above it (edt_right) / at or below it (edt_left), R + 1 when there is none within R.  The row
// reaches R voxels beyond the box on both sides, so a word index outside [0, nw) is never within R.
__device__ __forceinline__ unsigned edt_right(const unsigned long long* __restrict__ w, unsigned wi, unsigned b, unsigned nw, unsigned R) {
  unsigned long long mk = w[wi] >> b;
  if (mk) return (unsigned)__builtin_ctzll(mk);
  unsigned d = 64u - b;
  for (unsigned k = wi + 1u; d <= R && k < nw; ++k, d += 64u) {
    mk = w[k];
    if (mk) return d + (unsigned)__builtin_ctzll(mk);
  }
  return R + 1u;
}
__device__ __forceinline__ unsigned edt_left(const unsigned long long* __restrict__ w, unsigned wi, unsigned b, unsigned R) {
  unsigned long long mk = w[wi] << (63u - b);
  if (mk) return (unsigned)__builtin_clzll(mk);
  unsigned d = b + 1u;
  for (unsigned k = wi; d <= R && k > 0u; d += 64u) {
    mk = w[--k];
    if (mk) return d + (unsigned)__builtin_clzll(mk);
  }
  return R + 1u;
}

// x pass: item idx = (zz * (ny + 2R) + yy) * nx + x of the domain; out = dx^2 where the nearest site of the row is dx <= R away, else FAR
__global__ void __launch_bounds__(256) k_edt_x(EdtBox e, const unsigned long long* __restrict__ bits, unsigned short* __restrict__ out, unsigned n) {
  const unsigned R = e.halo, nx = e.n[0], Y = e.n[1] + 2u * R;
  const unsigned px0 = (unsigned)(e.lo[0] - 8 * e.b0[0]);                 // the box's x = 0 in the row's bits (>= R: b0 is the brick of lo - R)
  const unsigned py0 = (unsigned)(e.lo[1] - (int)R - 8 * e.b0[1]), pz0 = (unsigned)(e.lo[2] - (int)R - 8 * e.b0[2]);
  const size_t rows_y = (size_t)e.nbk[1] * 8u;
  for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx < n; idx += gridDim.x * 256u) {
    const unsigned x = idx % nx, row = idx / nx, yy = row % Y, zz = row / Y;
    const unsigned long long* w = bits + ((size_t)(zz + pz0) * rows_y + (yy + py0)) * e.row_words;
    const unsigned p = px0 + x, wi = p >> 6, b = p & 63u;
    const unsigned dr = edt_right(w, wi, b, e.row_words, R), dl = edt_left(w, wi, b, R);
    const unsigned d = dr < dl ? dr : dl;
    out[idx] = (unsigned short)(d <= R ? d * d : KF_EDT_FAR);
  }
}

// y pass and z pass: out[idx] = min over j in [-R, R] of in[c + j * stride] + j^2, FAR above R^2, with c = idx + ((idx / plane) * 2R + R) * stride.
//   y pass: in [nz + 2R][ny + 2R][nx], out [nz + 2R][ny][nx], plane = ny * nx, stride = nx;   z pass: in [nz + 2R][ny][nx], out [nz][ny][nx], plane = n, stride = ny * nx
__global__ void __launch_bounds__(256) k_edt_pass(const unsigned short* __restrict__ in, unsigned short* __restrict__ out, unsigned n, unsigned plane, unsigned stride,
                                                  unsigned R) {
  const unsigned R2 = R * R;
  for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx < n; idx += gridDim.x * 256u) {
    const unsigned c = idx + ((idx / plane) * 2u * R + R) * stride;
    unsigned best = in[c];
    unsigned up = c, dn = c;
    for (unsigned j = 1; j <= R; ++j) {
      const unsigned j2 = j * j;
      if (j2 >= best) break;                                              // every later term is >= j^2
      up += stride; dn -= stride;
      const unsigned a = in[up], b = in[dn];
      const unsigned t = (a < b ? a : b) + j2;
      best = t < best ? t : best;
    }
    out[idx] = (unsigned short)(best > R2 ? KF_EDT_FAR : best);
  }
}

static inline size_t edt_pad(size_t b) { return (b + 255u) & ~(size_t)255u; }
static inline unsigned edt_grid(size_t n) { const size_t g = (n + 255u) / 256u; return (unsigned)(g > 8192u ? 8192u : g); }

// KF_ERR_ARG or 0; n_dom: the x pass's item count
static int edt_args(const kf_ctx* c, const int32_t* lo, const uint32_t* dims, uint32_t radius, float level, uint32_t site_mask, uint64_t& n_dom) {
  if (!c || !lo || !dims) return KF_ERR_ARG;
  if (radius < 1u || radius > KF_EDT_MAX_RADIUS || site_mask < 1u || site_mask > 7u || level != level) return KF_ERR_ARG;
  const int64_t vmin = (int64_t)KF_BRICK_KEY_MIN * 8, vmax = (int64_t)KF_BRICK_KEY_MAX * 8;
  for (int k = 0; k < 3; ++k)
    if (dims[k] == 0u || (int64_t)lo[k] < vmin || (int64_t)lo[k] + (int64_t)dims[k] > vmax) return KF_ERR_ARG;
  const uint64_t a = (uint64_t)dims[0] * ((uint64_t)dims[1] + 2u * radius);
  if (a > KF_EDT_MAX_DOMAIN) return KF_ERR_ARG;
  n_dom = a * ((uint64_t)dims[2] + 2u * radius);
  return n_dom > KF_EDT_MAX_DOMAIN ? KF_ERR_ARG : 0;
}

// the context's scratch made at least `bytes` long.  Growing it frees the old one, which work already on the stream may still read: that work is waited for.
static int edt_scratch(kf_ctx* c, size_t bytes) {
  if (c->edt_scratch_bytes >= bytes) return 0;
  if (c->edt_scratch) {
    KF_CHECK(hipStreamSynchronize(c->stream));
    hipFree(c->edt_scratch);
    c->edt_scratch = nullptr; c->edt_scratch_bytes = 0;
  }
  if (hipMalloc(&c->edt_scratch, bytes) != hipSuccess) { c->edt_scratch = nullptr; (void)hipGetLastError(); return KF_ERR_ALLOC; }
  c->edt_scratch_bytes = bytes;
  return 0;
}
void kf_edt_scratch_free(kf_ctx* c) {
  if (c->edt_scratch) { hipFree(c->edt_scratch); c->edt_scratch = nullptr; }
  c->edt_scratch_bytes = 0;
}

extern "C" int kf_map_distance_field_device(kf_ctx* c, const int32_t lo_vox[3], const uint32_t dims[3], uint32_t radius, float level, uint32_t site_mask,
                                            uint16_t* dev_dist2, uint8_t* dev_cls) {
  uint64_t n_dom = 0;
  { const int as = edt_args(c, lo_vox, dims, radius, level, site_mask, n_dom); if (as) return as; }
  if (!kf_whole_volume(c)) return KF_ERR_STATE;
  if (!dev_dist2 && !dev_cls) return 0;
  KF_CHECK(hipSetDevice(c->cfg.device));
  const MapRef m = query_map(c);
  EdtBox e;
  e.halo = dev_dist2 ? radius : 0u;
  size_t nbricks = 1;
  for (int k = 0; k < 3; ++k) {
    e.lo[k] = lo_vox[k]; e.n[k] = dims[k];
    e.b0[k] = (lo_vox[k] - (int)e.halo) >> 3;
    e.nbk[k] = (unsigned)(((lo_vox[k] + (int)dims[k] - 1 + (int)e.halo) >> 3) - e.b0[k] + 1);
    nbricks *= e.nbk[k];
  }
  e.row_words = (e.nbk[0] + 7u) / 8u;
  const unsigned cgrid = (unsigned)(nbricks > 32768u ? 32768u : nbricks);
  if (!dev_dist2) {                                                      // the classes alone: the box's own bricks, no bits
    hipLaunchKernelGGL(k_edt_classify, dim3(cgrid), dim3(256), 0, c->stream, m, e, level, site_mask, (unsigned char*)nullptr, dev_cls);
    return (int)hipGetLastError();
  }
  const size_t R = radius, nx = dims[0], ny = dims[1], nz = dims[2];
  const size_t n_x = (size_t)n_dom, n_y = nx * ny * (nz + 2 * R), n_z = nx * ny * nz;
  const size_t b_bits = edt_pad((size_t)e.nbk[2] * 8u * e.nbk[1] * 8u * e.row_words * 8u), b_x = edt_pad(2 * n_x), b_y = edt_pad(2 * n_y);
  { const int ss = edt_scratch(c, b_bits + b_x + b_y); if (ss) return ss; }
  unsigned char* bits = (unsigned char*)c->edt_scratch;
  unsigned short* dx2 = (unsigned short*)(bits + b_bits);
  unsigned short* dy2 = (unsigned short*)(bits + b_bits + b_x);
  KF_CHECK(hipMemsetAsync(bits, 0, b_bits, c->stream));
  hipLaunchKernelGGL(k_edt_classify, dim3(cgrid), dim3(256), 0, c->stream, m, e, level, site_mask, bits, dev_cls);
  hipLaunchKernelGGL(k_edt_x, dim3(edt_grid(n_x)), dim3(256), 0, c->stream, e, (const unsigned long long*)bits, dx2, (unsigned)n_x);
  hipLaunchKernelGGL(k_edt_pass, dim3(edt_grid(n_y)), dim3(256), 0, c->stream, (const unsigned short*)dx2, dy2, (unsigned)n_y, (unsigned)(nx * ny), (unsigned)nx, radius);
  hipLaunchKernelGGL(k_edt_pass, dim3(edt_grid(n_z)), dim3(256), 0, c->stream, (const unsigned short*)dy2, dev_dist2, (unsigned)n_z, (unsigned)n_z, (unsigned)(nx * ny), radius);
  return (int)hipGetLastError();
}

// the host form: the two outputs in one temporary (KfCarveTemp), one wait
extern "C" int kf_map_distance_field(kf_ctx* c, const int32_t lo_vox[3], const uint32_t dims[3], uint32_t radius, float level, uint32_t site_mask, uint16_t* dist2,
                                     uint8_t* cls) {
  uint64_t n_dom = 0;
  { const int as = edt_args(c, lo_vox, dims, radius, level, site_mask, n_dom); if (as) return as; }
  if (!kf_whole_volume(c)) return KF_ERR_STATE;
  if (!dist2 && !cls) return 0;
  KF_CHECK(hipSetDevice(c->cfg.device));
  const size_t n = (size_t)dims[0] * dims[1] * dims[2];
  KfCarveTemp tmp;
  if (!tmp.get(KfCarveTemp::pad(2 * n) + KfCarveTemp::pad(n))) return KF_ERR_ALLOC;
  uint16_t* d_d = tmp.down(dist2, 2 * n);
  uint8_t* d_c = tmp.down(cls, n);
  return tmp.finish(c, kf_map_distance_field_device(c, lo_vox, dims, radius, level, site_mask, d_d, d_c));
}
