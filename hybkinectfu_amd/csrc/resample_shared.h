// resample_shared.h -- what the code that reads an incoming map through a hash table of its own shares: how the map reaches the device (kf_source_map_upload:
// resample.hip, halve.hip, align.hip), and for the two kernels that read it trilinearly -- k_store_resample_merge and k_store_align_sums -- the 27 source
// bricks around a destination brick (source_bricks27) and one corner's fetch (source_corner).  query.hip takes lerp1.  No reference counterpart.
#pragma once
#include "kf_internal.h"
#include "brick_key.h"
#include "brick_find.h"
#include <vector>

// the source map on the device: the three planes in kf_read_brick_store's layout, and its table as a KfBrickStore of which store_find reads tkey, tslot, mask
// and max_bricks (= the number of entries) only
struct KfResampleSource { const float* tsdf; const float* weight; const unsigned char* color; };

__device__ __forceinline__ float lerp1(float a, float b, float f) { return a + f * (b - a); }

// min(0, 7 r): the least a column entry adds to u over the brick's l in [0, 8)
__device__ __forceinline__ float least7(float r) { return fminf(0.f, 7.f * r); }

// The source bricks one destination brick can draw on.  (ib, fb): the source position of its voxel (0, 0, 0) as an integer and a fraction (rigid_keys.h),
// r<i><j> = (float)R[i][j].  u_j = sum_i r_ij l_i + fb_j spans at most 7 (|r_0j| + |r_1j| + |r_2j|) <= 7 sqrt(3) (1 + 1e-5) < 12.13 (a column of R has a norm
// within 1e-5 of 1).  lo_j = sum_i min(0, 7 r_ij) + fb_j - 0.01 lies below every u_j the lanes compute (their roundings are far below 0.01), so with
// n0 = floor(lo_j) every corner floor(u_j) + {0, 1} lies in [n0, n0 + 14]: 15 integers, at most three source bricks per axis from brick b0 = (ib + n0) >> 3 on.
// The first 27 lanes look the slots of b0 + [0, 3)^3 up into s_src (none when !fit: the brick has no base corner); returns whether this lane found one.  The
// caller joins the lanes' answers and orders the write to s_src before the reads, by a barrier of its own kind.
__device__ __forceinline__ bool source_bricks27(const KfBrickStore& stab, bool fit, int ibx, int iby, int ibz, float fbx, float fby, float fbz, float r00, float r01,
                                                float r02, float r10, float r11, float r12, float r20, float r21, float r22, int& b0x, int& b0y, int& b0z,
                                                unsigned* s_src) {
  b0x = (ibx + (int)floorf(((least7(r00) + least7(r10)) + least7(r20)) + fbx - 0.01f)) >> 3;
  b0y = (iby + (int)floorf(((least7(r01) + least7(r11)) + least7(r21)) + fby - 0.01f)) >> 3;
  b0z = (ibz + (int)floorf(((least7(r02) + least7(r12)) + least7(r22)) + fbz - 0.01f)) >> 3;
  bool any = false;
  if (threadIdx.x < 27u) {
    const int bx = b0x + (int)(threadIdx.x % 3u), by = b0y + (int)((threadIdx.x / 3u) % 3u), bz = b0z + (int)(threadIdx.x / 9u);
    unsigned slot = KF_BRICK_NO_SLOT;                                         // (a brick outside the key range has no key: packed, it would alias another)
    if (fit && kf_brick_key_in_range(bx) && kf_brick_key_in_range(by) && kf_brick_key_in_range(bz)) slot = store_find(stab, kf_brick_key_pack(bx, by, bz));
    s_src[threadIdx.x] = slot;
    any = slot != KF_BRICK_NO_SLOT;
  }
  return any;
}

// a source position along one axis, u relative to the base corner ib: the voxel floor(u) (returned) and the fraction f in [0, 1)
__device__ __forceinline__ int source_split(float u, int ib, float& f) {
  const float n = floorf(u);
  f = u - n;
  return ib + (int)n;
}

// One corner of a trilinear read: source voxel (x, y, z).  held: the source has its brick (and the corner was wanted); then o is the voxel's index into the
// planes and (t, w) its tsdf and weight, else (0, 0).  s_src: source_bricks27's slots; a corner outside b0 + [0, 3)^3 reads as not held (the bound above shows
// that none lies outside; the test keeps a rounding surprise from indexing past the table).
struct KfSourceCorner { bool held; size_t o; float t, w; };
__device__ __forceinline__ KfSourceCorner source_corner(const KfResampleSource& src, const unsigned* s_src, int x, int y, int z, int b0x, int b0y, int b0z,
                                                        bool wanted) {
  const unsigned tx = (unsigned)((x >> 3) - b0x), ty = (unsigned)((y >> 3) - b0y), tz = (unsigned)((z >> 3) - b0z);
  const unsigned slot = (wanted && tx < 3u && ty < 3u && tz < 3u) ? s_src[(tz * 3u + ty) * 3u + tx] : KF_BRICK_NO_SLOT;
  KfSourceCorner c = {slot != KF_BRICK_NO_SLOT, 0, 0.f, 0.f};
  if (c.held) {
    c.o = (size_t)slot * KF_BRICK_VOX + (size_t)(((z & 7) << 6) | ((y & 7) << 3) | (x & 7));
    c.w = src.weight[c.o];
    c.t = src.tsdf[c.o];
  }
  return c;
}

// the temporary device allocations of one call, freed on every way out
struct KfResampleTemp {
  void* p[8] = {};
  int n = 0;
  bool get(void** out, size_t bytes) {
    if (hipMalloc(out, bytes ? bytes : 1) != hipSuccess) { (void)hipGetLastError(); *out = nullptr; return false; }
    p[n++] = *out;
    return true;
  }
  ~KfResampleTemp() { for (int i = 0; i < n; ++i) hipFree(p[i]); }
};

// A source map of `count` bricks goes up: its planes (colour where given) and its table (rigid_keys.h: kf_source_keys_table) into allocations of tmp, the
// copies enqueued on the context's stream in that order.  False: an allocation failed and nothing is enqueued (the caller's KF_ERR_ALLOC: nothing touched).
// Else e is the first copy's error, or hipSuccess, and stab / src are what the kernels take; the caller synchronises either way before it returns, so that
// nothing still reads the caller's arrays.
static inline bool kf_source_map_upload(kf_ctx* c, KfResampleTemp& tmp, uint32_t count, const float* tsdf, const float* weight, const uint8_t* color,
                                        const std::vector<unsigned long long>& tkey, const std::vector<unsigned>& tslot, uint32_t mask, KfBrickStore& stab,
                                        KfResampleSource& src, hipError_t& e) {
  const size_t vox = (size_t)count * KF_BRICK_VOX;
  float *dt = nullptr, *dw = nullptr;
  unsigned char* dc = nullptr;
  unsigned long long* dtkey = nullptr;
  unsigned* dtslot = nullptr;
  if (!tmp.get((void**)&dt, vox * sizeof(float)) || !tmp.get((void**)&dw, vox * sizeof(float)) || (color && !tmp.get((void**)&dc, vox * 3)) ||
      !tmp.get((void**)&dtkey, tkey.size() * sizeof(unsigned long long)) || !tmp.get((void**)&dtslot, tslot.size() * sizeof(unsigned)))
    return false;
  e = hipSuccess;
  if (count) {                                               // (an empty source: the arrays are not looked at)
    e = hipMemcpyAsync(dt, tsdf, vox * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dw, weight, vox * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && color) e = hipMemcpyAsync(dc, color, vox * 3, hipMemcpyHostToDevice, c->stream);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(dtkey, tkey.data(), tkey.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dtslot, tslot.data(), tslot.size() * sizeof(unsigned), hipMemcpyHostToDevice, c->stream);
  stab = KfBrickStore{};
  stab.tkey = dtkey; stab.tslot = dtslot; stab.max_bricks = count; stab.mask = mask;
  src = KfResampleSource{dt, dw, dc};
  return true;
}
