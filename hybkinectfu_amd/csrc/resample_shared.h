// resample_shared.h -- what the two kernels that read an incoming map through a hash table of its own share: resample.hip (kf_merge_brick_store_rigid) and
// align.hip (kf_align_brick_store).  No reference counterpart.
#pragma once
#include "kf_internal.h"

// the source map on the device: the three planes in kf_read_brick_store's layout, and its table as a KfBrickStore of which store_find reads tkey, tslot, mask
// and max_bricks (= the number of entries) only
struct KfResampleSource { const float* tsdf; const float* weight; const unsigned char* color; };

__device__ __forceinline__ float lerp1(float a, float b, float f) { return a + f * (b - a); }

// min(0, 7 r): the least a column entry adds to u over the brick's l in [0, 8)
__device__ __forceinline__ float least7(float r) { return fminf(0.f, 7.f * r); }

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
