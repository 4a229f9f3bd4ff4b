// scan.h -- the ordered exclusive prefix sum the extraction (mcubes.hip) and the weld (weld.hip) share: a workgroup-wide scan of
// one value per lane, and the three-launch scan of an array in place.  Every translation unit that includes this gets kernels of
// its own (internal linkage).
#pragma once
#include <hip/hip_runtime.h>

#define KF_SCAN_CHUNK 4096u        // values scanned by one workgroup (16 per lane)

// workgroup-wide exclusive prefix of one value per lane (256 lanes); s_wave: 4 words; the trailing barrier frees s_wave again
__device__ __forceinline__ unsigned kf_block_excl_scan(unsigned local, unsigned* s_wave, unsigned& total) {
  unsigned inc = local;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { const unsigned t = __shfl_up(inc, off, 64); if ((threadIdx.x & 63) >= (unsigned)off) inc += t; }
  if ((threadIdx.x & 63) == 63) s_wave[threadIdx.x >> 6] = inc;
  __syncthreads();
  unsigned wave_off = 0;
  for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) wave_off += s_wave[w];
  total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
  __syncthreads();
  return wave_off + inc - local;
}

// ---- exclusive prefix sum of counts[0, n), in place, in three parallel steps ---------------------------------------------------
// (1) every workgroup sums its chunk of KF_SCAN_CHUNK counts; (2) one workgroup turns the chunk sums into their exclusive prefix (a
// few thousand values even at 2048^3); (3) every workgroup rescans its chunk on top of its offset.  total -> counts[n] (and *total_out).
// `counts` holds n + 1 words and is 16-byte aligned, `partials` ceil(n / KF_SCAN_CHUNK) words.
static __global__ void __launch_bounds__(256) k_scan_reduce(const unsigned* __restrict__ counts, unsigned n, unsigned* __restrict__ partials) {
  __shared__ unsigned s_wave[4];
  const unsigned i0 = blockIdx.x * KF_SCAN_CHUNK + threadIdx.x * 16u;
  unsigned local = 0;
  if (i0 + 16u <= n) {
    const uint4* p = reinterpret_cast<const uint4*>(counts + i0);
#pragma unroll
    for (int k = 0; k < 4; ++k) { const uint4 q = p[k]; local += q.x + q.y + q.z + q.w; }
  } else for (unsigned k = 0; k < 16u; ++k) if (i0 + k < n) local += counts[i0 + k];
  unsigned total;
  kf_block_excl_scan(local, s_wave, total);
  if (threadIdx.x == 0) partials[blockIdx.x] = total;
}
static __global__ void __launch_bounds__(256) k_scan_partials(unsigned* partials, unsigned n_chunks, unsigned* counts, unsigned n, unsigned* total_out) {
  __shared__ unsigned s_wave[4]; __shared__ unsigned s_carry;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  for (unsigned base = 0; base < n_chunks; base += 1024u) {
    const unsigned i0 = base + threadIdx.x * 4u;
    unsigned v[4]; unsigned local = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[k] = (i0 + k < n_chunks) ? partials[i0 + k] : 0u; local += v[k]; }
    unsigned total;
    unsigned excl = s_carry + kf_block_excl_scan(local, s_wave, total);
#pragma unroll
    for (int k = 0; k < 4; ++k) { if (i0 + k < n_chunks) partials[i0 + k] = excl; excl += v[k]; }
    __syncthreads();
    if (threadIdx.x == 0) s_carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) { counts[n] = s_carry; if (total_out) *total_out = s_carry; }
}
static __global__ void __launch_bounds__(256) k_scan_apply(unsigned* __restrict__ counts, unsigned n, const unsigned* __restrict__ partials) {
  __shared__ unsigned s_wave[4];
  const unsigned i0 = blockIdx.x * KF_SCAN_CHUNK + threadIdx.x * 16u;
  unsigned v[16]; unsigned local = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) { v[k] = (i0 + k < n) ? counts[i0 + k] : 0u; local += v[k]; }
  unsigned total;
  unsigned excl = partials[blockIdx.x] + kf_block_excl_scan(local, s_wave, total);
#pragma unroll
  for (int k = 0; k < 16; ++k) { if (i0 + k < n) counts[i0 + k] = excl; excl += v[k]; }
}
// the three launches; partials: at least ceil(n / KF_SCAN_CHUNK) words
static inline void kf_scan_in_place(unsigned* counts, unsigned n, unsigned* partials, unsigned* total_out, hipStream_t stream) {
  const unsigned n_chunks = (n + KF_SCAN_CHUNK - 1) / KF_SCAN_CHUNK;
  hipLaunchKernelGGL(k_scan_reduce, dim3(n_chunks), dim3(256), 0, stream, counts, n, partials);
  hipLaunchKernelGGL(k_scan_partials, dim3(1), dim3(256), 0, stream, partials, n_chunks, counts, n, total_out);
  hipLaunchKernelGGL(k_scan_apply, dim3(n_chunks), dim3(256), 0, stream, counts, n, partials);
}
