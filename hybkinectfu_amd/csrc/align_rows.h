// align_rows.h -- the device side the two Gauss-Newton evaluations share (align.hip: k_store_align_sums, a map against the brick store; relocal.hip: k_pose_sums,
// a point set against the map): how a row (J, e) enters a lane's 28 sums and how a workgroup of 256 lanes folds them into its row of 29 doubles.  The layout is
// align_step.h's, so kf_align_step applies to both kernels' sums unchanged.  No reference counterpart.  No atomic on a float anywhere: the same bits on every run.
#pragma once
#include "align_step.h"

// a transform or pose and the centre its rotations are taken about, as the kernels read them: 15 doubles
struct KfAlignXf { double m[12]; double c[3]; };

// the row's 21 + 6 + 1 products, each exact in fp64 (both factors are fp32 values), added to the lane's sums; 1 to its count
__device__ __forceinline__ void align_row_add(const double (&J)[6], double e, double (&acc)[28], unsigned& n) {
  int k = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = a; b < 6; ++b, ++k) acc[k] += J[a] * J[b];
#pragma unroll
  for (int a = 0; a < 6; ++a) acc[21 + a] += J[a] * e;
  acc[27] += e * e;
  n += 1u;
}

// The end of a sums kernel, reached by all 256 lanes: the wave's lanes by the butterfly xor 32 .. 1 (every lane ends with the same sum), the four waves through
// LDS in wave order, ((w0 + w1) + w2) + w3, and the workgroup's row of 29 doubles to `row`.  The count is exact as an integer and as a double (at most 2^24
// rows a lane in either kernel).
__device__ __forceinline__ void align_rows_fold(double (&acc)[28], unsigned n, double* __restrict__ row) {
  __shared__ double s_red[4][KF_ALIGN_SUMS];
#pragma unroll
  for (int k = 0; k < 28; ++k) {
    double v = acc[k];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    acc[k] = v;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) n += (unsigned)__shfl_xor((int)n, m);
  if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
    for (int k = 0; k < 28; ++k) s_red[threadIdx.x >> 6][k] = acc[k];
    s_red[threadIdx.x >> 6][28] = (double)n;
  }
  __syncthreads();
  if (threadIdx.x < KF_ALIGN_SUMS)
    row[threadIdx.x] = ((s_red[0][threadIdx.x] + s_red[1][threadIdx.x]) + s_red[2][threadIdx.x]) + s_red[3][threadIdx.x];
}
