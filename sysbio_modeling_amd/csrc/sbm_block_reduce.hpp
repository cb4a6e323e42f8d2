// sbm_block_reduce.hpp -- the reductions of the library's own kernels (sbm_core.hip and the headers it includes): a
// butterfly over the 64 lanes of a wavefront, a sum over a workgroup, and the "neither infinite nor NaN" test.
// Not for the model plugins: their sbm_wave_sum / sbm_wave_max (sbm_wave.hpp) broadcast through DPP.
#ifndef SBM_BLOCK_REDUCE_HPP
#define SBM_BLOCK_REDUCE_HPP

#include <hip/hip_runtime.h>
#include <float.h>

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

// sum over the workgroup, the same value on every thread: the wavefront partials are added in wavefront order, starting
// from +0.0 (an all-zero sum comes out as +0.0 whatever the signs of its terms).  red: one double per wavefront, in LDS
__device__ __forceinline__ double block_sum(double v, double* red /*[blockDim.x >> 6]*/) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  double s = 0.0;
  const int nw = blockDim.x >> 6;
  for (int i = 0; i < nw; ++i) s += red[i];
  return s;
}

__device__ __forceinline__ bool is_finite(double x) { return fabs(x) <= DBL_MAX; }      // (false for NaN)

#endif  // SBM_BLOCK_REDUCE_HPP
