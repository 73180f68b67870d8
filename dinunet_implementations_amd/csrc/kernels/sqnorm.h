// fp64 squared-norm partials of a flat fp32 gradient, shared by the clipped Adam (optim.hip
// ClipState) and the differentially private release (dp.hip DpState): a fixed grid of
// SQNORM_PARTS workgroups, every partial rewritten by every launch, and one fixed summation
// order in the consumer -- the same data always gives the same bits, with no atomics, no
// finalize launch and no "last workgroup" ticket.
#pragma once
#include "common.h"

constexpr int SQNORM_PARTS = 256;  // one workgroup per CU; ~4 float4 per thread at 1 M elements

__device__ __forceinline__ double wave_sum_f64(double x) {  // fixed butterfly: all lanes agree
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

// The 256 threads' accumulators of a workgroup summed in one fixed order into *slot (every thread
// of the workgroup calls it).
__device__ __forceinline__ void sqnorm_block_sum(double acc, double* __restrict__ slot) {
  __shared__ double wsum[4];
  acc = wave_sum_f64(acc);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) *slot = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// Body of a <<<SQNORM_PARTS, 256>>> launch: part[blockIdx.x] = sum of g^2 over this workgroup's
// grid-stride share of the n4 float4 of g.
__device__ __forceinline__ void sqnorm_partial(const float* __restrict__ g, long n4,
                                               double* __restrict__ part) {
  double acc = 0.0;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const f32x4 gg = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc += (double)gg[e] * (double)gg[e];
  }
  sqnorm_block_sum(acc, part + blockIdx.x);
}

// The partials summed in one fixed order (all 64 lanes of the wave active; every lane gets the
// same bits).
__device__ __forceinline__ double sqnorm_total(const double* __restrict__ part) {
  const int l = threadIdx.x & 63;
  return wave_sum_f64((part[l] + part[l + 64]) + (part[l + 128] + part[l + 192]));
}
