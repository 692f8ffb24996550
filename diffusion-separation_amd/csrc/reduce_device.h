// reduce_device.h — the fixed-order float64 block reductions behind "row (b, i) of a batch equals the B = 1 call bit for bit".
// ONE definition of the order, for every kernel outside the convolution stack:
//   1. the 64 lanes of a wave: butterfly v += v[lane ^ o], o = 32, 16, 8, 4, 2, 1 (every lane ends with the wave's total);
//   2. the NW wave totals through LDS, folded first to last: ((w0 + w1) + w2) + ... + w[NW-1], no leading zero.
// No floating-point atomics, nothing that depends on the grid, the stream or the batch.  tests/reduce_ref.py restates the order
// in NumPy and tests/test_reduce_order_gpu.py holds two entry points to it bit for bit.  Free functions only, all __device__
// inline in an anonymous namespace.  Included by stoi.hip, composite.hip, sde.hip, ode.hip, score_loss.hip, longform.hip and ensemble.hip;
// the block has NW * 64 threads and every thread of it makes the call.
#pragma once

#include "common.h"

namespace {

__device__ inline double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ inline double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// The total (maximum) of v over the block, returned to every thread.  sh: NW doubles of LDS.  One barrier before the LDS write
// (sh may be reused back to back, and whatever the block wrote to LDS before the call is published by it) and one after.
template <int NW>
__device__ inline double ds_block_sum_d(double v, double* sh) {
  v = wave_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = sh[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) r += sh[w];
  return r;
}
template <int NW>
__device__ inline double ds_block_max_d(double v, double* sh) {
  v = wave_max_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = sh[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) r = fmax(r, sh[w]);
  return r;
}

// n <= N values under one barrier pair: thread q < n returns the total of v[q] in the order above, the other threads' result
// is unspecified.  sh: N rows of NW doubles.
template <int NW, int N>
__device__ inline double ds_block_totals_d(const double* v, int n, double (*sh)[NW]) {
  __syncthreads();
#pragma unroll
  for (int q = 0; q < N; ++q) {
    if (q >= n) break;
    const double s = wave_sum_d(v[q]);
    if ((threadIdx.x & 63) == 0) sh[q][threadIdx.x >> 6] = s;
  }
  __syncthreads();
  const double* row = sh[(int)threadIdx.x < n ? threadIdx.x : 0];
  double r = row[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) r += row[w];
  return r;
}

}  // namespace
