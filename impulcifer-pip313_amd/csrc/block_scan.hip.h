// Reductions and the inclusive scan of one workgroup of kDecayThreads threads: what the decay kernels (ir_kernels.hip.h) and
// the energy decay curve (analysis_kernels.hip.h) share.
#pragma once
#include <hip/hip_runtime.h>

namespace imp {

constexpr int kDecayThreads = 1024;     // one workgroup per response: its threads share the scans and the line fits

__device__ inline double block_sum(double v, double* red) {
  const int t = threadIdx.x;
  __syncthreads();
  red[t] = v;
  __syncthreads();
  for (int s = kDecayThreads / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  return red[0];
}
__device__ inline double block_max(double v, double* red) {
  const int t = threadIdx.x;
  __syncthreads();
  red[t] = v;
  __syncthreads();
  for (int s = kDecayThreads / 2; s > 0; s >>= 1) {
    if (t < s) red[t] = fmax(red[t], red[t + s]);
    __syncthreads();
  }
  return red[0];
}
__device__ inline long long block_min_ll(long long v, long long* red) {
  const int t = threadIdx.x;
  __syncthreads();
  red[t] = v;
  __syncthreads();
  for (int s = kDecayThreads / 2; s > 0; s >>= 1) {
    if (t < s && red[t + s] < red[t]) red[t] = red[t + s];
    __syncthreads();
  }
  return red[0];
}
// inclusive scan of f(0..len) into out[0..len): tiles of kDecayThreads consecutive elements (coalesced loads and stores,
// f once per element), a shuffle scan inside every wave, the waves' totals and the running carry through LDS
template <class F>
__device__ inline void block_scan(F f, long long len, double* out, double* red) {
  constexpr int kWaves = kDecayThreads / 64;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  double carry = 0.0;
  for (long long base = 0; base < len; base += kDecayThreads) {
    const long long i = base + t;
    double v = i < len ? f(i) : 0.0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const double u = __shfl_up(v, d, 64);
      if (lane >= d) v += u;
    }
    __syncthreads();
    if (lane == 63) red[w] = v;
    __syncthreads();
    double before = carry, total = 0.0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
      const double r = red[k];
      if (k < w) before += r;
      total += r;
    }
    if (i < len) out[i] = v + before;
    carry += total;
  }
  __syncthreads();
}

}  // namespace imp
