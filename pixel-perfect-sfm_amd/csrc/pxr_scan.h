// pxr_scan.h -- the integer prefix sums and workgroup sums of the device code (DESIGN.md "Prefix sums"): every count -> scan ->
// write pipeline of csrc/ takes them from here.  Integers only: the result of an integer sum does not depend on how the additions
// are grouped (wrap-around of the unsigned types included), so these may regroup freely; a floating-point sum has an order to
// keep and does not belong here (block_sum of pxr_robust.h / pxr_ka.hip, the wave_sum variants, the DPP row sums).
//
// The two block functions hold __syncthreads and shuffles: every thread of the workgroup calls them, under uniform control flow.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

namespace pxr {

// the exclusive prefix of v over the workgroup in thread order, and the workgroup's total; s_part has THREADS / 64 slots
template <int THREADS, class T>
__device__ __forceinline__ T block_exclusive_scan(T v, T* s_part, T& total) {
  static_assert(std::is_integral<T>::value, "block_exclusive_scan regroups the additions: integers only");
  static_assert(THREADS % 64 == 0, "whole wavefronts");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T up = __shfl(inc, lane >= d ? lane - d : 0, 64);
    if (lane >= d) inc += up;
  }
  __syncthreads();                              // (the previous use of s_part is over)
  if (lane == 63) s_part[wave] = inc;
  __syncthreads();
  T before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < THREADS / 64; ++w) { if (w < wave) before += s_part[w]; total += s_part[w]; }
  return before + inc - v;
}

// the sum of v over the workgroup, on every thread; s_part has THREADS / 64 slots
template <int THREADS, class T>
__device__ __forceinline__ T block_int_sum(T v, T* s_part) {
  static_assert(std::is_integral<T>::value, "block_int_sum regroups the additions: integers only");
  static_assert(THREADS % 64 == 0, "whole wavefronts");
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();                              // (the previous use of s_part is over)
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
  __syncthreads();
  T sum = 0;
#pragma unroll
  for (int w = 0; w < THREADS / 64; ++w) sum += s_part[w];
  return sum;
}

// out[i] = in[0] + ... + in[i - 1] for i < n, summed in OUT, and out[n] = the total when write_total is set: ONE workgroup of
// THREADS threads, thread t owns the contiguous chunk [t per, min(n, (t + 1) per)) with per = ceil(n / THREADS).
// `in` may alias `out` when IN and OUT have the same size: every element is read and written by the same thread, read first
// (hence no __restrict__).
template <int THREADS, class IN, class OUT>
__global__ __launch_bounds__(THREADS) void k_exclusive_scan(int64_t n, const IN* in, OUT* out, int write_total) {
  __shared__ OUT s_part[THREADS / 64];
  const int64_t per = (n + THREADS - 1) / THREADS, t0 = (int64_t)threadIdx.x * per, t1 = min(n, t0 + per);
  OUT s = 0;
  for (int64_t i = t0; i < t1; ++i) s += (OUT)in[i];
  OUT total;
  OUT run = block_exclusive_scan<THREADS, OUT>(s, s_part, total);
  for (int64_t i = t0; i < t1; ++i) { const OUT c = (OUT)in[i]; out[i] = run; run += c; }
  if (write_total && threadIdx.x == 0) out[n] = total;
}

}  // namespace pxr
