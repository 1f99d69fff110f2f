// Test infrastructure (tests/test_triangulation_lanes_cpu.py): a stand-in for <hip/hip_runtime.h> under which
// csrc/pxr_triangulate.hip compiles as HOST C++ and runs without a GPU -- one std::thread per lane, a workgroup at a time;
// the cross-lane operations of a 16-lane group (__shfl, __shfl_xor, __ballot, the DPP row permutations behind row16_sum) go
// through an exchange buffer and a pthread barrier, which works because every branch around them is uniform over the group.
// "Device" pointers are host pointers.  Only what that translation unit and the headers it includes use is provided.
#pragma once
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <thread>
#include <vector>
#define __device__
#define __host__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(...)
#define __shared__ static
using std::isfinite; using std::max; using std::min;
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct uint3e { unsigned x, y, z; };
extern thread_local uint3e threadIdx, blockIdx, blockDim;
struct double2 { double x, y; };
inline double2 make_double2(double a, double b) { return {a, b}; }
typedef int hipError_t; enum { hipSuccess = 0 };
typedef void* hipStream_t; typedef void* hipEvent_t;
enum { hipMemcpyDeviceToHost, hipMemcpyHostToDevice, hipMemcpyDeviceToDevice };
inline const char* hipGetErrorString(hipError_t) { return "emu"; }
inline hipError_t hipSetDevice(int) { return 0; }
inline hipError_t hipGetLastError() { return 0; }
inline hipError_t hipStreamSynchronize(hipStream_t) { return 0; }
inline hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, int, hipStream_t) { memcpy(d, s, n); return 0; }
inline hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t) { memset(d, v, n); return 0; }
inline hipError_t hipMalloc(void** p, size_t n) { *p = malloc(n); return 0; }
inline hipError_t hipFree(void* p) { free(p); return 0; }
inline hipError_t hipEventCreate(hipEvent_t* e) { *e = (void*)1; return 0; }
inline hipError_t hipEventDestroy(hipEvent_t) { return 0; }
inline hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return 0; }
inline hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0; return 0; }
inline double __longlong_as_double(long long v) { double d; memcpy(&d, &v, 8); return d; }
inline long long __double_as_longlong(double v) { long long d; memcpy(&d, &v, 8); return d; }
inline long long __double2ll_rn(double v) { return llrint(v); }
inline double __fma_rn(double a, double b, double c) { return fma(a, b, c); }
inline float __fmaf_rn(float a, float b, float c) { return fmaf(a, b, c); }
inline float __fsub_rn(float a, float b) { return a - b; }
inline float __fmul_rn(float a, float b) { return a * b; }
inline double __dsub_rn(double a, double b) { return a - b; }
inline double __dmul_rn(double a, double b) { return a * b; }
template <class T> inline T atomicAdd(T* p, T v) { T o = *p; *p += v; return o; }
inline int atomicOr(int* p, int v) { return __atomic_fetch_or(p, v, __ATOMIC_SEQ_CST); }
inline void __threadfence_block() {}
inline void __syncthreads() {}
// ---- 16-lane groups
struct EmuGroup { pthread_barrier_t bar; uint64_t buf[16]; };
extern EmuGroup emu_groups[16];
inline void emu_wait() { pthread_barrier_wait(&emu_groups[threadIdx.x / 16].bar); }
template <class T> inline T emu_read(T v, int src) {
  EmuGroup& g = emu_groups[threadIdx.x / 16];
  uint64_t w = 0; memcpy(&w, &v, sizeof(T)); g.buf[threadIdx.x & 15] = w;
  emu_wait();
  T out; w = g.buf[src & 15]; memcpy(&out, &w, sizeof(T));
  emu_wait();
  return out;
}
template <class T> inline T __shfl_xor(T v, int m, int = 64) { return emu_read(v, (int)(threadIdx.x & 15) ^ m); }
template <class T> inline T __shfl(T v, int src, int = 64) { return emu_read(v, src); }
inline unsigned long long __ballot(bool p) {
  EmuGroup& g = emu_groups[threadIdx.x / 16];
  g.buf[threadIdx.x & 15] = p;
  emu_wait();
  unsigned long long m = 0;
  for (int i = 0; i < 16; ++i) if (g.buf[i]) m |= 1ull << (16 * ((threadIdx.x / 16) & 3) + i);
  emu_wait();
  return m;
}
inline int emu_update_dpp(int, int src, int ctrl, int, int, bool) {
  const int l = threadIdx.x & 15;
  const int from = ctrl == 0xB1 ? (l ^ 1) : ctrl == 0x4E ? (l ^ 2) : ctrl == 0x141 ? ((l & 8) | (7 - (l & 7))) : (15 - l);
  return emu_read(src, from);
}
#define __builtin_amdgcn_update_dpp emu_update_dpp
#define __builtin_amdgcn_wave_barrier emu_wait
template <class K, class... A> void emu_launch(K kernel, dim3 grid, dim3 block, A... args) {
  for (unsigned b = 0; b < grid.x; ++b) {
    for (int g = 0; g < 16; ++g) pthread_barrier_init(&emu_groups[g].bar, nullptr, 16);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < block.x; ++t)
      th.emplace_back([=]() { threadIdx = {t, 0, 0}; blockIdx = {b, 0, 0}; blockDim = {block.x, 1, 1}; kernel(args...); });
    for (auto& x : th) x.join();
    for (int g = 0; g < 16; ++g) pthread_barrier_destroy(&emu_groups[g].bar);
  }
}
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...) emu_launch(kernel, grid, block, __VA_ARGS__)
