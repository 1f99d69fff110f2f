// Test infrastructure (tests/test_abspose_lanes_cpu.py): a stand-in for <hip/hip_runtime.h> under which csrc/pxr_abspose.hip
// compiles as HOST C++ and runs without a GPU.  Unlike ../../hip/hip_runtime.h (a thread per lane, 16-lane groups) this one
// runs a whole workgroup with WORKGROUP-WIDE barriers: every lane is a fibre (ucontext) of one thread, resumed in lane order;
// __syncthreads and the cross-lane operations (__shfl, __shfl_xor over the 64 lanes of a wavefront, the DPP row permutations
// behind row16_sum) hand control back to the scheduler, which works because every branch around them is uniform over the
// workgroup.  "Device" pointers are host pointers.  Only what that translation unit and the headers it includes use is provided.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <ucontext.h>

#include <algorithm>
#include <cmath>
#include <functional>
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
extern uint3e threadIdx, blockIdx, blockDim;      // of the fibre that runs (set by the scheduler at every resume)
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
inline int atomicOr(int* p, int v) { int o = *p; *p |= v; return o; }
inline void __threadfence_block() {}

// ---- the workgroup: fibres and their scheduler
constexpr int EMU_MAX_THREADS = 1024;
constexpr size_t EMU_STACK = 512 * 1024;
struct EmuBlock {
  ucontext_t sched, ctx[EMU_MAX_THREADS];
  bool done[EMU_MAX_THREADS];
  unsigned calls[EMU_MAX_THREADS];                 // cross-lane exchanges a fibre has made (the same on all: uniform control flow)
  uint64_t xbuf[2][EMU_MAX_THREADS];               // two exchange buffers, used in turn
  int cur, live;
  std::function<void()> body;
};
extern EmuBlock emu_block;
inline void emu_yield() { swapcontext(&emu_block.ctx[emu_block.cur], &emu_block.sched); }
inline void __syncthreads() { emu_yield(); }
// every lane of the workgroup deposits v, then reads the deposit of workgroup lane `src`
template <class T> inline T emu_read(T v, int src) {
  static_assert(sizeof(T) <= 8, "exchange of at most 8 bytes");
  EmuBlock& b = emu_block;
  const int me = b.cur, par = b.calls[me]++ & 1;
  uint64_t w = 0; memcpy(&w, &v, sizeof(T)); b.xbuf[par][me] = w;
  emu_yield();
  T out; w = b.xbuf[par][src]; memcpy(&out, &w, sizeof(T));
  return out;
}
template <class T> inline T __shfl_xor(T v, int m, int width = 64) {
  const int t = threadIdx.x;
  return emu_read(v, (t & ~(width - 1)) | ((t ^ m) & (width - 1)));
}
template <class T> inline T __shfl(T v, int src, int width = 64) {
  const int t = threadIdx.x;
  return emu_read(v, (t & ~(width - 1)) | (src & (width - 1)));
}
inline int emu_update_dpp(int, int src, int ctrl, int, int, bool) {
  const int t = threadIdx.x, l = t & 15;
  const int from = ctrl == 0xB1 ? (l ^ 1) : ctrl == 0x4E ? (l ^ 2) : ctrl == 0x141 ? ((l & 8) | (7 - (l & 7))) : (15 - l);
  return emu_read(src, (t & ~15) | from);
}
#define __builtin_amdgcn_update_dpp emu_update_dpp
#define __builtin_amdgcn_wave_barrier emu_yield
inline void emu_fibre_main() {
  EmuBlock& b = emu_block;
  b.body();
  b.done[b.cur] = true;
  --b.live;
  swapcontext(&b.ctx[b.cur], &b.sched);            // never resumed
}
template <class K, class... A> void emu_launch(K kernel, dim3 grid, dim3 block, A... args) {
  EmuBlock& b = emu_block;
  const int n = (int)block.x;
  std::vector<char> stacks((size_t)n * EMU_STACK);
  b.body = [=]() { kernel(args...); };
  blockDim = {block.x, 1, 1};
  for (unsigned g = 0; g < grid.x; ++g) {
    blockIdx = {g, 0, 0};
    for (int t = 0; t < n; ++t) {
      getcontext(&b.ctx[t]);
      b.ctx[t].uc_stack.ss_sp = stacks.data() + (size_t)t * EMU_STACK;
      b.ctx[t].uc_stack.ss_size = EMU_STACK;
      b.ctx[t].uc_link = nullptr;
      makecontext(&b.ctx[t], emu_fibre_main, 0);
      b.done[t] = false; b.calls[t] = 0;
    }
    b.live = n;
    while (b.live > 0)
      for (int t = 0; t < n; ++t) {
        if (b.done[t]) continue;
        b.cur = t;
        threadIdx = {(unsigned)t, 0, 0};
        swapcontext(&b.sched, &b.ctx[t]);
      }
  }
}
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...) emu_launch(kernel, grid, block, __VA_ARGS__)
