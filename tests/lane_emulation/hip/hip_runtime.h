// Test infrastructure (tests/lanes.py, tests/test_*_lanes_cpu.py): the stand-in for <hip/hip_runtime.h> under which a csrc/*.hip
// file compiles as HOST C++ and runs without a GPU.  "Device" pointers are host pointers, a launch runs its workgroups one after
// another, and every lane of a workgroup is a fibre (ucontext) of the one calling thread.  Only what the emulated translation
// units and the headers they include use is provided.
//
// The scheduler resumes the live lanes of a workgroup in lane order, round after round; a lane runs until its next cross-lane
// call (__syncthreads, __syncthreads_count, __shfl, __shfl_xor, __ballot, a DPP row permutation, the MFMA stand-in, the wave
// barrier), where it deposits its operand and yields, and reads the other lanes' deposits when its turn comes again.
//  - Lanes that execute the same sequence of cross-lane calls stay in lockstep: call number k of one is answered by call number
//    k of the others.  This is all a kernel may rely on, and all it needs when every branch around a cross-lane call is uniform
//    over the lanes that exchange there (a 16-lane group, a wavefront, the workgroup).  Groups that take different paths, or
//    return early, do not disturb each other as long as no lane reads across groups.
//  - What a lane reads of a lane that did not execute the same call is stale: a __ballot bit, a shuffled value or a
//    __syncthreads_count addend of such a lane is not meaningful.
//  - __syncthreads is one scheduler round, so it is a true barrier only under workgroup-uniform control flow.
//  - Lanes never run at the same time: atomics are plain read-modify-writes, and nothing here shows what real concurrency, LDS
//    banking, occupancy or the device's libm do.  The MFMA stand-in states the instruction's documented lane maps and fmaf chain;
//    that the hardware computes them is established by the GPU tests.
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
struct float4 { float x, y, z, w; };
inline float4 make_float4(float x, float y, float z, float w) { return {x, y, z, w}; }
typedef int hipError_t; enum { hipSuccess = 0 };
typedef void* hipStream_t; typedef void* hipEvent_t;
enum { hipMemcpyDeviceToHost, hipMemcpyHostToDevice, hipMemcpyDeviceToDevice };
inline const char* hipGetErrorString(hipError_t) { return "emu"; }
inline hipError_t hipSetDevice(int) { return 0; }
inline hipError_t hipGetLastError() { return 0; }
inline hipError_t hipStreamSynchronize(hipStream_t) { return 0; }
inline hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, int, hipStream_t) { memcpy(d, s, n); return 0; }
inline hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t) { memset(d, v, n); return 0; }
inline int emu_malloc_calls = 0, emu_malloc_failures = 0;    // hipMalloc calls so far; how many of the next ones fail (workspace_on_host.cpp)
inline hipError_t hipMalloc(void** p, size_t n) {
  ++emu_malloc_calls;
  if (emu_malloc_failures > 0) { --emu_malloc_failures; *p = nullptr; return 2; }
  *p = malloc(n);
  return 0;
}
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
inline unsigned long long atomicCAS(unsigned long long* p, unsigned long long expected, unsigned long long desired) {
  const unsigned long long was = *p;
  if (was == expected) *p = desired;
  return was;
}
inline void __threadfence_block() {}

// ---- the workgroup: fibres and their scheduler
constexpr int EMU_MAX_THREADS = 1024;
constexpr size_t EMU_STACK = 512 * 1024;
struct EmuBlock {
  ucontext_t sched, ctx[EMU_MAX_THREADS];
  bool done[EMU_MAX_THREADS];
  unsigned calls[EMU_MAX_THREADS];                 // exchanges a fibre has made (the same on all lanes in lockstep)
  uint64_t xbuf[2][EMU_MAX_THREADS];               // two exchange buffers, used in turn: a lane that is one call ahead writes the other
  int cur, live;
  std::function<void()> body;
};
extern EmuBlock emu_block;
inline void emu_yield() { swapcontext(&emu_block.ctx[emu_block.cur], &emu_block.sched); }
inline void __syncthreads() { emu_yield(); }
// the running lane deposits w and yields; returns the deposits of that exchange, by workgroup lane
inline const uint64_t* emu_exchange(uint64_t w) {
  EmuBlock& b = emu_block;
  const int par = b.calls[b.cur]++ & 1;
  b.xbuf[par][b.cur] = w;
  emu_yield();
  return b.xbuf[par];
}
// every lane deposits v, then reads the deposit of workgroup lane `src`
template <class T> inline T emu_read(T v, int src) {
  static_assert(sizeof(T) <= 8, "exchange of at most 8 bytes");
  uint64_t w = 0; memcpy(&w, &v, sizeof(T));
  w = emu_exchange(w)[src];
  T out; memcpy(&out, &w, sizeof(T));
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
// bit i: the predicate of lane i of the caller's wavefront, over the lanes the workgroup has
inline unsigned long long __ballot(int pred) {
  const int wave = threadIdx.x & ~63u;
  const uint64_t* x = emu_exchange(pred != 0);
  unsigned long long m = 0;
  for (int i = 0; i < 64 && wave + i < (int)blockDim.x; ++i) m |= (unsigned long long)(x[wave + i] != 0) << i;
  return m;
}
// the number of lanes of the workgroup whose predicate is non-zero
inline int __syncthreads_count(int pred) {
  const uint64_t* x = emu_exchange(pred != 0);
  int n = 0;
  for (unsigned t = 0; t < blockDim.x; ++t) n += (int)x[t];
  return n;
}
// the DPP row permutations behind row16_sum / row8_sum: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror
inline int emu_update_dpp(int, int src, int ctrl, int, int, bool) {
  const int t = threadIdx.x, l = t & 15;
  const int from = ctrl == 0xB1 ? (l ^ 1) : ctrl == 0x4E ? (l ^ 2) : ctrl == 0x141 ? ((l & 8) | (7 - (l & 7))) : (15 - l);
  return emu_read(src, (t & ~15) | from);
}
#define __builtin_amdgcn_update_dpp emu_update_dpp
#define __builtin_amdgcn_wave_barrier emu_yield

// the f32-input MFMA, 32x32x2 form: lane l feeds A[row = l & 31][k = l >> 5] and B[k = l >> 5][column = l & 31]; register r of
// lane l is D[row = (r & 3) + 8 (r >> 2) + 4 (l >> 5)][column = l & 31] = fmaf(a[k=1], b[k=1], fmaf(a[k=0], b[k=0], C))
typedef float emu_f32x16 __attribute__((ext_vector_type(16)));
inline emu_f32x16 emu_mfma_f32_32x32x2f32(float a, float b, emu_f32x16 c, int, int, int) {
  const int wave = threadIdx.x & ~63u, l = threadIdx.x & 63;
  uint64_t w = 0; memcpy(&w, &a, 4); memcpy((char*)&w + 4, &b, 4);
  const uint64_t* x = emu_exchange(w) + wave;
  auto a_of = [&](int lane) { float v; memcpy(&v, &x[lane], 4); return v; };
  auto b_of = [&](int lane) { float v; memcpy(&v, (const char*)&x[lane] + 4, 4); return v; };
  const int col = l & 31;
  emu_f32x16 d;
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
    d[r] = fmaf(a_of(row + 32), b_of(col + 32), fmaf(a_of(row), b_of(col), c[r]));
  }
  return d;
}
#define __builtin_amdgcn_mfma_f32_32x32x2f32 emu_mfma_f32_32x32x2f32

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
