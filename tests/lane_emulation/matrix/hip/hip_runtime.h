// Test infrastructure (tests/test_matching_lanes_cpu.py): the workgroup stand-in of ../../workgroup/hip/hip_runtime.h (a fibre
// per lane, workgroup-wide barriers) plus what csrc/pxr_match.hip needs on top of it: a stand-in for the f32-input MFMA builtin
// that states the instruction's documented semantics (operand and accumulator lane maps of the 32x32x2 form; per output element
// the k-ordered fmaf chain D = fmaf(a[k=1], b[k=1], fmaf(a[k=0], b[k=0], C))), __syncthreads_count and float4.  That the hardware
// instruction has these semantics is what tests/test_matching_gpu.py establishes; this header only lets the index arithmetic,
// the merges, the masks and the host code around the instruction run without a GPU.
#pragma once
#include "../../workgroup/hip/hip_runtime.h"

struct float4 { float x, y, z, w; };
inline float4 make_float4(float x, float y, float z, float w) { return {x, y, z, w}; }

typedef float emu_f32x16 __attribute__((ext_vector_type(16)));
// lane l feeds A[row = l & 31][k = l >> 5] and B[k = l >> 5][column = l & 31]; register r of lane l is
// D[row = (r & 3) + 8 (r >> 2) + 4 (l >> 5)][column = l & 31]
inline emu_f32x16 emu_mfma_f32_32x32x2f32(float a, float b, emu_f32x16 c, int, int, int) {
  EmuBlock& blk = emu_block;
  const int me = blk.cur, par = blk.calls[me]++ & 1, wave = me & ~63, l = me & 63;
  uint64_t w = 0; memcpy(&w, &a, 4); memcpy((char*)&w + 4, &b, 4); blk.xbuf[par][me] = w;
  emu_yield();
  auto a_of = [&](int lane) { float v; memcpy(&v, &blk.xbuf[par][wave + lane], 4); return v; };
  auto b_of = [&](int lane) { float v; memcpy(&v, (const char*)&blk.xbuf[par][wave + lane] + 4, 4); return v; };
  const int col = l & 31;
  emu_f32x16 d;
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
    d[r] = fmaf(a_of(row + 32), b_of(col + 32), fmaf(a_of(row), b_of(col), c[r]));
  }
  return d;
}
#define __builtin_amdgcn_mfma_f32_32x32x2f32 emu_mfma_f32_32x32x2f32

// the number of lanes of the workgroup whose predicate is non-zero
inline int __syncthreads_count(int pred) {
  EmuBlock& blk = emu_block;
  const int me = blk.cur, par = blk.calls[me]++ & 1;
  blk.xbuf[par][me] = pred ? 1 : 0;
  emu_yield();
  int n = 0;
  for (unsigned t = 0; t < blockDim.x; ++t) n += (int)blk.xbuf[par][t];
  return n;
}
