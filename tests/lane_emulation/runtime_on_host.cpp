// The stand-in runtime itself, held to what hip/hip_runtime.h says of it (tests/test_lane_runtime_cpu.py): one small kernel per
// primitive, written as a csrc kernel writes it, behind entry points that launch it on host arrays.
#include "on_host.h"
#include "pxr_device.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ size_t global_lane() { return (size_t)blockIdx.x * blockDim.x + threadIdx.x; }

__global__ void k_shuffles(const double* v, const int* src, int mask, int width, double* picked, double* swapped) {
  const size_t i = global_lane();
  picked[i] = __shfl(v[i], src[i], width);
  swapped[i] = __shfl_xor(v[i], mask, width);
}

__global__ void k_row_sums(const double* v, double* sum16, double* sum8) {
  const size_t i = global_lane();
  sum16[i] = pxr::row16_sum(v[i]);
  sum8[i] = pxr::row8_sum(v[i]);
}

__global__ void k_ballot(const int* pred, unsigned long long* mask) {
  const size_t i = global_lane();
  mask[i] = __ballot(pred[i]);
}

__global__ void k_count(const int* pred, int* count) {
  const size_t i = global_lane();
  count[i] = __syncthreads_count(pred[i]);
}

// D = A B + C on one wavefront: A is 32 x K, B is K x 32, row-major, K even; two values of k per instruction, k ascending
__global__ void k_mfma(const float* A, const float* B, const float* C, int K, float* D) {
  const int l = threadIdx.x, col = l & 31, half = l >> 5;
  f32x16 acc;
  for (int r = 0; r < 16; ++r) acc[r] = C[((r & 3) + 8 * (r >> 2) + 4 * half) * 32 + col];
  for (int k = 0; k < K; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(A[(l & 31) * K + k + half], B[(k + half) * 32 + col], acc, 0, 0, 0);
  for (int r = 0; r < 16; ++r) D[((r & 3) + 8 * (r >> 2) + 4 * half) * 32 + col] = acc[r];
}

__global__ void k_cas(unsigned long long* slot, const unsigned long long* expected, const unsigned long long* desired, unsigned long long* was) {
  const size_t i = global_lane();
  was[i] = atomicCAS(slot + i, expected[i], desired[i]);
}

__global__ void k_indices(int* block, int* thread, int* dim) {
  const size_t i = global_lane();
  block[i] = blockIdx.x; thread[i] = threadIdx.x; dim[i] = blockDim.x;
}

// 16-lane groups on paths of their own: every fourth returns at once, the others sum their values once, twice or three times over
__global__ void k_groups(const double* v, double* out) {
  const size_t i = global_lane();
  const int group = threadIdx.x / 16;
  out[i] = -1.0;
  if (group % 4 == 3) return;
  double s = v[i];
  for (int round = 0; round <= group % 3; ++round)
    for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off, 16);
  out[i] = s;
}

extern "C" {
void emu_groups(int grid, int block, const double* v, double* out) {
  hipLaunchKernelGGL(k_groups, dim3(grid), dim3(block), 0, nullptr, v, out);
}
void emu_shuffles(int grid, int block, const double* v, const int* src, int mask, int width, double* picked, double* swapped) {
  hipLaunchKernelGGL(k_shuffles, dim3(grid), dim3(block), 0, nullptr, v, src, mask, width, picked, swapped);
}
void emu_row_sums(int grid, int block, const double* v, double* sum16, double* sum8) {
  hipLaunchKernelGGL(k_row_sums, dim3(grid), dim3(block), 0, nullptr, v, sum16, sum8);
}
void emu_ballot(int grid, int block, const int* pred, unsigned long long* mask) {
  hipLaunchKernelGGL(k_ballot, dim3(grid), dim3(block), 0, nullptr, pred, mask);
}
void emu_count(int grid, int block, const int* pred, int* count) {
  hipLaunchKernelGGL(k_count, dim3(grid), dim3(block), 0, nullptr, pred, count);
}
void emu_mfma(const float* A, const float* B, const float* C, int K, float* D) {
  hipLaunchKernelGGL(k_mfma, dim3(1), dim3(64), 0, nullptr, A, B, C, K, D);
}
void emu_cas(int grid, int block, unsigned long long* slot, const unsigned long long* expected, const unsigned long long* desired,
             unsigned long long* was) {
  hipLaunchKernelGGL(k_cas, dim3(grid), dim3(block), 0, nullptr, slot, expected, desired, was);
}
void emu_indices(int grid, int block, int* block_of, int* thread_of, int* dim_of) {
  hipLaunchKernelGGL(k_indices, dim3(grid), dim3(block), 0, nullptr, block_of, thread_of, dim_of);
}
}
