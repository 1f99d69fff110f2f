// pxr_spd_inverse.hip -- dense fp64 inverse of a symmetric positive definite matrix on gfx950: the covariance of the reduced
// camera system, Sigma_c = S^-1.
//
// A = L L^T comes from the blocked Cholesky of pxr_chol.hip (chol_factor_solve with a zero right-hand side), which leaves L
// below the diagonal tiles of the augmented matrix and, in its workspace, the inverses M_k = inv(L_kk) of the 64 x 64
// diagonal tiles' factors.  Then, in 64 x 64 tiles on v_mfma_f64_16x16x4_f64:
//   k_trinv_diag   T_kk = M_k (lower triangle, zeros above) into the tile grid of T = inv(L);
//   k_trinv_step   one launch per block column j = N - 2 .. 0, a workgroup per tile i > j:
//                      T_ij = -(sum_{k = j + 1 .. i} T_ik L_kj) M_j
//                  -- the left-looking form of T L = I: block column j needs only the block columns right of it, which the
//                  earlier launches wrote (the stream order is the dependency, as between two k_chol_step launches);
//   k_inv_product  one launch, a workgroup per tile i >= j:   X_ij = sum_{k >= i} T_ki^T T_kj   (X = T^T T = inv(A));
//   k_inv_mirror   the lower triangle and its mirror image into the caller's matrix: symmetric bit for bit.
// Every output tile has one owner and a fixed order of summation: no atomics, the same bits every run.
//
// Storage: T lives in the caller's n x n matrix (row-major, lower triangle; its input went into the augmented copy), X in the
// augmented matrix once L is no longer read (row-major, lower triangle, leading dimension n + 1).
#include <hip/hip_runtime.h>

#include "pxr_internal.h"

namespace pxr {

int chol_factor_solve(hipStream_t st, double* a, int n, int* d_info, double* linv_ws, double* x_out, bool zero_info);
size_t chol_workspace_doubles(int n);

namespace {

constexpr int INB = 64;
constexpr int IPAD = INB + 8;     // LDS row stride: spreads the four k-rows of an MFMA step over the banks
typedef double inv_d4 __attribute__((ext_vector_type(4)));

// operands of one tile product in MFMA order: C(ra, rb) += sum_m Pa[m][ra] Pb[m][rb]
struct InvLds {
  double Pa[INB][IPAD];
  double Pb[INB][IPAD];
};

// P[m][r] = base[m * stride_m + r * stride_r] for m < m_valid, r < r_valid, zero elsewhere (256 threads; the lanes run along the
// index that is contiguous in memory).  keep_lower: entries with r > m read as zero (a lower triangular tile)
template <bool M_CONTIGUOUS>
__device__ __forceinline__ void stage_tile(double (&P)[INB][IPAD], const double* __restrict__ base, size_t stride_m, size_t stride_r,
                                           int m_valid, int r_valid, bool keep_lower) {
#pragma unroll
  for (int q = 0; q < INB * INB / 256; ++q) {
    const int e = (int)threadIdx.x + 256 * q;
    const int f = e % INB, s = e / INB;
    const int m = M_CONTIGUOUS ? f : s, r = M_CONTIGUOUS ? s : f;
    // clamped address + select: no load outside the matrix
    const double v = base[(size_t)min(m, m_valid - 1) * stride_m + (size_t)min(r, r_valid - 1) * stride_r];
    P[m][r] = (m < m_valid && r < r_valid && !(keep_lower && r > m)) ? v : 0.0;
  }
}

// four wavefronts, each a 32 x 32 quarter of the tile = 2 x 2 MFMA blocks, K = 64 in 16 steps.  acc[x][y][t] is the element
//   ra = 32 wj + 16 x + (lane >> 4) + 4 t   (index of Pa),   rb = 32 wi + 16 y + (lane & 15)   (index of Pb)
// (C/D layout of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 * reg)
__device__ __forceinline__ void tile_mac(inv_d4 (&acc)[2][2], const InvLds& lds, int lane, int w) {
  const int lr = lane & 15, lk = lane >> 4, wi = w >> 1, wj = w & 1;
#pragma unroll 4
  for (int s = 0; s < INB / 4; ++s) {
    const int m = 4 * s + lk;
    const double a0 = lds.Pa[m][32 * wj + lr], a1 = lds.Pa[m][32 * wj + 16 + lr];
    const double b0 = lds.Pb[m][32 * wi + lr], b1 = lds.Pb[m][32 * wi + 16 + lr];
    acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
  }
}

__device__ __forceinline__ void zero_acc(inv_d4 (&acc)[2][2]) {
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) acc[x][y] = inv_d4{0.0, 0.0, 0.0, 0.0};
}

// T_kk = M_k: the diagonal tiles of T (row-major in t), zeros above the diagonal; the identity rows that pad a partial last tile
// in the workspace stay out
__global__ __launch_bounds__(256) void k_trinv_diag(const double* __restrict__ linv, double* __restrict__ t, int n) {
  const int k = blockIdx.x, k0 = k * INB;
  const double* M = linv + (size_t)k * INB * INB;
  for (int e = threadIdx.x; e < INB * INB; e += 256) {
    const int r = e / INB, c = e % INB;
    if (k0 + r < n && k0 + c < n) t[(size_t)(k0 + r) * n + (k0 + c)] = c <= r ? M[e] : 0.0;
  }
}

// block column j of T = inv(L): workgroup b owns tile (i, j), i = j + 1 + b
__global__ __launch_bounds__(256) void k_trinv_step(const double* __restrict__ aug, int ld, const double* __restrict__ linv,
                                                    double* __restrict__ t, int n, int j) {
  extern __shared__ __align__(16) unsigned char smem[];
  InvLds& lds = *reinterpret_cast<InvLds*>(smem);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int lr = lane & 15, lk = lane >> 4, wi = w >> 1, wj = w & 1;
  const int i = j + 1 + (int)blockIdx.x;
  const int i0 = i * INB, j0 = j * INB, rows_i = min(INB, n - i0);
  inv_d4 acc[2][2];
  zero_acc(acc);
  for (int k = j + 1; k <= i; ++k) {
    const int k0 = k * INB, nk = min(INB, n - k0);
    __syncthreads();                              // the previous product's operand reads
    // Pa[m][ra] = T_ik(ra, m): t is row-major;  Pb[m][rb] = L_kj(m, rb): aug is column-major (row n of aug, the right-hand side's
    // row, is not part of L: nk stops before it)
    stage_tile<true>(lds.Pa, t + (size_t)i0 * n + k0, 1, (size_t)n, nk, rows_i, false);
    stage_tile<true>(lds.Pb, aug + (size_t)k0 + (size_t)j0 * ld, 1, (size_t)ld, nk, INB, false);
    __syncthreads();
    tile_mac(acc, lds, lane, w);
  }
  __syncthreads();
  // G = sum T_ik L_kj sits in the accumulators as G(ra, rb); the second product T_ij(ra, c) = sum_m -G(ra, m) M_j(m, c) wants it
  // as Pa[m][ra]
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int r = 0; r < 4; ++r) lds.Pa[32 * wi + 16 * y + lr][32 * wj + 16 * x + lk + 4 * r] = -acc[x][y][r];
  stage_tile<false>(lds.Pb, linv + (size_t)j * INB * INB, (size_t)INB, 1, INB, INB, true);     // (j < N - 1: a full tile)
  __syncthreads();
  zero_acc(acc);
  tile_mac(acc, lds, lane, w);
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ra = 32 * wj + 16 * x + lk + 4 * r, rb = 32 * wi + 16 * y + lr;
        if (ra < rows_i) t[(size_t)(i0 + ra) * n + (j0 + rb)] = acc[x][y][r];
      }
}

// X = T^T T: workgroup b owns tile (i, j), i >= j, of the lower triangle; xs is row-major with leading dimension ld
__global__ __launch_bounds__(256) void k_inv_product(const double* __restrict__ t, int n, int n_tiles, double* __restrict__ xs, int ld) {
  extern __shared__ __align__(16) unsigned char smem[];
  InvLds& lds = *reinterpret_cast<InvLds*>(smem);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int lr = lane & 15, lk = lane >> 4, wi = w >> 1, wj = w & 1;
  int b = blockIdx.x, i = 0;
  while (b > i) { b -= i + 1; ++i; }              // tile b of row i: (i, b), b <= i
  const int j = b;
  const int i0 = i * INB, j0 = j * INB, rows_i = min(INB, n - i0), cols_j = min(INB, n - j0);
  inv_d4 acc[2][2];
  zero_acc(acc);
  for (int k = i; k < n_tiles; ++k) {
    const int k0 = k * INB, nk = min(INB, n - k0);
    __syncthreads();
    // Pa[m][ra] = T_ki(m, ra), Pb[m][rb] = T_kj(m, rb); the diagonal tiles of T hold zeros above the diagonal
    stage_tile<false>(lds.Pa, t + (size_t)k0 * n + i0, (size_t)n, 1, nk, rows_i, false);
    stage_tile<false>(lds.Pb, t + (size_t)k0 * n + j0, (size_t)n, 1, nk, cols_j, false);
    __syncthreads();
    tile_mac(acc, lds, lane, w);
  }
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ra = 32 * wj + 16 * x + lk + 4 * r, rb = 32 * wi + 16 * y + lr;
        if (ra < rows_i && rb < cols_j) xs[(size_t)(i0 + ra) * ld + (j0 + rb)] = acc[x][y][r];
      }
}

// out (n x n row-major) = the lower triangle of xs and its mirror image
__global__ __launch_bounds__(256) void k_inv_mirror(int n, const double* __restrict__ xs, int ld, double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)n * n) return;
  const int r = (int)(e / n), c = (int)(e % n);
  out[e] = r >= c ? xs[(size_t)r * ld + c] : xs[(size_t)c * ld + r];
}

// [S | 0] in the layout of chol_factor_solve from the upper triangle of a plain n x n row-major matrix
__global__ __launch_bounds__(256) void k_inv_pack(int n, const double* __restrict__ a, double* __restrict__ aug) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int ld = n + 1;
  if (e >= (int64_t)ld * ld) return;
  const int r = (int)(e / ld), c = (int)(e % ld);
  aug[e] = (r < n && c < n && r <= c) ? a[(size_t)r * n + c] : 0.0;
}

}  // namespace

size_t spd_inverse_max_n() { return (size_t)PXR_MAX_IMAGES_DIRECT * 18; }

// inv(A) = T^T T into out (n x n row-major, full) from the factor chol_factor_solve left in aug ((n + 1) x (n + 1)) and linv_ws;
// out holds T on the way, aug is overwritten by the lower triangle of the result
int spd_inverse_from_factor(hipStream_t st, double* aug, int n, double* out, const double* linv_ws) {
  const int N = (n + INB - 1) / INB, ld = n + 1;
  const size_t lds = sizeof(InvLds);
  if (int rc = hip_check(hipFuncSetAttribute((const void*)k_trinv_step, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), "LDS size")) return rc;
  if (int rc = hip_check(hipFuncSetAttribute((const void*)k_inv_product, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), "LDS size")) return rc;
  hipLaunchKernelGGL(k_trinv_diag, dim3(N), dim3(256), 0, st, linv_ws, out, n);
  for (int j = N - 2; j >= 0; --j)
    hipLaunchKernelGGL(k_trinv_step, dim3(N - 1 - j), dim3(256), lds, st, aug, ld, linv_ws, out, n, j);
  hipLaunchKernelGGL(k_inv_product, dim3((unsigned)((size_t)N * (N + 1) / 2)), dim3(256), lds, st, out, n, N, aug, ld);
  hipLaunchKernelGGL(k_inv_mirror, dim3((unsigned)(((size_t)n * n + 255) / 256)), dim3(256), 0, st, n, aug, ld, out);
  return hip_check(hipGetLastError(), "inverse launch");
}

// The inverse of the n x n matrix whose upper triangle is packed in aug ((n + 1) x (n + 1), the layout of chol_factor_solve, right-hand
// side zero) into out (n x n row-major, full).  out and aug are both overwritten; linv_ws: chol_workspace_doubles(n); x_scratch: n + 1
// doubles.  One host synchronisation, after the factorisation: *h_info = first non-positive pivot (then nothing more is launched).
static int spd_inverse_packed(hipStream_t st, double* aug, int n, double* out, double* linv_ws, double* x_scratch, int* d_info, int* h_info) {
  if (int rc = chol_factor_solve(st, aug, n, d_info, linv_ws, x_scratch, true)) return rc;
  if (int rc = hip_check(hipMemcpyAsync(h_info, d_info, sizeof(int), hipMemcpyDeviceToHost, st), "D2H info")) return rc;
  if (int rc = hip_check(hipStreamSynchronize(st), "sync")) return rc;
  if (*h_info != 0) return 0;
  return spd_inverse_from_factor(st, aug, n, out, linv_ws);
}

}  // namespace pxr

extern "C" int pxr_dense_spd_inverse(pxr_ctx* ctx, double* d_a, int n, int* h_info) {
  using namespace pxr;
  PXR_REQUIRE(ctx && d_a && h_info && n > 0, "pxr_dense_spd_inverse: invalid argument");
  PXR_REQUIRE((size_t)n <= spd_inverse_max_n(), "pxr_dense_spd_inverse: n = %d exceeds the direct solver's limit of %d columns", n,
              (int)spd_inverse_max_n());
  PXR_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  double *aug = nullptr, *linv = nullptr, *xs = nullptr;
  const size_t na = (size_t)(n + 1) * (n + 1), nl = chol_workspace_doubles(n);
  if (hipMalloc((void**)&aug, sizeof(double) * na) != hipSuccess || hipMalloc((void**)&linv, sizeof(double) * nl) != hipSuccess ||
      hipMalloc((void**)&xs, sizeof(double) * (size_t)(n + 1)) != hipSuccess) {
    (void)hipFree(aug); (void)hipFree(linv); (void)hipFree(xs);
    return set_error(PXR_ENOMEM, "pxr_dense_spd_inverse: workspace allocation failed");
  }
  int* d_info = reinterpret_cast<int*>(ctx->d_scratch);
  hipLaunchKernelGGL(k_inv_pack, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, st, n, d_a, aug);
  int rc = spd_inverse_packed(st, aug, n, d_a, linv, xs, d_info, h_info);
  if (!rc) rc = hip_check(hipStreamSynchronize(st), "sync");
  (void)hipFree(aug); (void)hipFree(linv); (void)hipFree(xs);
  return rc;
}
