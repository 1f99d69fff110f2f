// pxr_ba_cov.hip -- covariance of a bundle adjustment: blocks of inv(H) for poses, intrinsics and points (pxr_ba_covariance).
//
// Replaces ceres::Covariance::Compute / GetCovarianceBlockInTangentSpace as COLMAP's EstimateBACovariance drives them
// [upstream COLMAP estimators/covariance.cc; pycolmap.estimate_ba_covariance].
//
// Everything expensive about a covariance is what the LM loop builds at every iteration, and it is built by the LM loop's own
// code (ba_cov_system, pxr_ba_solve.hip): structure, k_jac, the point blocks V, the camera blocks U and the reduced camera matrix
// S = U - W inv(V) W^T in the fixed-point sums of the deterministic mode -- undamped, its columns scaled by powers of two.  Here:
//   pxr_chol / pxr_spd_inverse   Sigma_s = inv(S_scaled), dense, on the fp64 matrix pipe;
//   k_cov_points                 per variable point  Sigma_p = T + T (W_p^T Sigma_s[cols(p), cols(p)] W_p) T,  T = inv(V_p), over the
//                                stacked camera-side rows W_p of the point's observations in pt_obs order.  (W and Sigma_s carry the
//                                same column scaling, inverse to each other: the product needs no unscaling.)
//   k_cov_dense / _pose / _intr  Sigma_c = D Sigma_s D (D: the columns' powers of two -- exact) and its diagonal blocks in the fixed
//                                6 x 6 / KPAD x KPAD layouts, zeros where constant.
#include <hip/hip_runtime.h>

#include <chrono>
#include <climits>

#include "pxr_ba_cov.h"
#include "pxr_ba_driver.h"

namespace pxr {

int chol_factor_solve(hipStream_t st, double* a, int n, int* d_info, double* linv_ws, double* x_out, bool zero_info);

namespace {

constexpr double kUnit = 1.1102230246251565e-16;     // u = 2^-53
constexpr int COV_G = 16;                              // lanes per point

__global__ __launch_bounds__(256) void k_cov_diag(int n, const double* __restrict__ S, int ld, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = S[(size_t)i * ld + i];
}

// first column whose pivot L_kk^2 is not above thresh * S_kk: dependent on the columns before it up to rounding.
// ldiag: the diagonal tiles' factors (column-major 64 x 64 each); first_bad starts at INT_MAX (an integer minimum: exact in any order)
__global__ __launch_bounds__(256) void k_cov_pivot_check(int n, const double* __restrict__ ldiag, const double* __restrict__ sdiag,
                                                         double thresh, int* __restrict__ first_bad) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const double l = ldiag[(size_t)(k >> 6) * 4096 + (k & 63) * 65];
  if (!(l * l > thresh * sdiag[k])) atomicMin(first_bad, k + 1);
}

// One point per 16-lane group.  Lane a owns the camera-side rows a, a + 16 of every observation (DC <= 18): for its row r of the
// stacked W_p it forms q_r = sum_s Sigma_s[col(r), col(s)] W_p[s, :] over ALL rows s of the track in pt_obs order, then adds
// W_p[r, :]^T q_r to its part of the 3 x 3 matrix M; the parts meet in a fixed butterfly; lane 0 finishes T + T M T and writes
// nine doubles (upper triangle computed, lower mirrored: symmetric bit for bit).
__global__ __launch_bounds__(256) void k_cov_points(const SolveDev d, const int64_t* __restrict__ pt_ptr, const int64_t* __restrict__ pt_obs,
                                                    const double* __restrict__ W, const double* __restrict__ T,
                                                    const int* __restrict__ singular, const double* __restrict__ sig /* n_c x n_c or NULL */,
                                                    double* __restrict__ out) {
  const int lane = threadIdx.x % COV_G;
  const int64_t p = (int64_t)blockIdx.x * (256 / COV_G) + threadIdx.x / COV_G;
  const bool live = p < d.v.n_points;
  const bool var = live && d.pt_var[p] != 0 && singular[p] == 0;
  double m00 = 0.0, m01 = 0.0, m02 = 0.0, m11 = 0.0, m12 = 0.0, m22 = 0.0;
  if (var && sig) {
    const int64_t o0 = pt_ptr[p], o1 = pt_ptr[p + 1];
    for (int64_t o = o0; o < o1; ++o) {
      const int64_t i = pt_obs[o];
      const int img = d.v.d_obs_image[i], cam = d.v.d_image_camera[img];
      const int dci = d.pose_dim[img] + d.intr_dim[cam];
      for (int a = lane; a < dci; a += COV_G) {
        const double* srow = sig + (size_t)col_index(d, img, cam, a) * d.n_c;
        double q0 = 0.0, q1 = 0.0, q2 = 0.0;
        for (int64_t o2 = o0; o2 < o1; ++o2) {
          const int64_t j = pt_obs[o2];
          const int imgj = d.v.d_obs_image[j], camj = d.v.d_image_camera[imgj];
          const int dcj = d.pose_dim[imgj] + d.intr_dim[camj];
          const double* Wj = W + (size_t)j * d.DC * 3;
          for (int b = 0; b < dcj; ++b) {
            const double s = srow[col_index(d, imgj, camj, b)];
            q0 += s * Wj[3 * b]; q1 += s * Wj[3 * b + 1]; q2 += s * Wj[3 * b + 2];
          }
        }
        const double* Wi = W + ((size_t)i * d.DC + a) * 3;
        m00 += Wi[0] * q0; m01 += Wi[0] * q1; m02 += Wi[0] * q2;
        m11 += Wi[1] * q1; m12 += Wi[1] * q2; m22 += Wi[2] * q2;
      }
    }
  }
#pragma unroll
  for (int off = COV_G / 2; off > 0; off >>= 1) {
    m00 += __shfl_xor(m00, off, COV_G); m01 += __shfl_xor(m01, off, COV_G); m02 += __shfl_xor(m02, off, COV_G);
    m11 += __shfl_xor(m11, off, COV_G); m12 += __shfl_xor(m12, off, COV_G); m22 += __shfl_xor(m22, off, COV_G);
  }
  if (!live || lane != 0) return;
  double* o = out + 9 * (size_t)p;
  if (!var) {
    const double v = (d.pt_var[p] != 0 && singular[p] != 0) ? __longlong_as_double(0x7ff8000000000000ll) : 0.0;
#pragma unroll
    for (int e = 0; e < 9; ++e) o[e] = v;
    return;
  }
  const double* Tp = T + 6 * (size_t)p;
  const double t00 = Tp[0], t01 = Tp[1], t02 = Tp[2], t11 = Tp[3], t12 = Tp[4], t22 = Tp[5];
  // N = M T (M symmetric), P = T + T N
  const double n00 = m00 * t00 + m01 * t01 + m02 * t02, n01 = m00 * t01 + m01 * t11 + m02 * t12, n02 = m00 * t02 + m01 * t12 + m02 * t22;
  const double n10 = m01 * t00 + m11 * t01 + m12 * t02, n11 = m01 * t01 + m11 * t11 + m12 * t12, n12 = m01 * t02 + m11 * t12 + m12 * t22;
  const double n20 = m02 * t00 + m12 * t01 + m22 * t02, n21 = m02 * t01 + m12 * t11 + m22 * t12, n22 = m02 * t02 + m12 * t12 + m22 * t22;
  const double p00 = t00 + (t00 * n00 + t01 * n10 + t02 * n20), p01 = t01 + (t00 * n01 + t01 * n11 + t02 * n21);
  const double p02 = t02 + (t00 * n02 + t01 * n12 + t02 * n22), p11 = t11 + (t01 * n01 + t11 * n11 + t12 * n21);
  const double p12 = t12 + (t01 * n02 + t11 * n12 + t12 * n22), p22 = t22 + (t02 * n02 + t12 * n12 + t22 * n22);
  o[0] = p00; o[1] = p01; o[2] = p02; o[3] = p01; o[4] = p11; o[5] = p12; o[6] = p02; o[7] = p12; o[8] = p22;
}

// Sigma_c = D Sigma_s D
__global__ __launch_bounds__(256) void k_cov_dense(int n, const double* __restrict__ sig, const double* __restrict__ scale, double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)n * n) return;
  const int r = (int)(e / n), c = (int)(e % n);
  out[e] = sig[e] * scale[r] * scale[c];
}

// slot of local pose column a in the fixed (rotation, tx, ty, tz) order: the variable tvec components keep their order
__device__ __forceinline__ int pose_slot(int a, int tmask) {
  if (a < 3) return a;
  int left = a - 3;
  for (int k = 0; k < 3; ++k) {
    if ((tmask >> k) & 1) continue;
    if (left == 0) return 3 + k;
    --left;
  }
  return -1;
}
__device__ __forceinline__ int intr_slot(int a, int cmask) {     // parameter index of the a-th variable intrinsic
  int left = a;
  for (int k = 0; k < PXR_KPAD; ++k) {
    if ((cmask >> k) & 1) continue;
    if (left == 0) return k;
    --left;
  }
  return -1;
}

// a thread per image: 36 zeros, then the pose block of Sigma_c where the pose is variable
__global__ __launch_bounds__(256) void k_cov_pose(const SolveDev d, const double* __restrict__ sig, double* __restrict__ out) {
  const int img = blockIdx.x * blockDim.x + threadIdx.x;
  if (img >= d.v.n_images) return;
  double* o = out + 36 * (size_t)img;
  for (int e = 0; e < 36; ++e) o[e] = 0.0;
  const int pd = d.pose_dim[img], po = d.pose_off[img], tm = d.tmask[img];
  for (int a = 0; a < pd; ++a)
    for (int b = 0; b < pd; ++b) {
      const int sa = pose_slot(a, tm), sb = pose_slot(b, tm);
      if (sa >= 0 && sb >= 0) o[sa * 6 + sb] = sig[(size_t)(po + a) * d.n_c + (po + b)] * d.scale_c[po + a] * d.scale_c[po + b];
    }
}
__global__ __launch_bounds__(256) void k_cov_intr(const SolveDev d, const double* __restrict__ sig, double* __restrict__ out) {
  const int cam = blockIdx.x * blockDim.x + threadIdx.x;
  if (cam >= d.v.n_cameras) return;
  double* o = out + (size_t)PXR_KPAD * PXR_KPAD * cam;
  for (int e = 0; e < PXR_KPAD * PXR_KPAD; ++e) o[e] = 0.0;
  const int id = d.intr_dim[cam], io = d.intr_off[cam], cm = d.cmask[cam];
  for (int a = 0; a < id; ++a)
    for (int b = 0; b < id; ++b) {
      const int sa = intr_slot(a, cm), sb = intr_slot(b, cm);
      if (sa >= 0 && sb >= 0) o[sa * PXR_KPAD + sb] = sig[(size_t)(io + a) * d.n_c + (io + b)] * d.scale_c[io + a] * d.scale_c[io + b];
    }
}

double ms_since(std::chrono::steady_clock::time_point& t) {
  const auto now = std::chrono::steady_clock::now();
  const double ms = std::chrono::duration<double, std::milli>(now - t).count();
  t = now;
  return ms;
}

}  // namespace
}  // namespace pxr

extern "C" int pxr_ba_covariance(pxr_ctx* ctx, const pxr_ba_view* view, const double* d_rec, const pxr_loss* loss,
                                 const uint8_t* h_pose_const, const uint8_t* h_tvec_const_mask, const uint16_t* h_cam_const_mask,
                                 const uint8_t* h_point_const, double* d_cov_cameras, double* d_cov_pose, double* d_cov_intrinsics,
                                 double* d_cov_points, pxr_cov_summary* summary) {
  using namespace pxr;
  PXR_REQUIRE(ctx && view && d_rec && loss && summary, "pxr_ba_covariance: NULL argument");
  PXR_REQUIRE(h_pose_const && h_tvec_const_mask && h_cam_const_mask && h_point_const, "pxr_ba_covariance: NULL parameterisation array");
  PXR_REQUIRE(view->n_obs > 0, "pxr_ba_covariance: problem has no residuals");
  PXR_REQUIRE(!(ctx->comm != nullptr && (ctx->nranks > 1 || ctx->force_collective)),
              "pxr_ba_covariance: not available with a communicator (several ranks)");
  PXR_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  summary->num_camera_unknowns = 0; summary->info = 0; summary->num_singular_points = 0;
  summary->ms_linearise = summary->ms_factor_inverse = summary->ms_points = 0.0;
  DevBuf<int> singular, first_bad;
  DevBuf<unsigned long long> n_singular;
  RC(singular.alloc((size_t)view->n_points)); RC(first_bad.alloc(1)); RC(n_singular.alloc(1));
  auto t = std::chrono::steady_clock::now();
  return ba_cov_system(ctx, view, d_rec, loss, h_pose_const, h_tvec_const_mask, h_cam_const_mask, h_point_const, singular.p, n_singular.p,
                       [&](const CovSystem& sys) -> int {
    const int n_c = sys.n_c;
    summary->num_camera_unknowns = n_c;
    PXR_REQUIRE((size_t)n_c <= spd_inverse_max_n(), "pxr_ba_covariance: %d camera-side columns exceed the direct solver's limit of %d", n_c,
                (int)spd_inverse_max_n());
    unsigned long long h_singular = 0;
    PXR_HIP(hipMemcpyAsync(&h_singular, n_singular.p, sizeof(h_singular), hipMemcpyDeviceToHost, st));
    PXR_HIP(hipStreamSynchronize(st));
    summary->num_singular_points = (int64_t)h_singular;
    summary->ms_linearise = ms_since(t);
    const double* sig = nullptr;
    if (n_c > 0) {
      // the diagonal of the scaled S, copied before the factorisation updates the tiles it lives in: what the pivots are held against
      DevBuf<double> sdiag;
      RC(sdiag.alloc((size_t)n_c));
      hipLaunchKernelGGL(k_cov_diag, blocks_for(n_c, 256), dim3(256), 0, st, n_c, (const double*)sys.aug, n_c + 1, sdiag.p);
      RC(chol_factor_solve(st, sys.aug, n_c, sys.d_info, sys.linv, sys.xsol, /*zero_info=*/true));
      const int N = (n_c + 63) / 64;
      int h_info[2] = {0, INT_MAX};
      PXR_HIP(hipMemcpyAsync(first_bad.p, &h_info[1], sizeof(int), hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(k_cov_pivot_check, blocks_for(n_c, 256), dim3(256), 0, st, n_c, (const double*)(sys.linv + (size_t)(N + 1) * 4096),
                         (const double*)sdiag.p, 64.0 * n_c * kUnit, first_bad.p);
      LAUNCH_CHECK("pivot check");
      PXR_HIP(hipMemcpyAsync(&h_info[0], sys.d_info, sizeof(int), hipMemcpyDeviceToHost, st));
      PXR_HIP(hipMemcpyAsync(&h_info[1], first_bad.p, sizeof(int), hipMemcpyDeviceToHost, st));
      PXR_HIP(hipStreamSynchronize(st));
      int info = h_info[0];
      if (h_info[1] != INT_MAX && (info == 0 || h_info[1] < info)) info = h_info[1];
      summary->info = info;
      if (info != 0) { summary->ms_factor_inverse = ms_since(t); return PXR_OK; }     // rank deficient: outputs unspecified
      RC(spd_inverse_from_factor(st, sys.aug, n_c, sys.scratch, sys.linv));
      PXR_HIP(hipStreamSynchronize(st));
      sig = sys.scratch;
      summary->ms_factor_inverse = ms_since(t);
    }
    if (d_cov_points) {
      const int64_t groups = view->n_points;
      hipLaunchKernelGGL(k_cov_points, blocks_for(groups * COV_G, 256), dim3(256), 0, st, sys.dv, sys.pt_ptr, sys.pt_obs, sys.W, sys.T,
                         (const int*)singular.p, sig, d_cov_points);
    }
    if (d_cov_pose) {
      if (n_c > 0) hipLaunchKernelGGL(k_cov_pose, blocks_for(view->n_images, 256), dim3(256), 0, st, sys.dv, sig, d_cov_pose);
      else PXR_HIP(hipMemsetAsync(d_cov_pose, 0, sizeof(double) * 36 * (size_t)view->n_images, st));
    }
    if (d_cov_intrinsics) {
      if (n_c > 0) hipLaunchKernelGGL(k_cov_intr, blocks_for(view->n_cameras, 256), dim3(256), 0, st, sys.dv, sig, d_cov_intrinsics);
      else PXR_HIP(hipMemsetAsync(d_cov_intrinsics, 0, sizeof(double) * PXR_KPAD * PXR_KPAD * (size_t)view->n_cameras, st));
    }
    if (d_cov_cameras && n_c > 0)
      hipLaunchKernelGGL(k_cov_dense, blocks_for((int64_t)n_c * n_c, 256), dim3(256), 0, st, n_c, sig, (const double*)sys.dv.scale_c, d_cov_cameras);
    LAUNCH_CHECK("covariance kernels");
    PXR_HIP(hipStreamSynchronize(st));
    summary->ms_points = ms_since(t);
    return PXR_OK;
  });
}
