// pxr_ba_solve.hip -- featuremetric bundle adjustment: Levenberg-Marquardt with Schur
// elimination of the point blocks, entirely on the GPU.
//
// Replaces BundleOptimizer::SolveProblem -> ceres::Solve
// (bundle_adjustment/src/bundle_optimizer.h:172-245) and the parameterisation of :335-453.
// [upstream Ceres 2.1] trust_region_minimizer.cc / levenberg_marquardt_strategy.cc semantics.
//
// Because every residual block's Jacobian factors as J = G P (G: C x 2 descriptor gradients,
// P: 2 x n projection Jacobian), the robustified normal equations of observation i are
//     J~^T J~ = P^T M~ P ,  J~^T r~ = P^T b~ ,   M~ = rho'(G^T G - kappa b b^T), b~ = rho' G^T r
// with the 2x2 / 2-vector (M~, b~) coming straight out of the fused record of pxr_ba_eval.
// The solver therefore never touches C-dimensional data: one pass of the HBM-bound residual
// kernel per LM iteration, everything else is per-observation 2 x (dc+3) algebra.
//
// Pipeline per linearisation (observations sorted by point for K1 locality):
//   K_jac     thread/obs    M~, b~, E = d(x,y)/dX (2x3), B = d(x,y)/d(pose,intr) tangent (2xdc) and
//             W_i = B^T M~ E (dc x 3); records assembled in LDS, written as coalesced streams
//   K_point   thread/point  V_p = sum E^T M~ E, g_p = sum E^T b~
//   K_img     block/(image,chunk)  U (pose/intrinsics blocks, upper) and g_c from LDS-staged records
// per LM attempt (radius changes on rejection, linearisation is reused):
//   K_pinv    thread/point  T_p = (V_p + D_p/radius)^-1
//   K_schur_lds  block/(image chunk, column tile)  S -= Y_i W_j^T over the point's observation pairs
//             (upper triangle only), rhs -= Y_i g_p, Y_i = W_i T_p formed on the fly; privatised in LDS
//   all-reduce(S | rhs) over ranks (RCCL, multi-GPU), + LM damping, blocked dense Cholesky (pxr_chol.hip)
//   K_backsub lane group/point  delta_p = -T_p (g_p + sum W_i^T delta_c)
//   K_update  x (+) delta (quaternion manifold, subset manifolds), then pxr_ba_eval at the
//             candidate WITH Jacobians (same HBM traffic as cost-only, saves the second
//             evaluation Ceres does after an accepted step).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <thread>
#include <vector>

#include "pxr_ba_cov.h"
#include "pxr_ba_driver.h"
#include "pxr_ba_pcg.h"

namespace pxr {


// ---- K_jac ------------------------------------------------------------------------------------
// The 216-B L record and the 192-B W block of an observation are assembled in LDS (one row per lane)
// and written out by the wavefront as contiguous, fully coalesced streams: per-lane stores of
// 27 + 24 scattered doubles left partially written lines to be evicted and re-merged in HBM.
constexpr int JAC_THREADS = 128;

__global__ __launch_bounds__(JAC_THREADS) void k_jac(const SolveDev d, const double* __restrict__ rec,
                                                     pxr_loss loss, double* __restrict__ L, double* __restrict__ W) {
  extern __shared__ double jstage[];            // per wavefront: [64][LS] then [64][WS]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int LS = d.LS, W3 = 3 * d.DC, WS = W3 + 1;
  double* Lw = jstage + (size_t)wave * 64 * (LS + WS);
  double* Ww = Lw + (size_t)64 * LS;
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + wave * 64;      // first observation of this wavefront
  const int64_t i = i0 + lane;
  const int n_valid = (int)min((int64_t)64, d.v.n_obs - i0);
  if (i < d.v.n_obs) {
  const int img = d.v.d_obs_image[i], pt = d.v.d_obs_point[i], cam = d.v.d_image_camera[img];
  double q[4], t[3], X[3], k[PXR_KPAD];
#pragma unroll
  for (int j = 0; j < 4; ++j) q[j] = d.v.d_qvec[4 * (size_t)img + j];
#pragma unroll
  for (int j = 0; j < 3; ++j) { t[j] = d.v.d_tvec[3 * (size_t)img + j]; X[j] = d.v.d_xyz[3 * (size_t)pt + j]; }
#pragma unroll
  for (int j = 0; j < PXR_KPAD; ++j) k[j] = d.v.d_cam_params[(size_t)cam * PXR_KPAD + j];
  const int model = d.v.d_cam_model[cam];
  double x, y, A[2][3], Pq[2][4], PX[2][3], Pk[2][PXR_KPAD];
  world_to_pixel_jac(model, k, q, t, X, x, y, A, Pq, PX, Pk);

  const double* r = rec + (size_t)i * PXR_OBS_REC;
  const double s = r[0], gxx = r[1], gxy = r[2], gyy = r[3], bx = r[4], by = r[5];
  double rho[3];
  loss_eval(loss.type, loss.a, 1.0, s, rho);
  // corrector [upstream Ceres corrector.cc]: J~^T J~ = rho'(J^T J - kappa (J^T r)(J^T r)^T)
  double kappa = 0.0;
  if (s != 0.0 && rho[2] > 0.0) {
    const double D = 1.0 + 2.0 * s * rho[2] / rho[1];
    const double alpha = 1.0 - sqrt(D);
    kappa = (2.0 * alpha - alpha * alpha) / s;
  }
  double* Lo = Lw + (size_t)lane * LS;
  const double m00 = rho[1] * (gxx - kappa * bx * bx), m01 = rho[1] * (gxy - kappa * bx * by),
               m11 = rho[1] * (gyy - kappa * by * by);
  Lo[0] = m00; Lo[1] = m01; Lo[2] = m11;
  Lo[3] = rho[1] * bx;
  Lo[4] = rho[1] * by;
  // E = d(x,y)/dX, scaled
  const bool pvar = d.pt_var[pt] != 0;
  double e0[3], e1[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double sc = pvar ? d.scale_p[3 * (size_t)pt + j] : 0.0;
    e0[j] = PX[0][j] * sc; e1[j] = PX[1][j] * sc;
    Lo[5 + j] = e0[j];
    Lo[8 + j] = e1[j];
  }
  // W = B^T M~ E (dc x 3) is fixed for the whole linearisation point (it does not depend on the
  // trust-region radius), so it is produced here once instead of once per LM attempt
  double me0[3], me1[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    me0[j] = m00 * e0[j] + m01 * e1[j];
    me1[j] = m01 * e0[j] + m11 * e1[j];
  }
  double* Wo = Ww + (size_t)lane * WS;
  // B: tangent pose columns then variable intrinsics columns
  double* B0 = Lo + 11;
  double* B1 = B0 + d.DC;
  int col = 0;
  auto put = [&](int c, double b0, double b1) {
    B0[c] = b0; B1[c] = b1;
    Wo[3 * c] = b0 * me0[0] + b1 * me1[0];
    Wo[3 * c + 1] = b0 * me0[1] + b1 * me1[1];
    Wo[3 * c + 2] = b0 * me0[2] + b1 * me1[2];
  };
  if (d.pose_dim[img] > 0) {
    const int po = d.pose_off[img];
    // QuaternionManifold::PlusJacobian [upstream Ceres manifold.cc], 4x3
    const double PJ[4][3] = {{-q[1], -q[2], -q[3]}, {q[0], q[3], -q[2]}, {-q[3], q[0], q[1]}, {q[2], -q[1], q[0]}};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double sc = d.scale_c[po + a];
      put(col, (Pq[0][0] * PJ[0][a] + Pq[0][1] * PJ[1][a] + Pq[0][2] * PJ[2][a] + Pq[0][3] * PJ[3][a]) * sc,
          (Pq[1][0] * PJ[0][a] + Pq[1][1] * PJ[1][a] + Pq[1][2] * PJ[2][a] + Pq[1][3] * PJ[3][a]) * sc);
      ++col;
    }
    const int tm = d.tmask[img];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if ((tm >> a) & 1) continue;
      const double sc = d.scale_c[po + col];
      put(col, A[0][a] * sc, A[1][a] * sc);
      ++col;
    }
  }
  if (d.intr_dim[cam] > 0) {
    const int io = d.intr_off[cam], cm = d.cmask[cam], K = camera_num_params(model);
    int kc = 0;
#pragma unroll
    for (int a = 0; a < PXR_KPAD; ++a) {
      if (a >= K || ((cm >> a) & 1)) continue;
      const double sc = d.scale_c[io + kc];
      put(col, Pk[0][a] * sc, Pk[1][a] * sc);
      ++col; ++kc;
    }
  }
  for (; col < d.DC; ++col) put(col, 0.0, 0.0);
  }
  __threadfence_block();                        // LDS rows of the other lanes of this wavefront
  __builtin_amdgcn_wave_barrier();
  if (n_valid <= 0) return;
  double* Lg = L + (size_t)i0 * LS;
  for (int x = lane; x < n_valid * LS; x += 64) Lg[x] = Lw[x];
  double* Wg = W + (size_t)i0 * W3;
  for (int x = lane; x < n_valid * W3; x += 64) { const int o = x / W3; Wg[x] = Ww[o * WS + (x - o * W3)]; }
}

// ---- K_point ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_point(const SolveDev d, const int64_t* __restrict__ pt_ptr,
                                               const int64_t* __restrict__ pt_obs,
                                               const double* __restrict__ L, double* __restrict__ V,
                                               double* __restrict__ gp) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= d.v.n_points) return;
  double v[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
  for (int64_t o = pt_ptr[p]; o < pt_ptr[p + 1]; ++o) {
    const double* Lo = L + (size_t)pt_obs[o] * d.LS;
    const double m00 = Lo[0], m01 = Lo[1], m11 = Lo[2], b0 = Lo[3], b1 = Lo[4];
    const double e0[3] = {Lo[5], Lo[6], Lo[7]}, e1[3] = {Lo[8], Lo[9], Lo[10]};
    double me0[3], me1[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) { me0[j] = m00 * e0[j] + m01 * e1[j]; me1[j] = m01 * e0[j] + m11 * e1[j]; }
    v[0] += e0[0] * me0[0] + e1[0] * me1[0];
    v[1] += e0[0] * me0[1] + e1[0] * me1[1];
    v[2] += e0[0] * me0[2] + e1[0] * me1[2];
    v[3] += e0[1] * me0[1] + e1[1] * me1[1];
    v[4] += e0[1] * me0[2] + e1[1] * me1[2];
    v[5] += e0[2] * me0[2] + e1[2] * me1[2];
#pragma unroll
    for (int j = 0; j < 3; ++j) g[j] += e0[j] * b0 + e1[j] * b1;
  }
#pragma unroll
  for (int j = 0; j < 6; ++j) V[6 * p + j] = v[j];
#pragma unroll
  for (int j = 0; j < 3; ++j) gp[3 * p + j] = g[j];
}

// ---- K_img: U and g_c --------------------------------------------------------------------------
constexpr int IMG_BATCH = 128;   // observations staged in LDS per pass

__global__ __launch_bounds__(256) void k_img(const SolveDev d, const ImgChunk* __restrict__ chunks,
                                             const int64_t* __restrict__ img_obs,
                                             const double* __restrict__ L, double* __restrict__ U,
                                             double* __restrict__ gc, int block_form, double det_scale,
                                             double* __restrict__ chunk_trace, double* __restrict__ kpart, int ne_max) {
  // kpart (deterministic mode of the iterative solver): the chunk's NE sums go to kpart[chunk][ne_max] instead of into U and g_c by
  // atomics; pcg_blocks_from_partials adds them per image and per column in a fixed order
  // block_form = 0: U is the dense n_c x n_c matrix (upper triangle), direct solver;
  // block_form = 1: U is [n_images][DC][DC], the image's full symmetric dc x dc block (iterative solver)
  extern __shared__ double stage[];            // [IMG_BATCH][LS] records, then [256] reduction slots
  const ImgChunk ch = chunks[blockIdx.x];
  const int img = ch.img, cam = d.v.d_image_camera[img];
  const int dc = d.pose_dim[img] + d.intr_dim[cam];
  if (dc == 0) { if (threadIdx.x == 0 && chunk_trace) chunk_trace[blockIdx.x] = 0.0; return; }
  const int LS = d.LS;
  double* red = stage + (size_t)IMG_BATCH * LS;
  const int NP = dc * (dc + 1) / 2, NE = NP + dc;
  const int slices = 256 / NE;                 // NE <= 189
  const int e = threadIdx.x % NE, sl = threadIdx.x / NE;
  int a = 0, b = 0;
  const bool is_g = e >= NP;
  if (is_g) { a = e - NP; }
  else { int rem = e; a = 0; while (rem >= dc - a) { rem -= dc - a; ++a; } b = a + rem; }
  double acc = 0.0;
  // deterministic mode: every OBSERVATION's term is rounded to the fixed-point grid on its own and the integers are added (`qacc`)
  // -- a chunk's double sum rounded once would depend on which observations share a chunk, i.e. on how the points are dealt
  // to ranks; `acc` (the plain double sum) then only feeds the trace check of the overflow guard (chunk_trace)
  long long qacc = 0;
  const bool fixed = det_scale != 0.0;
  // The records of an image's observations are gathered (216 B each at DC = 8) into LDS with
  // coalesced, independent loads -- consecutive lanes read consecutive doubles of a record -- and
  // every thread then accumulates its matrix entry from LDS.  (A per-thread gather loop over the
  // observations was bound by the latency of its dependent loads.)
  // (the next batch's records are requested into registers before the current batch is consumed: a load -> LDS -> accumulate
  // loop exposed the gather's latency once per batch)
  constexpr int IMG_PF = 16;                   // doubles per thread and batch: IMG_BATCH * LS <= 256 * IMG_PF (LS <= 32)
  double pf[IMG_PF];
  auto request = [&](int64_t base) {
    const int nb = (int)min((int64_t)IMG_BATCH, ch.end - base);
#pragma unroll
    for (int j = 0; j < IMG_PF; ++j) {
      const int x = threadIdx.x + 256 * j;
      const int xc = min(x, nb * LS - 1);
      const int o = xc / LS, f = xc - o * LS;
      pf[j] = L[(size_t)img_obs[base + o] * LS + f];
    }
  };
  if (LS <= 2 * IMG_PF) {
    if (ch.begin < ch.end) request(ch.begin);
    for (int64_t base = ch.begin; base < ch.end; base += IMG_BATCH) {
      const int nb = (int)min((int64_t)IMG_BATCH, ch.end - base);
#pragma unroll
      for (int j = 0; j < IMG_PF; ++j) { const int x = threadIdx.x + 256 * j; if (x < nb * LS) stage[x] = pf[j]; }
      __syncthreads();
      if (base + IMG_BATCH < ch.end) request(base + IMG_BATCH);
      if (sl < slices) {
        for (int o = sl; o < nb; o += slices) {
          const double* Lo = stage + (size_t)o * LS;
          const double* B0 = Lo + 11; const double* B1 = B0 + d.DC;
          const double term = is_g ? B0[a] * Lo[3] + B1[a] * Lo[4]
                                   : B0[a] * (Lo[0] * B0[b] + Lo[1] * B1[b]) + B1[a] * (Lo[1] * B0[b] + Lo[2] * B1[b]);
          acc += term;
          if (fixed) qacc += __double2ll_rn(term * det_scale);
        }
      }
      __syncthreads();
    }
  } else {
  for (int64_t base = ch.begin; base < ch.end; base += IMG_BATCH) {
    const int nb = (int)min((int64_t)IMG_BATCH, ch.end - base);
    for (int x = threadIdx.x; x < nb * LS; x += 256) {
      const int o = x / LS, f = x - o * LS;
      stage[x] = L[(size_t)img_obs[base + o] * LS + f];
    }
    __syncthreads();
    if (sl < slices) {
      for (int o = sl; o < nb; o += slices) {
        const double* Lo = stage + (size_t)o * LS;
        const double* B0 = Lo + 11; const double* B1 = B0 + d.DC;
        const double term = is_g ? B0[a] * Lo[3] + B1[a] * Lo[4]
                                 : B0[a] * (Lo[0] * B0[b] + Lo[1] * B1[b]) + B1[a] * (Lo[1] * B0[b] + Lo[2] * B1[b]);
        acc += term;
        if (fixed) qacc += __double2ll_rn(term * det_scale);
      }
    }
    __syncthreads();
  }
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  if (sl == 0) for (int s2 = 1; s2 < slices; ++s2) acc += red[s2 * NE + e];
  if (fixed) {                                   // the integers' turn through the same reduction slots
    __syncthreads();
    red[threadIdx.x] = __longlong_as_double(qacc);
    __syncthreads();
    if (sl == 0) for (int s2 = 1; s2 < slices; ++s2) qacc += __double_as_longlong(red[s2 * NE + e]);
    __syncthreads();
    // the chunk's trace(U) contribution, in plain doubles: only compared with a threshold (overflow guard of the solver)
    red[threadIdx.x] = (sl == 0 && !is_g && a == b) ? acc : 0.0;
    __syncthreads();
    if (threadIdx.x == 0 && chunk_trace) {
      double tr = 0.0;
      for (int x = 0; x < NP; ++x) tr += red[x];
      chunk_trace[blockIdx.x] = tr;
    }
  }
  if (sl == 0 && kpart) {
    kpart[(size_t)blockIdx.x * ne_max + e] = acc;
  } else if (sl == 0) {
    const int ra = col_index(d, img, cam, a);
    // (det_scale != 0: deterministic mode, order-independent fixed-point accumulation -- pxr_device.h)
    const double v = fixed ? __longlong_as_double(qacc) : acc;
    if (is_g) accum_flush(gc + ra, v, det_scale);
    else if (block_form) {
      double* Ub = U + (size_t)img * d.DC * d.DC;
      accum_flush(Ub + a * d.DC + b, v, det_scale);
      if (a != b) accum_flush(Ub + b * d.DC + a, v, det_scale);
    } else accum_flush(U + (size_t)ra * d.n_c + col_index(d, img, cam, b), v, det_scale);
  }
}

// ---- K_pinv: T_p = (V_p + D_p / radius)^-1 -----------------------------------------------------
__global__ __launch_bounds__(256) void k_pinv(int64_t n_points, const int* __restrict__ pt_var,
                                              const double* __restrict__ V,
                                              const double* __restrict__ Vdiag0 /* clamped diag */,
                                              double inv_radius, double* __restrict__ T,
                                              double* __restrict__ zero_ptr, int zero_n) {
  // side job of the attempt's first kernel: clear the attempt's scalars / limbs / info word (one fill launch less per attempt;
  // nothing before the Schur kernels of this attempt touches them)
  if (blockIdx.x == 0) for (int e = threadIdx.x; e < zero_n; e += blockDim.x) zero_ptr[e] = 0.0;
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_points) return;
  double* To = T + 6 * p;
  if (!pt_var[p]) { for (int j = 0; j < 6; ++j) To[j] = 0.0; return; }
  const double a00 = V[6 * p] + Vdiag0[3 * p] * inv_radius, a01 = V[6 * p + 1], a02 = V[6 * p + 2];
  const double a11 = V[6 * p + 3] + Vdiag0[3 * p + 1] * inv_radius, a12 = V[6 * p + 4];
  const double a22 = V[6 * p + 5] + Vdiag0[3 * p + 2] * inv_radius;
  const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
  const double det = a00 * c00 + a01 * c01 + a02 * c02;
  const double id = 1.0 / det;
  To[0] = c00 * id; To[1] = c01 * id; To[2] = c02 * id;
  To[3] = (a00 * a22 - a02 * a02) * id; To[4] = (a01 * a02 - a00 * a12) * id;
  To[5] = (a00 * a11 - a01 * a01) * id;
}

// ---- K_pinv_checked: T_p = V_p^-1 for the covariance (pxr_ba_cov.hip), by a 3 x 3 Cholesky that can say no -------------------------
// A pivot that is not above 64 u times its diagonal entry is not distinguishable from zero in a V_p summed in floating point: the
// point is SINGULAR (a point seen from one image, a track without parallax) -- flag 1, T_p = 0, so that the Schur kernels leave
// it out of S as they leave a constant point out.  No damping, no determinant formula: the inverse comes from the factor.
__global__ __launch_bounds__(256) void k_pinv_checked(int64_t n_points, const int* __restrict__ pt_var, const double* __restrict__ V,
                                                      double* __restrict__ T, int* __restrict__ singular, unsigned long long* __restrict__ n_singular) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_points) return;
  double* To = T + 6 * p;
  singular[p] = 0;
  if (!pt_var[p]) { for (int j = 0; j < 6; ++j) To[j] = 0.0; return; }
  const double tiny = 64.0 * 1.1102230246251565e-16;
  const double a00 = V[6 * p], a01 = V[6 * p + 1], a02 = V[6 * p + 2], a11 = V[6 * p + 3], a12 = V[6 * p + 4], a22 = V[6 * p + 5];
  bool ok = a00 > 0.0 && isfinite(a00);
  const double l00 = sqrt(ok ? a00 : 1.0);
  const double l10 = a01 / l00, l20 = a02 / l00;
  const double d1 = a11 - l10 * l10;
  ok = ok && d1 > tiny * a11;
  const double l11 = sqrt(ok ? d1 : 1.0);
  const double l21 = (a12 - l20 * l10) / l11;
  const double d2 = a22 - l20 * l20 - l21 * l21;
  ok = ok && d2 > tiny * a22;
  if (!ok) {
    for (int j = 0; j < 6; ++j) To[j] = 0.0;
    singular[p] = 1;
    atomicAdd(n_singular, 1ull);                   // (a count: exact in any order)
    return;
  }
  const double l22 = sqrt(d2);
  // M = inv(L) (lower), T = M^T M
  const double m00 = 1.0 / l00, m11 = 1.0 / l11, m22 = 1.0 / l22;
  const double m10 = -l10 * m00 * m11;
  const double m21 = -l21 * m11 * m22;
  const double m20 = -(l20 * m00 + l21 * m10) * m22;
  To[0] = m00 * m00 + m10 * m10 + m20 * m20; To[1] = m10 * m11 + m20 * m21; To[2] = m20 * m22;
  To[3] = m11 * m11 + m21 * m21; To[4] = m21 * m22;
  To[5] = m22 * m22;
}

// the accepted candidate becomes the current point: four arrays, ONE launch (four hipMemcpyAsync cost four dispatches)
struct Copy4 { const double* src[4]; double* dst[4]; int64_t n[4]; };
__global__ __launch_bounds__(256) void k_copy4(const Copy4 c) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
#pragma unroll
  for (int a = 0; a < 4; ++a)
    for (int64_t e = t0; e < c.n[a]; e += stride) c.dst[a][e] = c.src[a][e];
}

// ---- K_schur: S -= Y_i W_j^T (upper), rhs -= Y_i g_p ----------------------------------------------
__global__ __launch_bounds__(256) void k_schur(const SolveDev d, const int64_t* __restrict__ pt_ptr,
                                               const int64_t* __restrict__ pt_obs,
                                               const double* __restrict__ W, const double* __restrict__ T,
                                               const double* __restrict__ gp, double* __restrict__ S,
                                               double* __restrict__ rhs, double det_scale) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t i = tid / d.DC;
  const int a = (int)(tid - i * d.DC);
  if (i >= d.v.n_obs) return;
  const int img = d.v.d_obs_image[i], cam = d.v.d_image_camera[img];
  const int dci = d.pose_dim[img] + d.intr_dim[cam];
  if (a >= dci) return;
  const int pt = d.v.d_obs_point[i];
  if (!d.pt_var[pt]) return;
  double y0, y1, y2;
  y_row(W, T, i, a, d.DC, pt, y0, y1, y2);
  const int r = col_index(d, img, cam, a);
  accum_add(rhs + (size_t)r * d.ldS, -(y0 * gp[3 * (size_t)pt] + y1 * gp[3 * (size_t)pt + 1] + y2 * gp[3 * (size_t)pt + 2]), det_scale);
  for (int64_t o = pt_ptr[pt]; o < pt_ptr[pt + 1]; ++o) {
    const int64_t j = pt_obs[o];
    const int imgj = d.v.d_obs_image[j], camj = d.v.d_image_camera[imgj];
    const int dcj = d.pose_dim[imgj] + d.intr_dim[camj];
    const double* Wj = W + (size_t)j * d.DC * 3;
    for (int b = 0; b < dcj; ++b) {
      const int c = col_index(d, imgj, camj, b);
      if (r > c) continue;   // upper triangle only: the mirrored entry comes from the ordered pair (j, i)
      accum_add(S + (size_t)r * d.ldS + c, -(y0 * Wj[3 * b] + y1 * Wj[3 * b + 1] + y2 * Wj[3 * b + 2]), det_scale);
    }
  }
}

// ---- K_schur_lds: same contraction, privatised in LDS ------------------------------------------------
// A workgroup owns (image chunk, column tile): it accumulates the block row
//   S[rows of (pose(img), intr(cam)), c0 : c0 + CT]  -=  Y_i W_j^T
// in LDS with ds_add_f64 and flushes it once with global atomics.  The dense-S atomics drop
// from one per (i, j, a, b) contribution (~1.7e8 at 1M observations) to one per (chunk, row,
// column) (~2.5e6); the contraction itself runs at LDS-atomic speed.
template <int G>   // lanes per observation: G >= DC (8, 16 or 32)
__global__ __launch_bounds__(1024) void k_schur_lds(const SolveDev d, const ImgChunk* __restrict__ chunks,
                                                    const int4* __restrict__ so,      // per image-ordered slot: {obs, point, first partner, partners (0 = constant point)}
                                                    const int* __restrict__ pj,       // partner observation of each (point, k) slot
                                                    const int4* __restrict__ pcols,   // its {pose_off, pose_dim, intr_off, intr_dim}
                                                    const double* __restrict__ W, const double* __restrict__ T,
                                                    const double* __restrict__ gp, int CT,
                                                    double* __restrict__ S, double* __restrict__ rhs, double det_scale) {
  extern __shared__ double acc[];              // [DC][CT] then [DC] for the right-hand side
  const ImgChunk ch = chunks[blockIdx.x];
  const int img = ch.img, cam = d.v.d_image_camera[img];
  const int dci = d.pose_dim[img] + d.intr_dim[cam];
  if (dci == 0) return;
  const int c0 = blockIdx.y * CT, c1 = min(d.n_c, c0 + CT);
  double* racc = acc + (size_t)d.DC * CT;
  double* ybuf = racc + d.DC;                  // [blockDim.x][3]: the rows of Y_i, handed round the lane group through LDS
  for (int e = threadIdx.x; e < dci * CT + d.DC; e += blockDim.x) {
    if (e < dci * CT) acc[(e / CT) * CT + (e % CT)] = 0.0; else racc[e - dci * CT] = 0.0;
  }
  __syncthreads();
  // G lanes share one observation.  Lane a first forms row a of Y_i = W_i T_p; the dc_i x 3 rows are
  // handed round the group ONCE per observation (shuffles).  Then, per partner observation j of the
  // same point, lane b loads row b of W_j (one coalesced read of the whole dc_j x 3 block per group,
  // all partners of a batch in flight together) and adds its column of the block -Y_i W_j^T to the
  // LDS tile.  The host flattens obs -> point -> partner list -> column descriptors into three
  // levels of loads (so[], then pj / pcols / W_i / T / gp, then W_j).
  const int lane_b = threadIdx.x % G, grp = threadIdx.x / G, n_grp = blockDim.x / G;
  int rrow[G];                                             // global row of Y_i row a (same for every observation of the image)
#pragma unroll
  for (int a = 0; a < G; ++a) rrow[a] = a < dci ? col_index(d, img, cam, a) : 0x7fffffff;
  // The loads of an observation form a chain: slot descriptor -> (W_i, T_p, g_p, the partner list) -> the partners' rows.  As
  // first written every link waited for the one before it -- and W_i / T, g_p, the partner descriptors were three links of
  // their own: five dependent round trips per observation, eight observations per lane group, 80 % of the wave cycles
  // waiting (profiles/r4_hot_kernels_pmc.json).  Now: the next observation's descriptor is requested one iteration ahead,
  // everything it addresses goes out TOGETHER (unconditional loads at clamped indices, selected afterwards: a conditional
  // load is a branch + a wait), then the partners' rows: two links on the critical path.
  constexpr int PB = 8;                                    // partners per batch of loads in flight
  const bool first_tile = blockIdx.y == 0;
  int64_t o = ch.begin + grp;
  int4 s = o < ch.end ? so[o] : make_int4(0, 0, 0, 0);
  while (o < ch.end) {
    const int64_t o_next = o + n_grp;
    const int4 s_next = o_next < ch.end ? so[o_next] : make_int4(0, 0, 0, 0);
    if (s.w != 0) {                                        // (0: constant point; uniform over the group)
      const int64_t i = s.x, pt = s.y;
      const bool row_ok = lane_b < dci;
      // -- link 1: W_i row, T_p, g_p, partner observations and their column descriptors
      const double* Wi = W + ((size_t)i * d.DC + (row_ok ? lane_b : 0)) * 3;
      const double* Tp = T + 6 * (size_t)pt;
      const double* gpp = gp + 3 * (size_t)pt;
      const double w0 = Wi[0], w1 = Wi[1], w2 = Wi[2];
      const double t0 = Tp[0], t1 = Tp[1], t2 = Tp[2], t3 = Tp[3], t4 = Tp[4], t5 = Tp[5];
      const double g0 = gpp[0], g1 = gpp[1], g2 = gpp[2];
      double y0 = 0.0, y1 = 0.0, y2 = 0.0;
      // (one copy of the batch body: tracks of more than PB observations -- rare -- come round again with kb = PB, 2 PB, ...)
      for (int kb = 0; kb < s.w; kb += PB) {
        int jj[PB];
        int4 cc[PB];
#pragma unroll
        for (int u = 0; u < PB; ++u) {
          const int idx = s.z + min(kb + u, s.w - 1);
          jj[u] = pj[idx]; cc[u] = pcols[idx];
        }
        // -- link 2: row lane_b of every partner's W_j
        double mm[PB][3];
        int col[PB];                                        // global column of that row, or -1: not this lane's / outside the tile
#pragma unroll
        for (int u = 0; u < PB; ++u) {
          const int pdj = cc[u].y, dcj = pdj + cc[u].w;
          const bool has = kb + u < s.w && lane_b < dcj;
          const double* Wj = W + ((size_t)jj[u] * d.DC + (has ? lane_b : 0)) * 3;
          mm[u][0] = Wj[0]; mm[u][1] = Wj[1]; mm[u][2] = Wj[2];
          const int c = lane_b < pdj ? cc[u].x + lane_b : cc[u].z + (lane_b - pdj);
          col[u] = (has && c >= c0 && c < c1) ? c : -1;
        }
        if (kb == 0) {     // -- Y_i row (from link 1) and the right-hand side, while the partners' rows are on their way
          if (row_ok) { y0 = w0 * t0 + w1 * t1 + w2 * t2; y1 = w0 * t1 + w1 * t3 + w2 * t4; y2 = w0 * t2 + w1 * t4 + w2 * t5; }
          if (first_tile && row_ok) accum_add(racc + lane_b, -(y0 * g0 + y1 * g1 + y2 * g2), det_scale);
          // (a wavefront's LDS operations execute in order: the group's reads below see these writes, and the next
          // observation's writes come after this one's reads)
          double* yb = ybuf + 3 * (size_t)threadIdx.x;
          yb[0] = y0; yb[1] = y1; yb[2] = y2;
        }
        // row a of Y_i comes round the group through LDS (three broadcast reads: all lanes of the group read one address; as
        // 64-bit shuffles they were six ds_bpermute per row) and meets every partner's row: the 24 values of all rows at once
        // were 48 registers next to the 48 of the partners' rows
        const double* yg = ybuf + 3 * (size_t)(threadIdx.x - lane_b);
#pragma unroll
        for (int a = 0; a < G; ++a) {
          const double ya0 = yg[3 * a], ya1 = yg[3 * a + 1], ya2 = yg[3 * a + 2];
#pragma unroll
          for (int u = 0; u < PB; ++u) {
            const int c = col[u];
            if (c >= 0 && c >= rrow[a])                      // upper triangle (rrow = INT_MAX beyond dc_i)
              accum_add(acc + (size_t)a * CT + (c - c0), -(ya0 * mm[u][0] + ya1 * mm[u][1] + ya2 * mm[u][2]), det_scale);
          }
        }
      }
    }
    o = o_next; s = s_next;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < dci * CT; e += blockDim.x) {
    const int a = e / CT, cl = e % CT;
    const double v = acc[(size_t)a * CT + cl];
    if (__double_as_longlong(v) != 0ll) accum_flush(S + (size_t)col_index(d, img, cam, a) * d.ldS + (c0 + cl), v, det_scale);
  }
  if (blockIdx.y == 0 && threadIdx.x < dci) {
    const double v = racc[threadIdx.x];
    if (__double_as_longlong(v) != 0ll) accum_flush(rhs + (size_t)col_index(d, img, cam, threadIdx.x) * d.ldS, v, det_scale);
  }
}

// ---- small vector kernels --------------------------------------------------------------------------
// S is n x (n + 1) row-major (column n = right-hand side).  add_u = 1: S <- [upper(U) | 0];
// add_u = 0: S += diag(damp) / radius and rhs += gc (after the all-reduce).
__global__ void k_copy_upper_add_diag(int n, const double* __restrict__ U, const double* __restrict__ damp,
                                      double inv_radius, const double* __restrict__ gc, double* __restrict__ S,
                                      int add_u, double det_scale) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int ld = n + 1;
  if (t >= (int64_t)n * ld) return;
  const int r = (int)(t / ld), c = (int)(t % ld);
  double v = S[t];
  if (add_u) {
    // deterministic mode: U still holds its fixed-point integers (the same grid), the Schur kernel adds integers to these slots and
    // the second pass of this kernel (add_u = 0) turns the sums back -- AFTER the ranks' integers were added: a slot of 2^59 units does not survive a round
    // trip through a double (53 bits), and rounding every rank's partial sum would make the result depend on the partition
    v = (c < n && r <= c) ? U[(size_t)r * n + c] : 0.0;
  }
  else {
    if (det_scale != 0.0) v = (double)__double_as_longlong(v) / det_scale;    // (the slots' integers become doubles here: one pass)
    if (r == c) v += damp[r] * inv_radius;
    if (c == n) v += gc[r];
  }
  S[t] = v;
}

__global__ void k_extract_diag(int n, const double* __restrict__ U, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = U[(size_t)i * n + i];
}

__global__ void k_clamp(int64_t n, const double* __restrict__ in, double lo, double hi, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = fmin(fmax(in[i], lo), hi);
}

__global__ void k_point_diag(int64_t n_points, const double* __restrict__ V, double* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_points) return;
  out[3 * p] = V[6 * p]; out[3 * p + 1] = V[6 * p + 3]; out[3 * p + 2] = V[6 * p + 5];
}

__global__ void k_jacobi_scale(int64_t n, const double* __restrict__ diag, double* __restrict__ scale) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) scale[i] = 1.0 / (1.0 + sqrt(diag[i]));
}

// ---- deterministic direct solver: columns that stay small under Ceres' Jacobi scaling --------------------------------------------
// The fixed-point grid of a linearisation is ONE absolute step for every slot of U, g_c and S, made for the largest diagonal entry.
// Ceres' scaling 1 / (1 + sqrt d) leaves a column with d = |J_col|^2 << 1 as small as it was -- the r^6 coefficients of FULL_OPENCV
// have d ~ 1e-6 .. 1e-10 where a rotation has 1e6 --, so such a column (a) had its d measured by the unscaled pass to a few per cent
// only, hence a Jacobi scale and a damping that were not Ceres', and (b) kept 30 .. 40 significant bits in U and S where the
// others keep 60: a reduced system that is ill-conditioned in just those columns (k3 against k6) ended 1e-4 away from the
// floating-point solve.  The cure is a power of two 2^k per column on top of Ceres' scale: powers of two commute with every
// rounding of the floating-point path (the system becomes P S P, its Cholesky factor P L, the step keeps its bits), only the grid
// sees them.  pow_c = 4^k; the damping is Ceres': clamp(diag / 4^k) 4^k (k_clamp_pow).
//  * k_column_pow2, apply = 0: count the columns whose diagonal is below `below`;  apply = 1: move every column into [1/4, 1)
//    (scale, pow_c and -- the same linearisation point -- the damping follow).
//  * At the start (LmSolve::resolve_small_columns): only when the unscaled pass leaves a column with fewer than 2^16 grid steps
//    (d < 5e-4 on the first grid) the columns are moved and measured again; a scene without such a column -- the usual models,
//    whose focal lengths have d ~ 3e-3 .. 1 -- takes the path and the bits it always took (cols_pow2 stays false).
//  * k is NOT fixed for the solve the way Ceres' scale is: a column's norm may be small at the first point only (the FOV scene of
//    tests/test_camera_models_ext.py has one that grows by 1e5 with the first step), and left at its first k it would set the
//    grid of every later linearisation and take the bits from all the others.  The columns are moved again before every new
//    linearisation, from the diagonal of the last one, and after the overflow guard had to repeat one (LmSolve::move_columns).
__global__ void k_column_pow2(int64_t n, const double* __restrict__ diag, double below, int apply, double* __restrict__ scale,
                              double* __restrict__ pow_c, double* __restrict__ damp, double* __restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double v = diag[i];
  if (!(v > 0.0) || !isfinite(v)) return;        // (a column without a derivative stays as it is)
  if (!apply) { if (v < below) atomicAdd(count, 1.0); return; }      // (a sum of ones: exact in any order)
  int e;
  (void)frexp(v, &e);                            // v = m 2^e, m in [1/2, 1)
  const int dk = min(max((-e) >> 1, -300), 300); // e + 2 dk in {-1, 0}
  scale[i] = ldexp(scale[i], dk);
  pow_c[i] = ldexp(pow_c[i], 2 * dk);
  damp[i] = ldexp(damp[i], 2 * dk);
}

// Ceres' scale from d = diag / pow_c (the diagonal was measured with the columns moved by pow_c = 4^k), times the 2^k that brings the
// SCALED column's d / (1 + sqrt d)^2 into [1/4, 1) (k = 0 for d >= 1); pow_c = 4^k afterwards
__global__ void k_jacobi_scale_pow2(int64_t n, const double* __restrict__ diag, double* __restrict__ scale, double* __restrict__ pow_c) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double d = diag[i] / pow_c[i];
  const double s = 1.0 / (1.0 + sqrt(d));
  const double ds = d * s * s;
  int k = 0;
  if (ds > 0.0 && isfinite(ds)) {
    int e;
    (void)frexp(ds, &e);                         // ds = m 2^e, m in [1/2, 1)
    k = min(max((-e) >> 1, 0), 300);             // e + 2 k in {-1, 0}
  }
  scale[i] = ldexp(s, k);
  pow_c[i] = ldexp(1.0, 2 * k);
}

__global__ void k_clamp_pow(int64_t n, const double* __restrict__ in, const double* __restrict__ pow_c, double lo, double hi,
                            double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = fmin(fmax(in[i] / pow_c[i], lo), hi) * pow_c[i];
}

__global__ void k_axpy1(int n, const double* __restrict__ x, double* __restrict__ y) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] += x[i];
}

__global__ void k_fill(int64_t n, double v, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = v;
}

// delta_c = -x ; accumulates the replicated scalar SCAL_MODEL_CAM: d.D.d - d.g (camera side)
__global__ void k_finish_camera_step(int n, const double* __restrict__ x, const double* __restrict__ gc,
                                     const double* __restrict__ damp, double inv_radius,
                                     double* __restrict__ delta_c, double* __restrict__ scal_rep, long long* __restrict__ limb) {
  __shared__ long long lsh[PXR_LIMBS * 4];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double part = 0.0;
  if (i < n) {
    const double dl = -x[i];
    delta_c[i] = dl;
    part = dl * (damp[i] * inv_radius * dl - gc[i]);
  }
  if (limb) {                                    // deterministic mode: one limb addend per column (pxr_device.h)
    Limbs l;
    if (i < n) l.add(part);
    limbs_block_add(l, limb + SCAL_MODEL_CAM * PXR_LIMBS, lsh);
    return;
  }
  for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
  if ((threadIdx.x & 63) == 0) atomicAdd(scal_rep + (SCAL_MODEL_CAM - kScalRep), part);
}

// ---- K_backsub: delta_p = -T (g_p + sum_i W_i^T delta_c) ---------------------------------------------
// G lanes share one point (lane a = row a of every W_i: one coalesced 24 G-byte read per observation and group; a thread per
// point read its 24 doubles per observation at the stride of the whole track and waited on each -- 136 us at 1M observations
// against 45 us for the same layout in k_pt_u of the iterative solver).  Fixed butterfly over the group, lane 0 applies T_p.
constexpr int BACKSUB_PPG = 8;
template <int G>
__global__ __launch_bounds__(256) void k_backsub(const SolveDev d, const int64_t* __restrict__ pt_ptr,
                                                 const int* __restrict__ pj, const int4* __restrict__ pcols,
                                                 const double* __restrict__ W, const double* __restrict__ T,
                                                 const double* __restrict__ gp, const double* __restrict__ delta_c,
                                                 const double* __restrict__ Vdiag0, double inv_radius,
                                                 double* __restrict__ delta_p, double* __restrict__ scal_sum, long long* __restrict__ limb) {
  __shared__ double red[256 / 64];
  __shared__ long long lsh[PXR_LIMBS * 4];
  const int lane_a = threadIdx.x % G;
  double part = 0.0;
  Limbs lpart;                                   // deterministic mode: one limb addend per POINT
  // BACKSUB_PPG points per group and one atomic per workgroup: the model-cost scalar is ONE address, and an atomic per
  // wavefront of eight points (25 000 of them) serialised there for longer than the kernel's own work
  for (int rep = 0; rep < BACKSUB_PPG; ++rep) {
  const int64_t p = ((int64_t)blockIdx.x * BACKSUB_PPG + rep) * (256 / G) + threadIdx.x / G;
  const bool live = p < d.v.n_points;                  // whole groups are live or not
  const bool var = live && d.pt_var[p];
  double v0 = 0.0, v1 = 0.0, v2 = 0.0;
  if (var) {
    // four observations per trip: their descriptors first, then every W row and camera-step entry they address, at clamped
    // indices (one observation per trip was a chain of two dependent gathers per observation); the additions keep the track's order
    const int64_t o_end = pt_ptr[p + 1];
    for (int64_t o = pt_ptr[p]; o < o_end; o += 4) {
      int4 ci[4];                                        // {pose_off, pose_dim, intr_off, intr_dim} of the observation pj[.]
      int jj[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { const int64_t idx = min(o + u, o_end - 1); ci[u] = pcols[idx]; jj[u] = pj[idx]; }
      double w[4][3], dcv[4];
      bool ok[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        ok[u] = o + u < o_end && lane_a < ci[u].y + ci[u].w;
        const double* Wi = W + ((size_t)jj[u] * d.DC + (ok[u] ? lane_a : 0)) * 3;
        w[u][0] = Wi[0]; w[u][1] = Wi[1]; w[u][2] = Wi[2];
        dcv[u] = delta_c[ok[u] ? (lane_a < ci[u].y ? ci[u].x + lane_a : ci[u].z + (lane_a - ci[u].y)) : 0];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (ok[u]) { v0 += w[u][0] * dcv[u]; v1 += w[u][1] * dcv[u]; v2 += w[u][2] * dcv[u]; }
    }
  }
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) {
    v0 += __shfl_xor(v0, off); v1 += __shfl_xor(v1, off); v2 += __shfl_xor(v2, off);
  }
  if (live && lane_a == 0) {
    double dl[3] = {0, 0, 0};
    if (var) {
      v0 += gp[3 * p]; v1 += gp[3 * p + 1]; v2 += gp[3 * p + 2];
      const double* Tp = T + 6 * p;
      dl[0] = -(Tp[0] * v0 + Tp[1] * v1 + Tp[2] * v2);
      dl[1] = -(Tp[1] * v0 + Tp[3] * v1 + Tp[4] * v2);
      dl[2] = -(Tp[2] * v0 + Tp[4] * v1 + Tp[5] * v2);
      double pp = 0.0;
#pragma unroll
      for (int j = 0; j < 3; ++j) pp += dl[j] * (Vdiag0[3 * p + j] * inv_radius * dl[j] - gp[3 * p + j]);
      if (limb) lpart.add(pp); else part += pp;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) delta_p[3 * p + j] = dl[j];
  }
  }
  if (limb) { limbs_block_add(lpart, limb + SCAL_MODEL_PT * PXR_LIMBS, lsh); return; }
  part = wave_sum(part);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(scal_sum + SCAL_MODEL_PT, red[0] + red[1] + red[2] + red[3]);
}

// ---- K_update: candidate = x (+) scale * delta --------------------------------------------------------
struct ParamPtrs { double* q; double* t; double* k; double* X; };
constexpr int UPDATE_IPT = 4;

__global__ __launch_bounds__(256) void k_update(const SolveDev d, const double* __restrict__ delta_c,
                                                const double* __restrict__ delta_p, ParamPtrs out,
                                                double* __restrict__ scal_rep, double* __restrict__ scal_sum, long long* __restrict__ limb) {
  // UPDATE_IPT items per thread and one pair of atomics per workgroup: the four norms are four addresses, and an atomic per
  // wavefront (3 100 of them at 200 000 points) serialised there for most of the kernel's 82 us
  __shared__ double red[4][256 / 64];
  __shared__ long long lsh[PXR_LIMBS * 4];
  const int n_img = d.v.n_images, n_cam = d.v.n_cameras;
  double step2_rep = 0, x2_rep = 0, step2_sum = 0, x2_sum = 0;
  Limbs l_step_rep, l_x_rep, l_step_sum, l_x_sum;          // deterministic mode: one limb addend per image / camera / point
  for (int rep = 0; rep < UPDATE_IPT; ++rep) {
  const int64_t tid = ((int64_t)blockIdx.x * UPDATE_IPT + rep) * blockDim.x + threadIdx.x;
  if (tid < n_img) {
    const int i = (int)tid;
    double q0[4], t0[3], q1[4], t1[3];
    for (int j = 0; j < 4; ++j) q1[j] = q0[j] = d.v.d_qvec[4 * i + j];
    for (int j = 0; j < 3; ++j) t1[j] = t0[j] = d.v.d_tvec[3 * i + j];
    if (d.pose_dim[i] > 0) {
      const int po = d.pose_off[i];
      const double dd[3] = {delta_c[po] * d.scale_c[po], delta_c[po + 1] * d.scale_c[po + 1],
                            delta_c[po + 2] * d.scale_c[po + 2]};
      const double nd = sqrt(dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2]);
      if (nd != 0.0) {   // QuaternionManifold::Plus [upstream Ceres manifold.cc]
        const double sn = sin(nd) / nd;
        const double qd[4] = {cos(nd), sn * dd[0], sn * dd[1], sn * dd[2]};
        q1[0] = qd[0] * q0[0] - qd[1] * q0[1] - qd[2] * q0[2] - qd[3] * q0[3];
        q1[1] = qd[0] * q0[1] + qd[1] * q0[0] + qd[2] * q0[3] - qd[3] * q0[2];
        q1[2] = qd[0] * q0[2] - qd[1] * q0[3] + qd[2] * q0[0] + qd[3] * q0[1];
        q1[3] = qd[0] * q0[3] + qd[1] * q0[2] - qd[2] * q0[1] + qd[3] * q0[0];
      }
      int col = 3;
      for (int a = 0; a < 3; ++a) {
        if ((d.tmask[i] >> a) & 1) continue;
        t1[a] = t0[a] + delta_c[po + col] * d.scale_c[po + col];
        ++col;
      }
      double ix = 0.0, is = 0.0;
      for (int j = 0; j < 4; ++j) { ix += q0[j] * q0[j]; is += (q1[j] - q0[j]) * (q1[j] - q0[j]); }
      for (int j = 0; j < 3; ++j) { ix += t0[j] * t0[j]; is += (t1[j] - t0[j]) * (t1[j] - t0[j]); }
      if (limb) { l_x_rep.add(ix); l_step_rep.add(is); } else { x2_rep += ix; step2_rep += is; }
    }
    for (int j = 0; j < 4; ++j) out.q[4 * i + j] = q1[j];
    for (int j = 0; j < 3; ++j) out.t[3 * i + j] = t1[j];
  } else if (tid < n_img + n_cam) {
    const int c = (int)(tid - n_img);
    const int K = camera_num_params(d.v.d_cam_model[c]);
    int kc = 0;
    double ix = 0.0, is = 0.0;
    for (int a = 0; a < PXR_KPAD; ++a) {
      const double k0 = d.v.d_cam_params[(size_t)c * PXR_KPAD + a];
      double k1 = k0;
      if (d.intr_dim[c] > 0 && a < K) {
        if (!((d.cmask[c] >> a) & 1)) {
          const int io = d.intr_off[c] + kc;
          k1 = k0 + delta_c[io] * d.scale_c[io];
          ++kc;
        }
        ix += k0 * k0; is += (k1 - k0) * (k1 - k0);
      }
      out.k[(size_t)c * PXR_KPAD + a] = k1;
    }
    if (limb) { l_x_rep.add(ix); l_step_rep.add(is); } else { x2_rep += ix; step2_rep += is; }
  } else if (tid < n_img + n_cam + d.v.n_points) {
    const int64_t p = tid - n_img - n_cam;
    double ix = 0.0, is = 0.0;
    for (int j = 0; j < 3; ++j) {
      const double x0 = d.v.d_xyz[3 * p + j];
      double x1 = x0;
      if (d.pt_var[p]) {
        x1 = x0 + delta_p[3 * p + j] * d.scale_p[3 * p + j];
        ix += x0 * x0; is += (x1 - x0) * (x1 - x0);
      }
      out.X[3 * p + j] = x1;
    }
    if (limb) { l_x_sum.add(ix); l_step_sum.add(is); } else { x2_sum += ix; step2_sum += is; }
  }
  }
  if (limb) {
    limbs_block_add(l_step_rep, limb + SCAL_STEP2_CAM * PXR_LIMBS, lsh); __syncthreads();
    limbs_block_add(l_x_rep, limb + SCAL_X2_CAM * PXR_LIMBS, lsh); __syncthreads();
    limbs_block_add(l_step_sum, limb + SCAL_STEP2_PT * PXR_LIMBS, lsh); __syncthreads();
    limbs_block_add(l_x_sum, limb + SCAL_X2_PT * PXR_LIMBS, lsh);
    return;
  }
  step2_rep = wave_sum(step2_rep); x2_rep = wave_sum(x2_rep);
  step2_sum = wave_sum(step2_sum); x2_sum = wave_sum(x2_sum);
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    red[0][w] = step2_rep; red[1][w] = x2_rep; red[2][w] = step2_sum; red[3][w] = x2_sum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double r[4];
    for (int k = 0; k < 4; ++k) r[k] = red[k][0] + red[k][1] + red[k][2] + red[k][3];
    if (r[0] != 0.0 || r[1] != 0.0) { atomicAdd(scal_rep + (SCAL_STEP2_CAM - kScalRep), r[0]); atomicAdd(scal_rep + (SCAL_X2_CAM - kScalRep), r[1]); }
    if (r[2] != 0.0 || r[3] != 0.0) { atomicAdd(scal_sum + SCAL_STEP2_PT, r[2]); atomicAdd(scal_sum + SCAL_X2_PT, r[3]); }
  }
}

__global__ void k_point_step_norm(int64_t n_points, const int* __restrict__ pt_var, const double* __restrict__ X0,
                                  const double* __restrict__ X1, double* __restrict__ out, long long* __restrict__ limb_slot) {
  __shared__ long long lsh[PXR_LIMBS * 4];
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double s = 0.0;
  if (p < n_points && pt_var[p])
    for (int j = 0; j < 3; ++j) { const double d = X1[3 * p + j] - X0[3 * p + j]; s += d * d; }
  if (limb_slot) { Limbs l; l.add(s); limbs_block_add(l, limb_slot, lsh); return; }   // deterministic mode
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0 && s != 0.0) atomicAdd(out, s);
}

__global__ void k_normalize_q(int n, double* __restrict__ q) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double nn = sqrt(q[4 * i] * q[4 * i] + q[4 * i + 1] * q[4 * i + 1] + q[4 * i + 2] * q[4 * i + 2] + q[4 * i + 3] * q[4 * i + 3]);
  for (int j = 0; j < 4; ++j) q[4 * i + j] /= nn;   // colmap::Image::NormalizeQvec, bundle_optimizer.h:255
}

// gradient_tolerance test [upstream: max |g_i| <= tolerance, g in the unscaled variables]: the NUMBER of entries
// above the tolerance is accumulated instead of the maximum, because a count can be summed over the ranks with the
// all-reduce(sum) the solver already has (the point gradient is sharded; a rank-local maximum would let the ranks
// disagree about termination).
__global__ void k_count_above(int64_t n, const double* __restrict__ g, const double* __restrict__ scale, double tol,
                              double* __restrict__ out, long long* __restrict__ limb_slot) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double v = (i < n && !(fabs(g[i] / scale[i]) <= tol)) ? 1.0 : 0.0;
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0 && v != 0.0) {
    if (limb_slot) atomicAdd(reinterpret_cast<unsigned long long*>(limb_slot + 1), (unsigned long long)((long long)v << 20));   // digit on the 2^-20 grid
    else atomicAdd(out, v);
  }
}

// Several ranks: only the upper triangle of [S | rhs] carries data (row r: columns r .. n, the last one the right-hand side --
// one contiguous run of n - r + 1 doubles), so the collective moves the packed n (n + 3) / 2 doubles instead of the n (n + 1)
// of the square (10.2 MB instead of 20.3 MB at 200 cameras).  One workgroup per row, coalesced both ways.
__device__ __forceinline__ int64_t packed_row_offset(int n, int r) { return (int64_t)r * (n + 1) - (int64_t)r * (r - 1) / 2; }
__global__ __launch_bounds__(256) void k_pack_upper(int n, const double* __restrict__ S, double* __restrict__ packed) {
  const int r = blockIdx.x, len = n - r + 1;
  const double* src = S + (size_t)r * (n + 1) + r;
  double* dst = packed + packed_row_offset(n, r);
  for (int x = threadIdx.x; x < len; x += blockDim.x) dst[x] = src[x];
}
__global__ __launch_bounds__(256) void k_unpack_upper(int n, const double* __restrict__ packed, double* __restrict__ S) {
  const int r = blockIdx.x, len = n - r + 1;
  double* dst = S + (size_t)r * (n + 1) + r;
  const double* src = packed + packed_row_offset(n, r);
  for (int x = threadIdx.x; x < len; x += blockDim.x) dst[x] = src[x];
}

// cost = sum 0.5 rho(s) over the records as limbs (pxr_device.h): one addend per observation, integer atomics per workgroup --
// the same integers whatever the launch shape or the rank count.  (The cost fused into the residual kernel was one
// floating-point atomic per wavefront on one address: 50 us of serialisation at 1M observations.)
__global__ __launch_bounds__(256) void k_cost_limbs(const double* __restrict__ rec, int64_t n, pxr_loss loss, long long* __restrict__ slot) {
  __shared__ long long lsh[PXR_LIMBS * 4];
  Limbs l;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    double rho[3];
    loss_eval(loss.type, loss.a, 1.0, rec[i * PXR_OBS_REC], rho);
    l.add(0.5 * rho[0]);
  }
  limbs_block_add(l, slot, lsh);
}
// x[0 .. n) added to a limb slot, one addend per entry (the inner iterations' per-point costs)
__global__ __launch_bounds__(256) void k_limb_accumulate(const double* __restrict__ x, int64_t n, long long* __restrict__ slot) {
  __shared__ long long lsh[PXR_LIMBS * 4];
  Limbs l;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) l.add(x[i]);
  limbs_block_add(l, slot, lsh);
}
// scal[i] = value of limb slot i for every i in `mask`
__global__ void k_limbs_finish(const long long* __restrict__ limb, unsigned mask, double* __restrict__ scal) {
  const int i = threadIdx.x;
  if (i < kScalSlots && ((mask >> i) & 1u)) scal[i] = limb_value(limb + i * PXR_LIMBS);
}
// deterministic linearisation, before the ranks' sum: diag(U) (raw fixed-point slots) next to g_c, and the chunks' trace
// contributions as limbs behind them -- ONE workgroup (n_c is a few thousand at most)
__global__ __launch_bounds__(1024) void k_diag_and_trace(int n, const double* __restrict__ U, double* __restrict__ diag,
                                                          const double* __restrict__ chunk_trace, int n_chunks, long long* __restrict__ trace_out) {
  __shared__ double sh[1024];
  for (int i = threadIdx.x; i < n; i += 1024) diag[i] = U[(size_t)i * n + i];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n_chunks; i += 1024) acc += chunk_trace[i];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int off = 512; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    Limbs l; l.add(sh[0]);
    for (int k = 0; k < PXR_LIMBS; ++k) trace_out[k] = l.q[k];
  }
}
// ... and after it: the slots of diag(U) | g_c become doubles, and the overflow guard's statistics of the diagonal
__global__ __launch_bounds__(1024) void k_finish_and_stats(int n, int n_slots, double* __restrict__ gcd, double det_scale,
                                                            const long long* __restrict__ trace_limbs, double* __restrict__ out4) {
  __shared__ double smax[1024], ssum[1024], smin[1024];
  double mx = 0.0, sm = 0.0, mn = 0.0;
  for (int i = threadIdx.x; i < n_slots; i += 1024) {
    const double v = accum_value(gcd[i], det_scale);
    gcd[i] = v;
    if (i < n) { mx = fmax(mx, v); mn = fmin(mn, v); sm += v; }
  }
  smax[threadIdx.x] = mx; ssum[threadIdx.x] = sm; smin[threadIdx.x] = mn;
  __syncthreads();
  for (int off = 512; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) {
      smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + off]);
      smin[threadIdx.x] = fmin(smin[threadIdx.x], smin[threadIdx.x + off]);
      ssum[threadIdx.x] += ssum[threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out4[0] = smax[0]; out4[1] = ssum[0]; out4[2] = smin[0]; out4[3] = limb_value(trace_limbs); }
}
// 64-bit integers through a sum-of-doubles collective (the caller's all-reduce callback): each integer as its signed high and
// unsigned low 32-bit halves -- sums of up to 2^20 of them are exact in a double -- and back (modulo 2^64, like the integers)
__global__ void k_i64_split(int64_t n, const long long* __restrict__ in, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long long v = in[i];
  out[2 * i] = (double)(int)(v >> 32);
  out[2 * i + 1] = (double)(unsigned)(v & 0xffffffffll);
}
__global__ void k_i64_join(int64_t n, const double* __restrict__ in, long long* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned long long hi = (unsigned long long)(long long)in[2 * i], lo = (unsigned long long)(long long)in[2 * i + 1];
  out[i] = (long long)((hi << 32) + lo);
}

// keep rank 0's copy of a replicated buffer: the other ranks zero theirs before an all-reduce(sum)
__global__ void k_zero(int64_t n, double* __restrict__ x) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) x[i] = 0.0;
}

// ---- host orchestration -----------------------------------------------------------------------------------
// The ~60 work buffers of a solve come out of ONE grow-only allocation of the context (round 6): the first solve of a size takes
// them from hipMalloc and records what it needed, the next ones bump a pointer -- ~60 hipMalloc at the start and ~60 hipFree at the
// end (each a device synchronisation) were 4 ms of a 24 ms call at 1M observations (profiles/r6_lm_setup.txt).  The arena of the
// solve that is running on this thread; NULL outside pxr_ba_solve and with PXR_BA_ARENA=0.
struct SolveArena { char* base = nullptr; size_t cap = 0, used = 0, wanted = 0; };
static thread_local SolveArena* g_solve_arena = nullptr;
void* solve_scratch(size_t bytes, bool* owned) {
  const size_t b = ((bytes ? bytes : 1) + 255) & ~(size_t)255;
  if (SolveArena* a = g_solve_arena) {
    a->wanted += b;
    if (a->used + b <= a->cap) { void* p = a->base + a->used; a->used += b; *owned = false; return p; }
  }
  void* p = nullptr;
  *owned = true;
  if (hipMalloc(&p, b) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  return p;
}
// (constructed before every buffer of the solve and destroyed after all of them -- then the arena grows to what this solve asked for)
struct ArenaScope {
  pxr_ctx* ctx; SolveArena a; bool on;
  ArenaScope(pxr_ctx* c, bool enabled) : ctx(c), on(enabled) {
    a.base = static_cast<char*>(c->d_solve_arena); a.cap = c->solve_arena_bytes;
    if (on) g_solve_arena = &a;
  }
  ArenaScope(const ArenaScope&) = delete;
  ~ArenaScope() {
    g_solve_arena = nullptr;
    if (!on || a.wanted <= a.cap) return;
    (void)hipDeviceSynchronize();                         // (an error return may leave kernels of this solve in flight)
    if (ctx->d_solve_arena) (void)hipFree(ctx->d_solve_arena);
    ctx->d_solve_arena = nullptr; ctx->solve_arena_bytes = 0;
    const size_t want = a.wanted + a.wanted / 16 + (1u << 20);
    if (hipMalloc(&ctx->d_solve_arena, want) == hipSuccess) ctx->solve_arena_bytes = want;
    else { (void)hipGetLastError(); ctx->d_solve_arena = nullptr; }     // no room to keep it: the next solve allocates per buffer again
  }
};

SolveKnobs::SolveKnobs() {
  const char* e = std::getenv("PXR_BA_ARENA");
  arena = !(e && e[0] == '0');
  setup_host = std::getenv("PXR_BA_SETUP_HOST") != nullptr;
  verbose = std::getenv("PXR_VERBOSE") != nullptr;
  spin_wait = std::getenv("PXR_BLOCKING_WAIT") == nullptr;
  inner_packed = std::getenv("PXR_INNER_PACKED") != nullptr;
  inner_no_cache = std::getenv("PXR_INNER_NO_CACHE") != nullptr;
  inner_no_prebuild = std::getenv("PXR_INNER_NO_PREBUILD") != nullptr;
  schur_lds = std::getenv("PXR_SCHUR_GLOBAL_ATOMICS") == nullptr;
  phase_timing = std::getenv("PXR_PHASE_TIMING") != nullptr;   // adds a stream sync per phase
}

// pxr_chol.hip: factor the n x n SPD system stored row-major (upper) in the n x (n + 1) buffer `a` whose last
// column is the right-hand side (forward substitution is fused into the factorisation), then back-substitute.
int chol_factor_solve(hipStream_t st, double* a, int n, int* d_info, double* linv_ws, double* x_out, bool zero_info = true);
size_t chol_workspace_doubles(int n);
size_t inner_wave_stage_bytes(int64_t n_pts);        // pxr_ba_inner.hip: host room for the packed table of n_pts points, worst case

// pxr_ba_inner.hip
int launch_inner_iterations(pxr_ctx* ctx, pxr_arena* arena, const pxr_ba_view* view, const pxr_interp_cfg* cfg,
                            const pxr_loss* loss, const int64_t* d_pt_ptr, const int64_t* d_pt_obs,
                            const int* d_pt_var, double* d_cost_before, const InnerLists* lists, double* d_cost_per_point,
                            const GramCache* gram, bool gram_warm, bool prebuild);
int make_inner_lists(pxr_ctx* ctx, const int64_t* h_pt_ptr, int64_t n_pts, void* h_wave_stage, size_t wave_stage_bytes, const pxr_ba_view* view, const int64_t* d_pt_ptr, const int64_t* d_pt_obs,
                     InnerLists* out);
void free_inner_lists(InnerLists* l);

// the lane-group width of the Schur contraction and of the back-substitution: the smallest of 8, 16, 32 that holds DC rows
using SchurLdsKernel = decltype(&k_schur_lds<8>);
using BacksubKernel = decltype(&k_backsub<8>);
static SchurLdsKernel schur_lds_kernel(int DC) { return DC <= 8 ? k_schur_lds<8> : (DC <= 16 ? k_schur_lds<16> : k_schur_lds<32>); }
static BacksubKernel backsub_kernel(int DC) { return DC <= 8 ? k_backsub<8> : (DC <= 16 ? k_backsub<16> : k_backsub<32>); }
static int lane_group(int DC) { return DC <= 8 ? 8 : (DC <= 16 ? 16 : 32); }

// ---- deterministic mode (the default; pxr_set_deterministic(ctx, 0) / PXR_DETERMINISTIC=0 opt out) -------------------------
// Everything that is summed over observations, points or ranks is summed as INTEGERS, so that the result does not depend on
// the order of the adders, on the launch shapes or on how the points are dealt to ranks: an N-rank solve is bit-identical
// to the one-rank solve.
//  * matrix / vector slots (U, g_c, S | rhs): fixed point on ONE grid per linearisation, lin_scale = 2^k.  Integer atomics wrap
//    modulo 2^64, so only the FINAL content of a slot has to fit: |U_ij|, |S_ij| <= max diag(U) (U and the damped S are positive
//    semi-definite, S <= U) and |g_c|, |rhs| <= sqrt(max diag(U) 2 cost) (Cauchy-Schwarz; rho concave: rho' s <= rho).  The grid
//    of a linearisation comes from the measured max diag(U) of the previous one with a factor 8 of slack (the first,
//    Jacobi-scaled one: diag < 1 by construction), and every linearisation is CHECKED (lin_fits below): the finished
//    diagonal against the bound, and against the trace the chunks measured in floating point -- a diagonal slot that wrapped
//    is off by a multiple of 2^64 / scale.  A failed check repeats the linearisation on a grid from the measured trace.
//  * scalars (cost, model cost change, norms): four 40-bit limbs + a bad-addend count per scalar (pxr_device.h), one addend per
//    observation / point / column.
//  * several ranks: the integers are all-reduced as integers (ncclInt64; through a sum-of-doubles callback as exact 32-bit
//    halves), replicated quantities are computed identically by every rank and need no broadcast.
// (The grids need the Jacobi scaling of the options -- Ceres' and pixsfm's default: without it the large columns of the
//  unscaled Jacobian, rotations ~1e6, set a grid that drowns the small ones, focal length ~1e-2.  A solve that turns the
//  scaling off uses floating-point atomics; the iterative solver has its own form of the mode, det_iter.)
//
// det_iter: The iterative solver (> 1000 images) in deterministic mode: ORDERED PARTIAL SUMS instead of fixed point -- every chunk of an
// image leaves its part in a buffer and the parts are added per image / per column in a fixed order (k_img's kpart, pxr_ba_pcg.hip);
// the conjugate-gradient vectors span too many orders of magnitude for one grid.  Same bits on every run for a given number of
// ranks (the ranks' parts are all-reduced as doubles: the result depends on how the points are dealt to ranks, not on the run).
//
// bcast: Replicated quantities (camera step, replicated scalars) are computed by every rank from identical inputs, but
// with floating-point atomics whose order differs from rank to rank.  To keep the ranks bit-identical -- same
// parameters, same accept / reject / terminate decisions, hence the same sequence of collectives -- rank 0's copy
// is broadcast: the others zero theirs and join an all-reduce(sum).  Needs the rank (pxr_comm_init / _set_rank).
// (Only without the deterministic mode: with it every rank computes the same bits.)
// which of the solver's variants a call runs
struct SolveMode {
  bool geom;        // the geometric problem (records from geom_eval, inner iterations from k_inner_geom)
  bool iterative;   // conjugate gradients on the implicit Schur complement instead of the dense Cholesky
  bool multi;       // collectives run: the caller's callback, or the context's communicator with several (or forced: one) ranks
  bool native_i64;  // integer collectives through RCCL (else: the callback, as exact 32-bit halves)
  bool det_fixed;   // deterministic: fixed-point matrices (direct solver)
  bool det_iter;    // deterministic: ordered partial sums (iterative solver)
  bool det;         // either: scalars as integer limbs, no rank-0 broadcasts
  bool bcast;       // rank 0's copy of replicated quantities is broadcast
};

// ---- the device buffers of a solve (behind the structure's) ----------------------------------------------------------------------
struct SolveWorkspace {
  DevBuf<double> L, V, gp, Vd0, T, W, U, S /* S | rhs */, gcd /* diagU | g_c | trace limbs of the overflow guard */, damp_c, scale_c, pow_c /* resolve_small_columns */, scale_p,
      delta_c, delta_p, rec_a, rec_b, q1, t1, k1, X1, scal /* the scalar block, pxr_ba_solve.h */, xsol, linv;
  // iterative solver: preconditioner blocks and the conjugate-gradient work space
  PrecondBlocks precond;              // (host; alive while its uploads may be in flight)
  DevBuf<IntPair> col_group; DevBuf<int> group_size, group_cols;
  DevBuf<double> pcg_u, pcg_mloc, pcg_g, pcg_vec, pcg_scal;
  // deterministic mode of the iterative solver: where an image's chunks start (both chunkings), the (image, local column) entries of
  // every reduced-system column in ascending image order, and the buffers of the chunks' partial sums
  DevBuf<int> kchunk_ptr, schunk_ptr, col_ent_ptr;
  DevBuf<IntPair> col_ent;
  DevBuf<double> det_kpart, det_gimg, det_wpart, det_mpart;
  int det_ne_max = 0;
  DevBuf<double> cb_flags;            // iteration callbacks on several ranks: the ranks' answers, summed
  DevBuf<double> S_packed;            // several ranks, direct solver: the collective's buffer (upper triangle + rhs)
  int64_t packed_doubles = 0;
  DevBuf<double> i64_halves;          // several ranks through the callback: the integers' exact 32-bit halves
  DevBuf<double> det_part;            // the inner iterations' per-point costs (every mode)
  DevBuf<double> chunk_trace;
  DevBuf<double> col_count;           // k_column_pow2's answer

  int allocate(pxr_ctx* ctx, const pxr_ba_view* view, const SolveStructure& sx, const SolveMode& m) {
    hipStream_t st = ctx->stream;
    const int64_t n_obs = view->n_obs, n_pts = view->n_points;
    const int n_img = view->n_images, n_cam = view->n_cameras, n_c = sx.layout.n_c, DC = sx.layout.DC;
    const size_t nc1 = n_c ? n_c : 1;
    RC(L.alloc((size_t)n_obs * sx.layout.LS)); RC(V.alloc((size_t)n_pts * 6)); RC(gp.alloc((size_t)n_pts * 3));
    RC(Vd0.alloc((size_t)n_pts * 3)); RC(T.alloc((size_t)n_pts * 6));
    RC(W.alloc((size_t)n_obs * DC * 3));
    // S: n_c x (n_c + 1) [S | rhs] + one spare row for the factorisation
    // direct solver: dense U and [S | rhs]; iterative solver: one DC x DC block of U per image, nothing quadratic in n_c
    RC(U.alloc(m.iterative ? (size_t)n_img * DC * DC : nc1 * nc1)); RC(S.alloc(m.iterative ? 1 : (nc1 + 1) * (nc1 + 1)));
    RC(gcd.alloc(2 * nc1 + 8)); RC(damp_c.alloc(nc1));
    RC(scale_c.alloc(nc1)); RC(pow_c.alloc(nc1)); RC(scale_p.alloc((size_t)n_pts * 3)); RC(delta_c.alloc(nc1)); RC(delta_p.alloc((size_t)n_pts * 3));
    RC(rec_a.alloc((size_t)n_obs * PXR_OBS_REC)); RC(rec_b.alloc((size_t)n_obs * PXR_OBS_REC));
    RC(q1.alloc((size_t)n_img * 4)); RC(t1.alloc((size_t)n_img * 3)); RC(k1.alloc((size_t)n_cam * PXR_KPAD)); RC(X1.alloc((size_t)n_pts * 3));
    RC(scal.alloc(kScalAll));
    RC(xsol.alloc(nc1)); RC(linv.alloc(m.iterative ? 1 : chol_workspace_doubles(n_c)));
    if (m.iterative) {
      RC(col_group.upload(precond.col_group, st)); RC(group_size.upload(precond.group_size, st)); RC(group_cols.upload(precond.group_cols, st));
      RC(pcg_u.alloc((size_t)n_pts * 3)); RC(pcg_mloc.alloc((size_t)n_img * DC * DC));
      RC(pcg_g.alloc(precond.group_size.size() * PCG_GS * PCG_GS)); RC(pcg_vec.alloc(5 * nc1));
      RC(pcg_scal.alloc(16 + 8 * ((nc1 + 255) / 256)));   // 8 scalars + the loop's control block + the dot-product partials
    }
    det_ne_max = DC * (DC + 1) / 2 + DC;
    if (m.det_iter) {
      const std::vector<int> kptr = first_chunks(sx.chunks, n_img), sptr = first_chunks(sx.schur_chunks, n_img);       // (alive until the synchronisation below)
      RC(kchunk_ptr.upload(kptr, st)); RC(schunk_ptr.upload(sptr, st));
      ColumnEntries ce;
      column_entries(sx.layout, sx.image_camera.data(), &ce);
      RC(col_ent_ptr.upload(ce.ent_ptr, st)); RC(col_ent.upload(ce.ent, st));
      RC(det_kpart.alloc(std::max<size_t>(1, sx.chunks.size()) * det_ne_max)); RC(det_gimg.alloc((size_t)n_img * DC));
      RC(det_wpart.alloc(std::max<size_t>(1, sx.schur_chunks.size()) * DC)); RC(det_mpart.alloc(std::max<size_t>(1, sx.schur_chunks.size()) * DC * DC));
      PXR_HIP(hipMemsetAsync(det_kpart.p, 0, sizeof(double) * det_kpart.n, st));
      PXR_HIP(hipMemsetAsync(det_wpart.p, 0, sizeof(double) * det_wpart.n, st));
      PXR_HIP(hipMemsetAsync(det_mpart.p, 0, sizeof(double) * det_mpart.n, st));
      PXR_HIP(hipStreamSynchronize(st));        // (the host vectors above leave scope)
    }
    RC(cb_flags.alloc(2));
    packed_doubles = (int64_t)n_c * (n_c + 3) / 2;
    if (m.multi && !m.iterative && n_c > 0) RC(S_packed.alloc((size_t)packed_doubles));
    if (m.det && m.multi && !m.native_i64)
      RC(i64_halves.alloc((size_t)2 * std::max<int64_t>({packed_doubles, 2 * (int64_t)nc1 + 8, kScalSlots * PXR_LIMBS})));
    RC(det_part.alloc((size_t)n_pts + 8));
    RC(chunk_trace.alloc(sx.chunks.size() + 1));
    RC(col_count.alloc(1));
    return PXR_OK;
  }
};

// the grid of the deterministic mode's fixed-point slots: entries bounded by 8 max(md, sqrt(2 md cost)) fit 62 bits (md: the bound on
// diag(U) the grid is made for).  (A grid of 2^51 units with a one-addition rounding was tried: it saves nothing measurable -- the
// Schur kernel waits on its gathers -- and the 11 lost bits broke the parity of ill-conditioned reduced systems with the oracle.
// What the mode costs: `lm.nondeterministic` in profiles/r5_bench_n1.json, 2.37 against 2.45 ms per iteration.)
static double det_scale_for(double md, double cost_now) {
  const double bound = 8.0 * std::max({md, std::sqrt(2.0 * md * std::max(cost_now, 0.0)), 1e-300});
  return std::ldexp(1.0, 62 - (int)std::ceil(std::log2(bound)));
}

// ---- one solve: the LM loop of pxr_ba_solve and pxr_ba_solve_geometric ----------------------------------------------------------
// d_obs_xy != NULL: the geometric problem -- the records come from geom_eval and the inner iterations from k_inner_geom
// (pxr_ba_geom.hip), `arena` and `cfg` are not read, the Gram-matrix cache and the Gram-matrix inner kernel are off.  Everything
// else is the same code for both.
struct LmSolve {
  // the call
  pxr_ctx* ctx; pxr_arena* arena; const pxr_ba_view* view; const pxr_interp_cfg* cfg; const double* d_obs_xy; const pxr_loss* loss;
  const uint8_t* h_pose_const; const uint8_t* h_tvec_const_mask; const uint16_t* h_cam_const_mask; const uint8_t* h_point_const;
  const pxr_lm_options* opt; pxr_allreduce_fn allreduce; void* ar_user; pxr_lm_summary* sum;
  SolveKnobs knobs;
  hipStream_t st;
  SetupClock clock;
  std::chrono::steady_clock::time_point t_loop0;
  // sizes
  int64_t n_obs, n_pts; int n_img, n_cam;
  int n_c = 0, DC = 1, LS = 13, ldS = 1; size_t nc1 = 1;
  // stages
  SolveMode m;
  SolveStructure sx;
  SolveWorkspace ws;
  SolveDev dv;                          // the problem at the current parameters ...
  pxr_ba_view cand_view;                // ... and the candidate's parameters
  PcgArgs pcg;
  // views into the scalar block and its pinned host copy
  double* scal_sum = nullptr; double* scal_rep = nullptr; long long* slimb = nullptr; long long* limb_arg = nullptr;   // limb_arg: what the step kernels get, NULL = floating-point atomics into `scal`
  int* d_info = nullptr; double* lin_stats = nullptr;
  double* h_scal = nullptr; double* h_lin_stats = nullptr; const int* h_info_word = nullptr;
  double* rhs = nullptr; double* diagU = nullptr; double* gc = nullptr;
  double *cur_q = nullptr, *cur_t = nullptr, *cur_k = nullptr, *cur_X = nullptr;
  // evaluation
  bool gram_cache = false, gram_inner = false, inner_cache = false;
  bool geom_ext = false;                // geometric problem with a camera model beyond OPENCV: k_inner_geom<true>
  bool gram_warm = false;               // the cache holds every observation's matrices (after the first evaluation / inner call)
  int n_evaluations = 0;
  // The initial point is evaluated by the exact-order kernel, candidates from the cache: until a step is accepted the
  // current and the candidate cost come from two evaluations that differ by the rounding of the reference's fp32 pass (~1e-9
  // relative).  A solve that starts AT an optimum would decide its first steps on that difference: after the first rejected
  // step the current point is evaluated again, from the cache (its cells are mostly the candidate's: cheap), so that cost
  // changes compare like with like.
  bool cur_is_exact = true;
  GramCache gram;
  struct InnerListsOwner { InnerLists l; ~InnerListsOwner() { free_inner_lists(&l); } } inner_lists;
  // launch shape of the LDS-privatised Schur contraction
  int CT = 1, n_ctiles = 1; size_t schur_shmem = 0;
  // linearisation (deterministic mode)
  double lin_scale = 0.0;               // the fixed-point grid of U and g_c, 0: floating point
  double lin_md = 1.0;                  // the diag(U) bound the CURRENT grid was made for
  bool lin_not_finite = false;          // set by linearize_checked: the Jacobian at the current point is not finite
  // trust region
  double* rec_cur = nullptr; double* rec_cand = nullptr;
  double cost = 0.0, radius = 0.0, decrease_factor = 2.0;
  int invalid = 0;
  bool reuse_diag = false, inner_enabled = false, inner_useful = false;
  bool any_cb = false;
  double ph_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::chrono::steady_clock::time_point ph_t0;

  struct Candidate { bool ok = true; double cost = 0, model_cost_change = 0, step_norm = 0, x_norm = 0; bool repeat = false; };

  int setup();
  int run();

  int ar(double* buf, int64_t count);
  int ar_i64(long long* buf, int64_t count);
  int from_rank0(double* buf, int64_t count);
  int zero_scalars();
  int read_scalars(double* h16);
  int evaluate(const pxr_ba_view& v, double* rec);
  int linearize(const double* rec);
  bool lin_fits(const double* stt, double md_made_for) const;
  int linearize_checked(const double* rec, double md_guess, double cost_now, bool refine = false);
  int refresh_damping();
  int resolve_small_columns(const double* rec);
  int move_columns();
  bool cols_pow2 = false;
  int gradient_below_tolerance(bool* below);
  int reduced_system_direct(double inv_radius);
  int reduced_step_direct(double inv_radius);
  int reduced_step_iterative(double inv_radius, bool* ok, double* inexact_correction);
  int candidate(double inv_radius, double inexact_correction, Candidate* c);
  int reevaluate_current();
  int notify(int iteration, bool valid, bool successful, double cost_now, double change, double rel, double radius_next, double step);
  bool user_stop(int rc);
  int finish(int termination);                              // leaves final_radius alone
  int finish(int termination, double final_radius);
  void phase(int k);
  // the covariance (pxr_ba_cov.hip): the caller brings the records -- nothing is evaluated, no parameter is touched
  bool records_only = false;
  int covariance_system(const double* rec, int* singular, unsigned long long* n_singular, CovSystem* out);
};

// the collective: the caller's callback if given, else the context's RCCL communicator (pxr_comm_init)
int LmSolve::ar(double* buf, int64_t count) {
  if (allreduce) {
    if (allreduce(ar_user, buf, count) != 0) return set_error(PXR_EHIP, "pxr_ba_solve: all-reduce callback failed");
    return PXR_OK;
  }
  return comm_allreduce_sum(ctx, buf, count);
}
int LmSolve::from_rank0(double* buf, int64_t count) {
  if (!m.bcast) return PXR_OK;
  if (ctx->rank != 0) hipLaunchKernelGGL(k_zero, blocks_for(count, 256), dim3(256), 0, st, count, buf);
  return ar(buf, count);
}
int LmSolve::ar_i64(long long* buf, int64_t count) {    // in-place integer all-reduce(sum)
  if (!m.multi || count <= 0) return PXR_OK;
  if (m.native_i64) return comm_allreduce_sum_i64(ctx, buf, count);
  hipLaunchKernelGGL(k_i64_split, blocks_for(count, 256), dim3(256), 0, st, count, (const long long*)buf, ws.i64_halves.p);
  RC(ar(ws.i64_halves.p, 2 * count));
  hipLaunchKernelGGL(k_i64_join, blocks_for(count, 256), dim3(256), 0, st, count, (const double*)ws.i64_halves.p, buf);
  return PXR_OK;
}
int LmSolve::zero_scalars() {
  PXR_HIP(hipMemsetAsync(ws.scal.p, 0, sizeof(double) * kScalZeroed, st));   // scalars, limbs, the info word (the statistics behind them stay)
  return PXR_OK;
}
int LmSolve::read_scalars(double* h16) {
  if (m.det) {
    RC(ar_i64(slimb, kScalRep * PXR_LIMBS));
    hipLaunchKernelGGL(k_limbs_finish, dim3(1), dim3(64), 0, st, (const long long*)slimb, 0xffffu, ws.scal.p);
  } else {
    hipLaunchKernelGGL(k_limbs_finish, dim3(1), dim3(64), 0, st, (const long long*)slimb, (1u << SCAL_COST) | (1u << SCAL_COST_BEFORE_INNER), ws.scal.p);   // the costs
    RC(ar(scal_sum, kScalRep));
    RC(from_rank0(scal_rep, kScalSlots - kScalRep));
  }
  PXR_HIP(hipMemcpyAsync(h_scal, ws.scal.p, sizeof(double) * kScalAll, hipMemcpyDeviceToHost, st));     // the scalars ... the statistics: one copy of 800 bytes
  // the one host synchronisation of an LM attempt: polled (the blocking wait of hipStreamSynchronize sleeps on an interrupt and
  // wakes tens of microseconds late -- once per attempt, with the GPU idle meanwhile); PXR_BLOCKING_WAIT=1 restores it
  if (knobs.spin_wait) {
    PXR_HIP(hipEventRecord(ctx->ev_sync, st));
    hipError_t q;
    while ((q = hipEventQuery(ctx->ev_sync)) == hipErrorNotReady) {}
    PXR_HIP(q);
  } else PXR_HIP(hipStreamSynchronize(st));
  std::memcpy(h16, h_scal, sizeof(double) * kScalSlots);
  return PXR_OK;
}
int LmSolve::evaluate(const pxr_ba_view& v, double* rec) {   // rec + cost into the limbs of SCAL_COST
  // (the evaluation at the INITIAL point takes the exact-order kernel also with the cache on: the first trust-region step is
  // usually the largest of the solve -- at configs[2] 95 % of the projections leave their cell -- so matrices built there
  // would be built again at once, and 1.5 ms of builds cost more than 0.8 ms of texels)
  if (m.geom) RC(geom_eval(ctx, &v, d_obs_xy, rec, nullptr));
  else if (gram_cache && n_evaluations > 0) { RC(gram_evaluate(ctx, arena, &v, cfg, gram, rec)); gram_warm = true; }
  else RC(ba_eval_with_cost(ctx, arena, &v, cfg, 1, rec, nullptr, nullptr, nullptr, nullptr, nullptr));
  ++n_evaluations;
  hipLaunchKernelGGL(k_cost_limbs, dim3(1024), dim3(256), 0, st, (const double*)rec, n_obs, *loss, slimb + SCAL_COST * PXR_LIMBS);
  LAUNCH_CHECK("cost");
  return PXR_OK;
}
// linearise at the CURRENT parameters from record buffer `rec` (lin_scale: the fixed-point grid of U and g_c in
// deterministic mode, 0 otherwise)
int LmSolve::linearize(const double* rec) {
  hipLaunchKernelGGL(k_jac, dim3((unsigned)((n_obs + JAC_THREADS - 1) / JAC_THREADS)), dim3(JAC_THREADS),
                     sizeof(double) * (JAC_THREADS / 64) * 64 * (LS + 3 * DC + 1), st, dv, rec, *loss, ws.L.p, ws.W.p);
  hipLaunchKernelGGL(k_point, blocks_for(n_pts, 256), dim3(256), 0, st, dv, sx.d_pt_ptr.p, sx.d_pt_obs.p, ws.L.p, ws.V.p, ws.gp.p);
  PXR_HIP(hipMemsetAsync(ws.U.p, 0, sizeof(double) * ws.U.n, st));
  PXR_HIP(hipMemsetAsync(ws.gcd.p, 0, sizeof(double) * ws.gcd.n, st));
  if (n_c > 0 && !sx.chunks.empty()) {
    hipLaunchKernelGGL(k_img, dim3((unsigned)sx.chunks.size()), dim3(256), sizeof(double) * ((size_t)IMG_BATCH * LS + 256), st, dv,
                       sx.d_chunks.p, sx.d_img_obs.p, ws.L.p, ws.U.p, gc, m.iterative ? 1 : 0, lin_scale, lin_scale != 0.0 ? ws.chunk_trace.p : (double*)nullptr,
                       m.det_iter ? ws.det_kpart.p : (double*)nullptr, ws.det_ne_max);
    if (m.det_iter) {      // U blocks, diag(U) and g_c as ordered sums of the chunks' parts
      RC(pcg_blocks_from_partials(st, dv, ws.kchunk_ptr.p, ws.det_kpart.p, ws.det_ne_max, ws.U.p, ws.det_gimg.p, ws.col_ent_ptr.p, as_int2(ws.col_ent.p), diagU, gc));
      LAUNCH_CHECK("linearize kernels");
      RC(ar(ws.gcd.p, 2 * (int64_t)nc1));
      return PXR_OK;
    }
    if (lin_scale != 0.0) {
      // the integers of diag(U) and g_c (+ the trace) are summed over the ranks, THEN everything becomes doubles again
      hipLaunchKernelGGL(k_diag_and_trace, dim3(1), dim3(1024), 0, st, n_c, (const double*)ws.U.p, diagU, (const double*)ws.chunk_trace.p, (int)sx.chunks.size(),
                         reinterpret_cast<long long*>(ws.gcd.p + 2 * nc1));
      RC(ar_i64(reinterpret_cast<long long*>(ws.gcd.p), 2 * (int64_t)nc1 + PXR_LIMBS));
      // (U itself stays in fixed point: only the Schur complement reads it, as integers)
      hipLaunchKernelGGL(k_finish_and_stats, dim3(1), dim3(1024), 0, st, n_c, 2 * (int)nc1, ws.gcd.p, lin_scale,
                         reinterpret_cast<const long long*>(ws.gcd.p + 2 * nc1), lin_stats);
      LAUNCH_CHECK("linearize kernels");
      return PXR_OK;
    }
    if (m.iterative) RC(pcg_diag_from_blocks(st, dv, ws.U.p, diagU));
    else hipLaunchKernelGGL(k_extract_diag, blocks_for(n_c, 256), dim3(256), 0, st, n_c, ws.U.p, diagU);
  }
  LAUNCH_CHECK("linearize kernels");
  RC(ar(ws.gcd.p, 2 * (int64_t)nc1));   // global diag(U) and g_c
  return PXR_OK;
}
// the overflow guard: did every slot of the newest linearisation fit its grid?  (stats: lin_stats, read with the scalars or here)
bool LmSolve::lin_fits(const double* stt, double md_made_for) const {
  if (n_c == 0 || sx.chunks.empty()) return true;
  const double mx = stt[0], sm = stt[1], mn = stt[2], tr = stt[3];
  if (!(std::isfinite(mx) && std::isfinite(sm) && std::isfinite(tr))) return false;
  if (mn < 0.0) return false;                                               // a diagonal slot wrapped into the sign bit
  if (std::fabs(tr - sm) > std::ldexp(1.0, 61) / lin_scale) return false;   // ... or all the way round
  return mx <= 8.0 * md_made_for;                                           // the off-diagonal, Schur and gradient bounds hold
}
// linearise on a grid made for diag(U) <= 8 md_guess; repeat on a grid from the measured trace until the check passes
// (synchronises: used for the first two linearisations of a solve and on the -- never yet observed -- failure path)
int LmSolve::linearize_checked(const double* rec, double md_guess, double cost_now, bool refine) {
  if (!m.det_fixed) return linearize(rec);
  for (int attempt = 0; attempt < 8; ++attempt) {
    lin_md = md_guess;
    lin_scale = det_scale_for(lin_md, cost_now);
    RC(linearize(rec));
    PXR_HIP(hipMemcpyAsync(h_lin_stats, lin_stats, sizeof(double) * 4, hipMemcpyDeviceToHost, st));
    PXR_HIP(hipStreamSynchronize(st));
    if (lin_fits(h_lin_stats, lin_md)) {
      // `refine`: this linearisation is SOLVED with (no Jacobi scaling follows) -- a guess far above the measured diagonal
      // wasted resolution, once more on a grid made for the measurement
      if (refine && attempt == 0 && h_lin_stats[0] * 64.0 < md_guess) { md_guess = std::max(h_lin_stats[0], 1e-300); continue; }
      return PXR_OK;
    }
    // the trace was measured in floating point and bounds every diagonal entry.  NaN / Inf: the Jacobian itself is not finite --
    // [upstream] "Residual and Jacobian evaluation failed": the solve TERMINATES with FAILURE at the last accepted point, it is
    // not an error of the call (this used to return PXR_EINVAL)
    if (!(std::isfinite(h_lin_stats[3]) && h_lin_stats[3] >= 0.0)) { lin_not_finite = true; return PXR_OK; }
    md_guess = std::max(h_lin_stats[3], 2.0 * md_guess);
  }
  return set_error(PXR_EINVAL, "pxr_ba_solve: the fixed-point grid of the deterministic mode could not be fitted");
}
// deterministic direct solver, before the Jacobi scaling: diag(U) of the unscaled pass is in diagU.  If a column's entry is fewer
// than 2^16 steps of the grid it was measured on, every column is moved into [1/4, 1) by a power of two (scale_c, pow_c = its
// square) and the diagonal is measured again on the grid of that range -- and once more if a column that the first grid could not
// see at all shows up in the second.  cols_pow2: it happened (from then on the columns are kept there: move_columns)
// every column into [1/4, 1) by the diagonal of the newest linearisation (diagU); a linearisation must follow
int LmSolve::move_columns() {
  hipLaunchKernelGGL(k_column_pow2, blocks_for(n_c, 256), dim3(256), 0, st, (int64_t)n_c, (const double*)diagU, 0.0, 1, ws.scale_c.p, ws.pow_c.p, ws.damp_c.p,
                     ws.col_count.p);
  LAUNCH_CHECK("k_column_pow2");
  return PXR_OK;
}
int LmSolve::resolve_small_columns(const double* rec) {
  cols_pow2 = false;
  for (int pass = 0; pass < 4; ++pass) {
    double h = 0.0;
    PXR_HIP(hipMemsetAsync(ws.col_count.p, 0, sizeof(double), st));
    hipLaunchKernelGGL(k_column_pow2, blocks_for(n_c, 256), dim3(256), 0, st, (int64_t)n_c, (const double*)diagU, 65536.0 / lin_scale, 0,
                       ws.scale_c.p, ws.pow_c.p, ws.damp_c.p, ws.col_count.p);
    PXR_HIP(hipMemcpyAsync(&h, ws.col_count.p, sizeof(double), hipMemcpyDeviceToHost, st));
    PXR_HIP(hipStreamSynchronize(st));
    if (knobs.verbose) {
      std::vector<double> hd((size_t)n_c);
      PXR_HIP(hipMemcpy(hd.data(), diagU, sizeof(double) * n_c, hipMemcpyDeviceToHost));
      double mn = 1e300, mx = 0.0;
      for (double v : hd) if (v > 0.0) { mn = std::min(mn, v); mx = std::max(mx, v); }
      fprintf(stderr, "[pxr_ba_solve] pass %d: diag(U) in [%.3e, %.3e], grid step %.3e\n", pass, mn, mx, 1.0 / lin_scale);
    }
    if (h == 0.0) return PXR_OK;
    if (knobs.verbose) fprintf(stderr, "[pxr_ba_solve] %d columns of fewer than 2^16 grid steps: diag(U) measured again on their grid\n", (int)h);
    cols_pow2 = true;
    RC(move_columns());
    RC(linearize_checked(rec, 1.0 / 8.0, cost));
    if (lin_not_finite) return PXR_OK;
  }
  return PXR_OK;
}
int LmSolve::refresh_damping() {  // LevenbergMarquardtStrategy: diagonal clamped to [min, max]
  if (n_c > 0) hipLaunchKernelGGL(k_clamp_pow, blocks_for(n_c, 256), dim3(256), 0, st, (int64_t)n_c, diagU, ws.pow_c.p, opt->min_lm_diagonal, opt->max_lm_diagonal, ws.damp_c.p);
  hipLaunchKernelGGL(k_point_diag, blocks_for(n_pts, 256), dim3(256), 0, st, n_pts, ws.V.p, ws.Vd0.p);
  hipLaunchKernelGGL(k_clamp, blocks_for(n_pts * 3, 256), dim3(256), 0, st, n_pts * 3, ws.Vd0.p, opt->min_lm_diagonal, opt->max_lm_diagonal, ws.Vd0.p);
  LAUNCH_CHECK("damping kernels");
  return PXR_OK;
}
// gradient_tolerance [upstream]: max-norm of the gradient in the unscaled variables, over ALL ranks
int LmSolve::gradient_below_tolerance(bool* below) {
  double h[kScalSlots];
  RC(zero_scalars());
  if (n_c > 0) hipLaunchKernelGGL(k_count_above, blocks_for(n_c, 256), dim3(256), 0, st, (int64_t)n_c, gc, ws.scale_c.p, opt->gradient_tolerance, ws.scal.p + SCAL_GRAD_COUNT_CAM,
                                  m.det ? slimb + SCAL_GRAD_COUNT_CAM * PXR_LIMBS : (long long*)nullptr);
  hipLaunchKernelGGL(k_count_above, blocks_for(n_pts * 3, 256), dim3(256), 0, st, n_pts * 3, ws.gp.p, ws.scale_p.p, opt->gradient_tolerance, ws.scal.p + SCAL_GRAD_COUNT_PT,
                     m.det ? slimb + SCAL_GRAD_COUNT_PT * PXR_LIMBS : (long long*)nullptr);
  RC(read_scalars(h));
  *below = h[SCAL_GRAD_COUNT_PT] == 0.0 && h[SCAL_GRAD_COUNT_CAM] == 0.0;
  return PXR_OK;
}
void LmSolve::phase(int k) {
  if (!knobs.phase_timing) return;
  (void)hipStreamSynchronize(st);
  const auto now = std::chrono::steady_clock::now();
  ph_ms[k] += std::chrono::duration<double, std::milli>(now - ph_t0).count();
  ph_t0 = now;
}
int LmSolve::finish(int termination, double final_radius) {
  sum->final_radius = final_radius;
  return finish(termination);
}
int LmSolve::finish(int termination) {
  sum->termination = termination; sum->final_cost = cost;
  sum->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_loop0).count();
  return PXR_OK;
}

// ---- set-up: structure, mode, buffers, evaluation paths, launch shapes -----------------------------------------------------------
int LmSolve::setup() {
  m.geom = d_obs_xy != nullptr;
  n_obs = view->n_obs; n_pts = view->n_points; n_img = view->n_images; n_cam = view->n_cameras;
  RC(build_structure(ctx, view, h_pose_const, h_tvec_const_mask, h_cam_const_mask, h_point_const, knobs, clock, &sx));
  n_c = sx.layout.n_c; DC = sx.layout.DC; LS = sx.layout.LS; ldS = n_c + 1; nc1 = n_c ? n_c : 1;
  // linear solver by image count, like bundle_optimizer.h:180-191 overrides the user's choice
  PXR_REQUIRE(opt->linear_solver >= PXR_LINEAR_AUTO && opt->linear_solver <= PXR_LINEAR_ITERATIVE,
              "pxr_ba_solve: unknown linear_solver %d", opt->linear_solver);
  m.iterative = n_c > 0 && (opt->linear_solver == PXR_LINEAR_ITERATIVE || (opt->linear_solver == PXR_LINEAR_AUTO && n_img > PXR_MAX_IMAGES_DIRECT));
  m.multi = allreduce != nullptr || (ctx->comm != nullptr && (ctx->nranks > 1 || ctx->force_collective));   // (forced: a one-rank communicator runs the whole multi-rank branch through RCCL -- tests / bench, pxr_comm_force)
  m.native_i64 = allreduce == nullptr;
  m.det_fixed = ctx->deterministic && !m.iterative && opt->jacobi_scaling != 0;
  m.det_iter = ctx->deterministic && m.iterative;
  m.det = m.det_fixed || m.det_iter;
  m.bcast = m.multi && ctx->nranks > 1 && !m.det;
  sum->linear_solver = m.iterative ? PXR_LINEAR_ITERATIVE : PXR_LINEAR_DIRECT;
  sum->linear_iterations = 0; sum->collective_kib = 0;
  if (m.iterative) {
    StructError err;
    if (precond_blocks(sx.layout, sx.image_camera.data(), PCG_GS, &ws.precond, &err)) return struct_error(err);
  }
  RC(ws.allocate(ctx, view, sx, m));
  clock.mark("work buffers allocated");
  sum->collective_kib = (m.multi && !m.iterative) ? (int)((ws.packed_doubles * 8 + 1023) / 1024) : 0;
  sum->accumulation = m.det_fixed ? 1 : (m.det_iter ? 2 : 0); sum->initial_us = 0;

  scal_sum = ws.scal.p; scal_rep = ws.scal.p + kScalRep;
  slimb = reinterpret_cast<long long*>(ws.scal.p + kScalLimbs);
  limb_arg = m.det ? slimb : nullptr;
  d_info = reinterpret_cast<int*>(ws.scal.p + kScalInfo);   // zeroed with the scalars, read back with them
  lin_stats = ws.scal.p + kScalStats;
  rhs = ws.S.p + n_c;               // column n_c of S, stride ldS
  diagU = ws.gcd.p; gc = ws.gcd.p + nc1;
  // read back into PINNED host memory: an asynchronous copy into pageable memory (a stack array) is staged by the runtime and
  // blocks the host until it is done -- two such copies per attempt (scalars, factorisation info) left the GPU idle for ~25 us
  // each (profiles/r6_lm_timeline.txt)
  if (!ctx->h_readback) PXR_HIP(hipHostMalloc(&ctx->h_readback, 4096, hipHostMallocDefault));
  static_assert(sizeof(double) * kScalAll <= 4096, "read-back buffer");
  h_scal = static_cast<double*>(ctx->h_readback);
  std::memset(h_scal, 0, sizeof(double) * kScalAll);
  h_lin_stats = h_scal + kScalStats;
  h_info_word = reinterpret_cast<const int*>(h_scal + kScalInfo);

  cur_q = const_cast<double*>(view->d_qvec); cur_t = const_cast<double*>(view->d_tvec);
  cur_k = const_cast<double*>(view->d_cam_params); cur_X = const_cast<double*>(view->d_xyz);
  if (!records_only) hipLaunchKernelGGL(k_normalize_q, blocks_for(n_img, 256), dim3(256), 0, st, n_img, cur_q);

  dv.v = *view;
  dv.pose_off = sx.d_pose_off.p; dv.pose_dim = sx.d_pose_dim.p; dv.tmask = sx.d_tmask.p;
  dv.intr_off = sx.d_intr_off.p; dv.intr_dim = sx.d_intr_dim.p; dv.cmask = sx.d_cmask.p; dv.pt_var = sx.d_pt_var.p;
  dv.scale_c = ws.scale_c.p; dv.scale_p = ws.scale_p.p; dv.n_c = n_c; dv.DC = DC; dv.LS = LS; dv.ldS = ldS;
  cand_view = *view;
  cand_view.d_qvec = ws.q1.p; cand_view.d_tvec = ws.t1.p; cand_view.d_cam_params = ws.k1.p; cand_view.d_xyz = ws.X1.p;

  // pxr_set_gram_cache: the records from cached Gram matrices of the stencils instead of from the texels (pxr_ba_gram.hip)
  // (default on since round 5: pinned against the reference functor's vectors at 1e-5, tests/test_gram_cache_gpu.py.  check_bounds
  //  needs no care: with reference descriptors the functor ignores the bounds check, feature_reference.h:128-136.)
  // (InterpolationConfig.use_float_simd asks for the reference's ALL-fp32 splines: the Gram-matrix paths -- exact fp64 algebra -- would
  // silently compute something finer; a solve with that flag keeps the texel kernels, which have the fp32 arithmetic bit for bit)
  gram_cache = !records_only && !m.geom && ctx->gram_cache && gram_eval_supported(arena, view) && cfg->use_float_simd == 0;
  // The Gram-matrix kernel of the inner iterations keeps its matrices in the same cache from call to call (it writes back what
  // it builds), whether or not the LM loop evaluates from them: the same numbers as without a cache, fewer builds.  (That kernel
  // is built without the six extended camera models -- their forward-mode duals cost ~100 registers: a problem that uses one
  // keeps the packed kernel for every point.)
  gram_inner = !records_only && !m.geom && opt->use_inner_iterations != 0 && arena->dtype != PXR_F64 && (arena->C == 128 || arena->C == 64) &&
               !knobs.inner_packed && cfg->use_float_simd == 0;
  for (int c = 0; c < n_cam; ++c) gram_inner = gram_inner && sx.cam_model[c] <= PXR_OPENCV;
  inner_cache = gram_inner && gram_eval_supported(arena, view) && !knobs.inner_no_cache;
  if ((gram_cache || inner_cache) && gram_eval_prepare(ctx, arena, view, &gram) != PXR_OK) {
    // no memory for the cache (1.4 KB per observation, next to the solver's own buffers): not an error of this solve -- a problem
    // that fitted before the cache became the default must still run.  The LM loop evaluates from the texels (the exact-order
    // kernel), the inner iterations build their matrices at every call.
    gram_cache = false; inner_cache = false;
    (void)set_error(PXR_OK, "");    // pxr_last_error() must not keep the allocation's message
  }
  for (int c = 0; c < n_cam; ++c) geom_ext = geom_ext || sx.cam_model[c] > PXR_OPENCV;
  clock.mark("Gram-matrix cache prepared");

  if (m.iterative) {
    pcg.st = st; pcg.dv = dv;
    pcg.chunks = sx.d_schur_chunks.p; pcg.n_chunks = (int)sx.schur_chunks.size(); pcg.so = sx.d_so.p;
    pcg.pt_ptr = sx.d_pt_ptr.p; pcg.part_obs = sx.d_part_obs.p; pcg.obs_cols = sx.d_obs_cols.p;
    pcg.W = ws.W.p; pcg.T = ws.T.p; pcg.gp = ws.gp.p; pcg.gc = gc; pcg.damp_c = ws.damp_c.p; pcg.Ublk = ws.U.p;
    pcg.n_groups = (int)ws.precond.group_size.size(); pcg.col_group = as_int2(ws.col_group.p); pcg.group_size = ws.group_size.p;
    pcg.group_cols = ws.group_cols.p;
    pcg.u = ws.pcg_u.p; pcg.Mloc = ws.pcg_mloc.p; pcg.Gm = ws.pcg_g.p;
    pcg.x = ws.xsol.p; pcg.r = ws.pcg_vec.p; pcg.p = ws.pcg_vec.p + nc1; pcg.q = ws.pcg_vec.p + 2 * nc1; pcg.z = ws.pcg_vec.p + 3 * nc1;
    pcg.b = ws.pcg_vec.p + 4 * nc1; pcg.cgs = ws.pcg_scal.p; pcg.cg_part = ws.pcg_scal.p + 16; pcg.d_fail = d_info;
    pcg.det = m.det_iter;
    if (m.det_iter) {
      pcg.chunk_ptr = ws.schunk_ptr.p; pcg.col_ent_ptr = ws.col_ent_ptr.p; pcg.col_ent = as_int2(ws.col_ent.p);
      pcg.wpart = ws.det_wpart.p; pcg.mpart = ws.det_mpart.p;
    }
  }

  // the inner iterations' tables (a pass over the points on the host, two small uploads): set-up, like the observation lists
  if (gram_inner) {
    const int64_t* h_pt_ptr = sx.host.pt_ptr.data();        // (general path)
    std::vector<int64_t> pageable;
    void* wave_stage = nullptr;                              // pinned room for the table the host packs (uploaded from where it is built)
    const size_t ptr_bytes = (sizeof(int64_t) * ((size_t)n_pts + 1) + 255) & ~(size_t)255, wave_bytes = inner_wave_stage_bytes(n_pts);
    if (sx.device_lists) {                                   // fast path: the offsets come back once, through pinned memory
      int64_t* stage = (ptr_bytes + wave_bytes) <= ((size_t)1 << 28) ? static_cast<int64_t*>(setup_staging(ctx, ptr_bytes + wave_bytes)) : nullptr;
      if (stage) wave_stage = reinterpret_cast<char*>(stage) + ptr_bytes;
      else { pageable.resize((size_t)n_pts + 1); stage = pageable.data(); }
      PXR_HIP(hipMemcpyAsync(stage, sx.d_pt_ptr.p, sizeof(int64_t) * ((size_t)n_pts + 1), hipMemcpyDeviceToHost, st));
      PXR_HIP(hipStreamSynchronize(st));
      h_pt_ptr = stage;
    }
    RC(make_inner_lists(ctx, h_pt_ptr, n_pts, wave_stage, wave_stage ? wave_bytes : 0, view, sx.d_pt_ptr.p, sx.d_pt_obs.p, &inner_lists.l));
  }
  clock.mark("inner-iteration tables");
  t_loop0 = std::chrono::steady_clock::now();
  sum->setup_ms = std::chrono::duration<double, std::milli>(t_loop0 - clock.t0).count();
  sum->num_camera_unknowns = n_c; sum->num_point_unknowns = 3 * sx.n_pvar;
  sum->iterations = 0; sum->num_successful = 0; sum->termination = PXR_TERM_NO_CONVERGENCE;
  // LDS-privatised Schur contraction: column tile so that DC x CT doubles fit in 128 KiB of LDS
  CT = n_c > 0 ? std::min(n_c, (int)((128 * 1024 / 8 - DC) / DC)) : 1;
  n_ctiles = n_c > 0 ? (n_c + CT - 1) / CT : 1;
  CT = n_c > 0 ? (n_c + n_ctiles - 1) / n_ctiles : 1;       // balance the tiles
  schur_shmem = sizeof(double) * ((size_t)DC * CT + DC + 3 * 1024);   // tile, right-hand side, the lane groups' Y rows
  if (knobs.schur_lds && n_c > 0)
    PXR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(schur_lds_kernel(DC)), hipFuncAttributeMaxDynamicSharedMemorySize, (int)schur_shmem));
  PXR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_jac), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(sizeof(double) * (JAC_THREADS / 64) * 64 * (LS + 3 * DC + 1))));
  ph_t0 = std::chrono::steady_clock::now();
  return PXR_OK;
}

// ---- the reduced camera system of an attempt ---------------------------------------------------------------------------------------
// ITERATIVE_SCHUR: preconditioned conjugate gradients on the implicit Schur complement (pxr_ba_pcg.hip)
int LmSolve::reduced_step_iterative(double inv_radius, bool* ok, double* inexact_correction) {
  PcgResult pr;
  RC(pcg_solve(pcg, inv_radius, opt, [this](double* buf, int64_t count) { return ar(buf, count); }, &pr));
  phase(2);
  sum->linear_iterations += pr.iterations;
  if (!pr.ok) *ok = false;                                // LINEAR_SOLVER_FAILURE: invalid step
  // The camera step only approximately solves S x = b; the points are eliminated exactly for that x.  With
  // e = b - S x:  model cost change = delta.(D^2 delta - g) / 2 + x.e / 2
  *inexact_correction = 0.5 * pr.x_dot_r;
  PXR_HIP(hipMemsetAsync(d_info, 0, sizeof(int), st));    // (the CG loop's failure flag lives in the info word: reported through pr.ok)
  hipLaunchKernelGGL(k_finish_camera_step, blocks_for(n_c, 256), dim3(256), 0, st, n_c, ws.xsol.p, gc, ws.damp_c.p, inv_radius, ws.delta_c.p, scal_rep, limb_arg);
  return from_rank0(ws.delta_c.p, n_c);
}
// Schur complement (dense): [S + D_c / radius | rhs] in ws.S ...
int LmSolve::reduced_system_direct(double inv_radius) {
  const double schur_scale = m.det_fixed ? lin_scale : 0.0;    // the SAME grid as U's: re-quantising the finished U is exact
  hipLaunchKernelGGL(k_copy_upper_add_diag, blocks_for((int64_t)n_c * ldS, 256), dim3(256), 0, st, n_c, ws.U.p, (const double*)nullptr, 0.0, (const double*)nullptr, ws.S.p, 1, schur_scale);
  if (knobs.schur_lds) {
    const SchurLdsKernel kern = schur_lds_kernel(DC);
    hipLaunchKernelGGL(kern, dim3((unsigned)sx.schur_chunks.size(), (unsigned)n_ctiles), dim3(1024), schur_shmem, st, dv,
                       sx.d_schur_chunks.p, sx.d_so.p, sx.d_part_obs.p, sx.d_obs_cols.p, ws.W.p, ws.T.p, ws.gp.p, CT, ws.S.p, rhs, schur_scale);
  } else {
    hipLaunchKernelGGL(k_schur, blocks_for(n_obs * DC, 256), dim3(256), 0, st, dv, sx.d_pt_ptr.p, sx.d_pt_obs.p, ws.W.p, ws.T.p, ws.gp.p, ws.S.p, rhs, schur_scale);
  }
  LAUNCH_CHECK("schur kernels");
  phase(0);
  if (m.multi) {       // sum of U_local - Schur_local and of -Y g_p over the ranks: packed upper triangle + rhs
    hipLaunchKernelGGL(k_pack_upper, dim3((unsigned)n_c), dim3(256), 0, st, n_c, ws.S.p, ws.S_packed.p);
    if (schur_scale != 0.0) RC(ar_i64(reinterpret_cast<long long*>(ws.S_packed.p), ws.packed_doubles));   // the fixed-point integers
    else RC(ar(ws.S_packed.p, ws.packed_doubles));
    hipLaunchKernelGGL(k_unpack_upper, dim3((unsigned)n_c), dim3(256), 0, st, n_c, ws.S_packed.p, ws.S.p);
    LAUNCH_CHECK("pack / unpack of the reduced camera system");
  }
  phase(1);
  // the fixed-point slots back to doubles (deterministic mode), rhs += g_c (global), S += D_c / radius: one pass
  hipLaunchKernelGGL(k_copy_upper_add_diag, blocks_for((int64_t)n_c * ldS, 256), dim3(256), 0, st, n_c, ws.U.p, ws.damp_c.p, inv_radius, gc, ws.S.p, 0, schur_scale);
  return PXR_OK;
}
// ... + Cholesky
int LmSolve::reduced_step_direct(double inv_radius) {
  RC(reduced_system_direct(inv_radius));
  // row-major upper == column-major lower; the pivot check is read back with the scalars of
  // this attempt (no extra host synchronisation): a failed factorisation = invalid step.
  RC(chol_factor_solve(st, ws.S.p, n_c, d_info, ws.linv.p, ws.xsol.p, /*zero_info=*/false));     // (the attempt's first kernel cleared the info word)
  phase(2);
  hipLaunchKernelGGL(k_finish_camera_step, blocks_for(n_c, 256), dim3(256), 0, st, n_c, ws.xsol.p, gc, ws.damp_c.p, inv_radius, ws.delta_c.p, scal_rep, limb_arg);
  return from_rank0(ws.delta_c.p, n_c);
}

// ---- the candidate: back-substitution, update, inner iterations, evaluation; the attempt's scalars come to the host ----------------
int LmSolve::candidate(double inv_radius, double inexact_correction, Candidate* c) {
  const int G = lane_group(DC);
  const BacksubKernel backsub = backsub_kernel(DC);
  hipLaunchKernelGGL(backsub, blocks_for((n_pts * G + BACKSUB_PPG - 1) / BACKSUB_PPG, 256), dim3(256), 0, st, dv, sx.d_pt_ptr.p, sx.d_part_obs.p, sx.d_obs_cols.p,
                     ws.W.p, ws.T.p, ws.gp.p, ws.delta_c.p, ws.Vd0.p, inv_radius, ws.delta_p.p, scal_sum, limb_arg);
  ParamPtrs out{ws.q1.p, ws.t1.p, ws.k1.p, ws.X1.p};
  const int64_t upd_blocks = blocks_for(((int64_t)n_img + n_cam + n_pts + UPDATE_IPT - 1) / UPDATE_IPT, 256).x;
  hipLaunchKernelGGL(k_update, dim3((unsigned)upd_blocks), dim3(256), 0, st, dv, ws.delta_c.p, ws.delta_p.p, out, scal_rep, scal_sum, limb_arg);
  LAUNCH_CHECK("step kernels");
  const bool do_inner = inner_enabled;
  if (do_inner) {   // DoInnerIterationsIfNeeded [upstream]: refine every variable point of the candidate on its own
    // the cost at the unrefined candidate: per-point values, summed as limbs in every mode (one floating-point atomic per
    // point on ONE address -- 200 000 of them at configs[2] -- serialised for 0.5-1 ms of the 2-4 ms call:
    // profiles/r4_inner_cost_atomic.txt)
    PXR_HIP(hipMemsetAsync(ws.det_part.p, 0, sizeof(double) * (size_t)n_pts, st));   // points without observations stay 0
    if (m.geom) RC(launch_inner_geom(ctx, &cand_view, d_obs_xy, loss, sx.d_pt_ptr.p, sx.d_pt_obs.p, sx.d_pt_var.p, scal_sum + SCAL_COST_BEFORE_INNER, ws.det_part.p, geom_ext));
    else {
      RC(launch_inner_iterations(ctx, arena, &cand_view, cfg, loss, sx.d_pt_ptr.p, sx.d_pt_obs.p, sx.d_pt_var.p, scal_sum + SCAL_COST_BEFORE_INNER, gram_inner ? &inner_lists.l : nullptr,
                                 ws.det_part.p, (gram_cache || inner_cache) ? &gram : nullptr, gram_warm, !knobs.inner_no_prebuild));
      gram_warm = true;
    }
    hipLaunchKernelGGL(k_limb_accumulate, dim3(256), dim3(256), 0, st, (const double*)ws.det_part.p, n_pts, slimb + SCAL_COST_BEFORE_INNER * PXR_LIMBS);
    PXR_HIP(hipMemsetAsync(scal_sum + SCAL_STEP2_PT, 0, sizeof(double), st));   // point part of |x - candidate|^2 after refinement
    PXR_HIP(hipMemsetAsync(slimb + SCAL_STEP2_PT * PXR_LIMBS, 0, sizeof(long long) * PXR_LIMBS, st));
    hipLaunchKernelGGL(k_point_step_norm, blocks_for(n_pts, 256), dim3(256), 0, st, n_pts, sx.d_pt_var.p, cur_X, ws.X1.p, scal_sum + SCAL_STEP2_PT,
                       m.det ? slimb + SCAL_STEP2_PT * PXR_LIMBS : (long long*)nullptr);
    LAUNCH_CHECK("inner iteration kernels");
  }
  phase(4);
  double hs[kScalSlots];
  RC(evaluate(cand_view, rec_cand));
  RC(read_scalars(hs));
  const int h_info = *h_info_word;
  if (m.det_fixed && !lin_fits(h_lin_stats, lin_md)) {
    // the overflow guard: a slot of the linearisation this iteration was computed from did not fit its grid -- repeat the
    // linearisation on a grid from the measured trace and the iteration with it (state untouched: radius, damping, counts)
    RC(linearize_checked(rec_cur, std::max(h_lin_stats[3], 2.0 * lin_md), cost));
    if (cols_pow2 && !lin_not_finite) {      // a column outgrew its power of two: moved by the diagonal just measured, once more on the fine grid
      RC(move_columns());
      RC(linearize_checked(rec_cur, 1.0 / 8.0, cost));
    }
    c->repeat = true;
    return PXR_OK;
  }
  if (n_c > 0 && h_info != 0) c->ok = false;
  phase(5);
  c->cost = hs[SCAL_COST];
  c->model_cost_change = 0.5 * (hs[SCAL_MODEL_PT] + hs[SCAL_MODEL_CAM]) + inexact_correction;   // 0.5 * delta.(D^2 delta - g) == -(J d).(r + J d / 2)
  c->step_norm = std::sqrt(hs[SCAL_STEP2_PT] + hs[SCAL_STEP2_CAM]);
  c->x_norm = std::sqrt(hs[SCAL_X2_PT] + hs[SCAL_X2_CAM]);
  if (!(c->model_cost_change > 0.0) || !std::isfinite(c->model_cost_change)) c->ok = false;
  // A candidate that cannot be evaluated (check_bounds, a point behind a camera) is NOT an invalid step:
  // [upstream] sets candidate_cost = DBL_MAX and the step is rejected through the relative decrease.
  if (!std::isfinite(c->cost)) c->cost = std::numeric_limits<double>::max();
  inner_useful = false;
  if (c->ok && do_inner && c->cost < std::numeric_limits<double>::max()) {
    const double cost_before = hs[SCAL_COST_BEFORE_INNER];
    c->model_cost_change += cost_before - c->cost;
    inner_useful = c->cost < cost;
    inner_enabled = (1.0 - c->cost / cost_before) > opt->inner_iteration_tolerance;
  }
  return PXR_OK;
}
int LmSolve::reevaluate_current() {          // rec_cur and `cost` through the cache path
  if (!(gram_cache && cur_is_exact && n_evaluations > 1)) return PXR_OK;
  double h2[kScalSlots];
  RC(zero_scalars());
  RC(evaluate(dv.v, rec_cur));
  RC(read_scalars(h2));
  if (std::isfinite(h2[SCAL_COST])) cost = h2[SCAL_COST];
  cur_is_exact = false;
  return PXR_OK;
}
// ceres::IterationCallback (pxr_set_iteration_callback): 1 = SOLVER_ABORT, 2 = SOLVER_TERMINATE_SUCCESSFULLY
int LmSolve::notify(int iteration, bool valid, bool successful, double cost_now, double change, double rel, double radius_next, double step) {
  if (!any_cb) return 0;
  int rc = 0;
  if (ctx->iter_cb) {
    pxr_iteration_summary is;
    is.iteration = iteration; is.step_is_valid = valid; is.step_is_successful = successful; is.cost = cost_now; is.cost_change = change;
    is.relative_decrease = rel; is.trust_region_radius = radius_next; is.step_norm = step;
    rc = ctx->iter_cb(&is, ctx->iter_user);
  }
  if (m.multi) {
    // every rank must leave the loop at the same iteration (the next collective would hang otherwise): the answers are
    // summed over the ranks, an abort anywhere aborts everywhere, else a termination request anywhere terminates
    double h[2] = {rc == 1 ? 1.0 : 0.0, rc == 2 ? 1.0 : 0.0};
    if (hipMemcpyAsync(ws.cb_flags.p, h, sizeof(h), hipMemcpyHostToDevice, st) != hipSuccess || ar(ws.cb_flags.p, 2) != PXR_OK ||
        hipMemcpyAsync(h, ws.cb_flags.p, sizeof(h), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
      return 1;
    rc = h[0] > 0.0 ? 1 : (h[1] > 0.0 ? 2 : 0);
  }
  return rc;
}
bool LmSolve::user_stop(int rc) {   // true: leave the loop
  if (rc == 1) { sum->termination = PXR_TERM_FAILURE; return true; }
  if (rc == 2) { sum->termination = PXR_TERM_CONVERGENCE; return true; }
  return false;
}

// ---- the trust-region loop [upstream Ceres 2.1 trust_region_minimizer.cc] ------------------------------------------------------------
int LmSolve::run() {
  // ---- iteration 0: evaluate, Jacobi scaling, linearise
  double hs[kScalSlots];
  rec_cur = ws.rec_a.p; rec_cand = ws.rec_b.p;
  RC(zero_scalars());
  RC(evaluate(dv.v, rec_cur));
  RC(read_scalars(hs));
  cost = hs[SCAL_COST];
  sum->initial_cost = cost;
  if (!std::isfinite(cost)) return finish(PXR_TERM_FAILURE);   // [upstream] "Initial residual and Jacobian evaluation failed" (e.g. check_bounds)
  hipLaunchKernelGGL(k_fill, blocks_for(nc1, 256), dim3(256), 0, st, (int64_t)nc1, 1.0, ws.scale_c.p);
  hipLaunchKernelGGL(k_fill, blocks_for(nc1, 256), dim3(256), 0, st, (int64_t)nc1, 1.0, ws.pow_c.p);
  hipLaunchKernelGGL(k_fill, blocks_for(n_pts * 3, 256), dim3(256), 0, st, n_pts * 3, 1.0, ws.scale_p.p);
  // (deterministic mode: the UNSCALED pass only yields diag(U) for the Jacobi scaling and has no a-priori bound: a first guess
  //  of 2^32 for its diagonal -- unit-norm descriptors give 1e3 .. 1e6 -- and the checked retry from the measured trace otherwise)
  RC(linearize_checked(rec_cur, std::ldexp(1.0, 32), cost, !opt->jacobi_scaling));
  if (lin_not_finite) return finish(PXR_TERM_FAILURE, opt->initial_radius);
  if (opt->jacobi_scaling) {   // 1 / (1 + sqrt(diag(J~^T J~))), fixed for the whole solve
    if (m.det_fixed && n_c > 0) {
      RC(resolve_small_columns(rec_cur));
      if (lin_not_finite) return finish(PXR_TERM_FAILURE, opt->initial_radius);
    }
    if (n_c > 0 && cols_pow2) hipLaunchKernelGGL(k_jacobi_scale_pow2, blocks_for(n_c, 256), dim3(256), 0, st, (int64_t)n_c, diagU, ws.scale_c.p, ws.pow_c.p);
    else if (n_c > 0) hipLaunchKernelGGL(k_jacobi_scale, blocks_for(n_c, 256), dim3(256), 0, st, (int64_t)n_c, diagU, ws.scale_c.p);
    hipLaunchKernelGGL(k_point_diag, blocks_for(n_pts, 256), dim3(256), 0, st, n_pts, ws.V.p, ws.Vd0.p);
    hipLaunchKernelGGL(k_jacobi_scale, blocks_for(n_pts * 3, 256), dim3(256), 0, st, n_pts * 3, ws.Vd0.p, ws.scale_p.p);
    RC(linearize_checked(rec_cur, 1.0 / 8.0, cost));      // scaled columns have norm < 1: diag(U) < 1 = 8 x 1/8
    if (lin_not_finite) return finish(PXR_TERM_FAILURE, opt->initial_radius);
  }
  if (opt->gradient_tolerance > 0.0) {   // [upstream] the test is also made at iteration 0
    bool below = false;
    RC(gradient_below_tolerance(&below));
    if (below) return finish(PXR_TERM_CONVERGENCE, opt->initial_radius);
  }
  radius = opt->initial_radius; decrease_factor = 2.0;
  invalid = 0; reuse_diag = false;
  inner_enabled = opt->use_inner_iterations != 0; inner_useful = false;
  PXR_HIP(hipStreamSynchronize(st));         // (already idle in the deterministic mode: linearize_checked synchronises)
  sum->initial_us = (int32_t)std::min<double>(2e9, 1e3 * std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_loop0).count());
  // Several ranks: a callback installed on SOME ranks only (rank 0 logging, say) must not put the ranks' collectives out of
  // step -- whether any rank has one is agreed on once here; if so, every rank joins the per-iteration exchange of answers
  // (a rank without a callback answers "continue").
  any_cb = ctx->iter_cb != nullptr;
  if (m.multi) {
    double h = any_cb ? 1.0 : 0.0;
    PXR_HIP(hipMemcpyAsync(ws.cb_flags.p, &h, sizeof(h), hipMemcpyHostToDevice, st));
    RC(ar(ws.cb_flags.p, 1));
    PXR_HIP(hipMemcpyAsync(&h, ws.cb_flags.p, sizeof(h), hipMemcpyDeviceToHost, st));
    PXR_HIP(hipStreamSynchronize(st));
    any_cb = h > 0.0;
  }
  if (user_stop(notify(0, false, false, cost, 0.0, 0.0, radius, 0.0))) return finish(sum->termination, radius);

  while (true) {
    if (sum->iterations >= opt->max_iterations) { sum->termination = PXR_TERM_NO_CONVERGENCE; break; }
    if (radius < opt->min_radius) { sum->termination = PXR_TERM_CONVERGENCE; break; }
    ++sum->iterations;
    phase(7);
    if (!reuse_diag) RC(refresh_damping());
    const double inv_radius = 1.0 / radius;
    // point elimination (+ the side job of the attempt's first kernel: clear the attempt's scalars), reduced camera system
    hipLaunchKernelGGL(k_pinv, blocks_for(n_pts, 256), dim3(256), 0, st, n_pts, sx.d_pt_var.p, ws.V.p, ws.Vd0.p, inv_radius, ws.T.p, ws.scal.p, kScalZeroed);
    if (n_pts == 0) RC(zero_scalars());
    Candidate c;
    double inexact_correction = 0.0;
    if (n_c > 0 && m.iterative) RC(reduced_step_iterative(inv_radius, &c.ok, &inexact_correction));
    else if (n_c > 0) RC(reduced_step_direct(inv_radius));
    phase(3);
    if (c.ok) {
      RC(candidate(inv_radius, inexact_correction, &c));
      if (c.repeat) {
        if (lin_not_finite) { sum->termination = PXR_TERM_FAILURE; break; }
        --sum->iterations;
        continue;
      }
    }
    if (knobs.verbose)
      fprintf(stderr, "[pxr_ba_solve] it %3d cost %.9e cand %.9e mcc %.3e radius %.3e |dx| %.3e %s\n", sum->iterations,
              cost, c.cost, c.model_cost_change, radius, c.step_norm, c.ok ? "" : "INVALID");
    if (!c.ok) {   // HandleInvalidStep
      if (++invalid >= opt->max_consecutive_invalid_steps) { sum->termination = PXR_TERM_FAILURE; break; }
      radius *= 0.5; reuse_diag = true;
      if (user_stop(notify(sum->iterations, false, false, cost, 0.0, 0.0, radius, c.step_norm))) break;
      continue;
    }
    invalid = 0;
    if (c.step_norm <= opt->parameter_tolerance * (c.x_norm + opt->parameter_tolerance)) { sum->termination = PXR_TERM_CONVERGENCE; break; }
    const double cost_change = cost - c.cost;
    if (std::fabs(cost_change) <= opt->function_tolerance * cost) { sum->termination = PXR_TERM_CONVERGENCE; break; }
    const double rel = cost_change / c.model_cost_change;
    if (inner_useful || rel > opt->min_relative_decrease) {   // IsStepSuccessful + HandleSuccessfulStep
      // the accepted candidate becomes the current point
      Copy4 c4{{ws.q1.p, ws.t1.p, ws.k1.p, ws.X1.p}, {cur_q, cur_t, cur_k, cur_X},
               {(int64_t)4 * n_img, (int64_t)3 * n_img, (int64_t)PXR_KPAD * n_cam, (int64_t)3 * n_pts}};
      hipLaunchKernelGGL(k_copy4, dim3((unsigned)std::min<int64_t>(1024, blocks_for(3 * n_pts + 1, 256).x)), dim3(256), 0, st, c4);
      std::swap(rec_cur, rec_cand);
      cost = c.cost;
      cur_is_exact = false;
      if (m.det_fixed) { lin_md = std::max(h_lin_stats[0], 1e-300); lin_scale = det_scale_for(lin_md, cost); }   // checked with the next iteration's scalars
      if (cols_pow2) RC(move_columns());      // (by the diagonal at the point that is left: a factor 4 of drift at most is carried along)
      RC(linearize(rec_cur));
      phase(6);
      ++sum->num_successful;
      const double tmp = 2.0 * rel - 1.0;
      radius = radius / std::max(1.0 / 3.0, 1.0 - tmp * tmp * tmp);
      radius = std::min(opt->max_radius, radius);
      decrease_factor = 2.0; reuse_diag = false;
      if (opt->gradient_tolerance > 0.0) {
        bool below = false;
        RC(gradient_below_tolerance(&below));
        if (below) { sum->termination = PXR_TERM_CONVERGENCE; break; }
      }
      if (user_stop(notify(sum->iterations, true, true, cost, cost_change, rel, radius, c.step_norm))) break;
    } else {   // StepRejected
      RC(reevaluate_current());
      radius = radius / decrease_factor; decrease_factor *= 2.0; reuse_diag = true;
      if (user_stop(notify(sum->iterations, true, false, cost, cost_change, rel, radius, c.step_norm))) break;
    }
  }
  PXR_HIP(hipStreamSynchronize(st));
  if (knobs.phase_timing)
    fprintf(stderr, "[pxr_ba_solve] phase ms over %d iterations: schur-build %.2f allreduce %.2f potrf %.2f potrs %.2f "
            "backsub+update %.2f eval+cost %.2f linearize %.2f other %.2f\n", sum->iterations, ph_ms[0], ph_ms[1],
            ph_ms[2], ph_ms[3], ph_ms[4], ph_ms[5], ph_ms[6], ph_ms[7]);
  return finish(sum->termination, radius);
}

// ---- the covariance's linear algebra up to the factor of S (pxr_ba_cov.hip has the rest) -------------------------------------------
// The linearisation of the LM loop at the caller's records, WITHOUT damping: columns moved into [1/4, 1) by powers of two alone
// (scale_c starts at 1 and only k_column_pow2 touches it: S_scaled = D S D exactly, the covariance is D inv(S_scaled) D without a
// rounding), points unscaled, T_p = inv(V_p) from k_pinv_checked, then reduced_system_direct at 1 / radius = 0: the Schur
// complement on the grid of the deterministic mode, in the layout chol_factor_solve takes.
int LmSolve::covariance_system(const double* rec, int* singular, unsigned long long* n_singular, CovSystem* out) {
  double hs[kScalSlots];
  RC(zero_scalars());
  hipLaunchKernelGGL(k_cost_limbs, dim3(1024), dim3(256), 0, st, rec, n_obs, *loss, slimb + SCAL_COST * PXR_LIMBS);
  LAUNCH_CHECK("cost");
  RC(read_scalars(hs));
  cost = hs[SCAL_COST];
  PXR_REQUIRE(std::isfinite(cost), "pxr_ba_covariance: the records do not give a finite cost");
  hipLaunchKernelGGL(k_fill, blocks_for(nc1, 256), dim3(256), 0, st, (int64_t)nc1, 1.0, ws.scale_c.p);
  hipLaunchKernelGGL(k_fill, blocks_for(nc1, 256), dim3(256), 0, st, (int64_t)nc1, 1.0, ws.pow_c.p);
  hipLaunchKernelGGL(k_fill, blocks_for(nc1, 256), dim3(256), 0, st, (int64_t)nc1, 1.0, ws.damp_c.p);
  hipLaunchKernelGGL(k_fill, blocks_for(n_pts * 3, 256), dim3(256), 0, st, n_pts * 3, 1.0, ws.scale_p.p);
  RC(linearize_checked(rec, std::ldexp(1.0, 32), cost));
  if (n_c > 0 && !lin_not_finite) {
    if (m.det_fixed) RC(resolve_small_columns(rec));
    if (!lin_not_finite) {
      RC(move_columns());
      RC(linearize_checked(rec, 1.0 / 8.0, cost));
    }
  }
  PXR_REQUIRE(!lin_not_finite, "pxr_ba_covariance: the Jacobian at these parameters is not finite");
  RC(zero_scalars());
  PXR_HIP(hipMemsetAsync(n_singular, 0, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_pinv_checked, blocks_for(n_pts, 256), dim3(256), 0, st, n_pts, sx.d_pt_var.p, ws.V.p, ws.T.p, singular, n_singular);
  LAUNCH_CHECK("k_pinv_checked");
  if (n_c > 0) RC(reduced_system_direct(0.0));
  out->dv = dv; out->n_c = n_c; out->DC = DC;
  out->aug = ws.S.p; out->linv = ws.linv.p; out->xsol = ws.xsol.p; out->d_info = d_info; out->scratch = ws.U.p;
  out->W = ws.W.p; out->T = ws.T.p; out->pt_ptr = sx.d_pt_ptr.p; out->pt_obs = sx.d_pt_obs.p;
  out->deterministic = m.det_fixed;
  return PXR_OK;
}

int ba_cov_system(pxr_ctx* ctx, const pxr_ba_view* view, const double* d_rec, const pxr_loss* loss, const uint8_t* h_pose_const,
                  const uint8_t* h_tvec_const_mask, const uint16_t* h_cam_const_mask, const uint8_t* h_point_const, int* d_singular,
                  unsigned long long* d_n_singular, const std::function<int(const CovSystem&)>& then) {
  const SolveKnobs knobs;
  const SetupClock clock{knobs.verbose};
  ArenaScope arena_scope(ctx, knobs.arena);
  pxr_lm_options opt;
  std::memset(&opt, 0, sizeof(opt));
  opt.jacobi_scaling = 1; opt.linear_solver = PXR_LINEAR_DIRECT; opt.min_lm_diagonal = 1e-6; opt.max_lm_diagonal = 1e32;
  pxr_lm_summary sum;
  std::memset(&sum, 0, sizeof(sum));
  LmSolve s{ctx, nullptr, view, nullptr, nullptr, loss, h_pose_const, h_tvec_const_mask, h_cam_const_mask, h_point_const, &opt, nullptr, nullptr, &sum,
            knobs, ctx->stream, clock};
  s.records_only = true;
  RC(s.setup());
  PXR_REQUIRE(!s.m.multi, "pxr_ba_covariance: not available with a communicator (several ranks)");
  CovSystem sys;
  RC(s.covariance_system(d_rec, d_singular, d_n_singular, &sys));
  return then(sys);
}

static int ba_solve(pxr_ctx* ctx, pxr_arena* arena, const pxr_ba_view* view, const pxr_interp_cfg* cfg, const double* d_obs_xy,
                    const pxr_loss* loss, const uint8_t* h_pose_const, const uint8_t* h_tvec_const_mask,
                    const uint16_t* h_cam_const_mask, const uint8_t* h_point_const,
                    const pxr_lm_options* opt, pxr_allreduce_fn allreduce, void* ar_user, pxr_lm_summary* sum) {
  PXR_REQUIRE(ctx && view && loss && opt && sum && (d_obs_xy || (arena && cfg)), "pxr_ba_solve: NULL argument");
  PXR_REQUIRE(h_pose_const && h_tvec_const_mask && h_cam_const_mask && h_point_const,
              "pxr_ba_solve: NULL parameterisation array");
  PXR_REQUIRE(view->n_obs > 0, "pxr_ba_solve: problem has no residuals (bundle_optimizer.h:174-176)");
  PXR_HIP(hipSetDevice(ctx->device));
  const SolveKnobs knobs;
  const SetupClock clock{knobs.verbose};
  ArenaScope arena_scope(ctx, knobs.arena);
  LmSolve s{ctx, arena, view, cfg, d_obs_xy, loss, h_pose_const, h_tvec_const_mask, h_cam_const_mask, h_point_const, opt, allreduce, ar_user, sum,
            knobs, ctx->stream, clock};
  RC(s.setup());
  return s.run();
}

}  // namespace pxr

extern "C" int pxr_ba_solve(pxr_ctx* ctx, pxr_arena* arena, const pxr_ba_view* view, const pxr_interp_cfg* cfg,
                            const pxr_loss* loss, const uint8_t* h_pose_const, const uint8_t* h_tvec_const_mask,
                            const uint16_t* h_cam_const_mask, const uint8_t* h_point_const,
                            const pxr_lm_options* opt, pxr_allreduce_fn allreduce, void* ar_user,
                            pxr_lm_summary* sum) {
  PXR_REQUIRE(arena && cfg, "pxr_ba_solve: NULL argument");
  return pxr::ba_solve(ctx, arena, view, cfg, nullptr, loss, h_pose_const, h_tvec_const_mask, h_cam_const_mask, h_point_const, opt,
                       allreduce, ar_user, sum);
}

extern "C" int pxr_ba_solve_geometric(pxr_ctx* ctx, const pxr_ba_view* view, const double* d_obs_xy, const pxr_loss* loss,
                                      const uint8_t* h_pose_const, const uint8_t* h_tvec_const_mask,
                                      const uint16_t* h_cam_const_mask, const uint8_t* h_point_const,
                                      const pxr_lm_options* opt, pxr_allreduce_fn allreduce, void* ar_user,
                                      pxr_lm_summary* sum) {
  PXR_REQUIRE(d_obs_xy, "pxr_ba_solve_geometric: the observed keypoints are missing");
  return pxr::ba_solve(ctx, nullptr, view, nullptr, d_obs_xy, loss, h_pose_const, h_tvec_const_mask, h_cam_const_mask, h_point_const,
                       opt, allreduce, ar_user, sum);
}
