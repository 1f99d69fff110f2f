// pxr_ba_geom.hip -- geometric (reprojection-error) bundle adjustment on gfx950: the evaluation and the inner
// iterations that need no patch arena.
//
// Replaces GeometricBundleOptimizer::AddResiduals' cost functions (bundle_adjustment/src/geometric_bundle_optimizer.h:39-88,
// residuals/src/geometric.h -> [upstream COLMAP 3.8] BundleAdjustmentCostFunction / ...ConstantPoseCostFunction):
//     r = WorldToPixel(camera, q, t, X) - xy_observed                         (2 residuals per observation)
// The solver (pxr_ba_solve.hip) consumes the 64-byte record of pxr_ba_eval and the projection Jacobian only.  With
// J = I_2 P the record of an observation is
//     [s, gx.gx, gx.gy, gy.gy, gx.r, gy.r, x, y] = [rx^2 + ry^2, 1, 0, 1, rx, ry, x, y]
// at linearisation points and trial points alike, so there is one kernel and no with_jacobian variant.
//
//   geom_eval_kernel   one lane per observation; the wavefront's 64 records are assembled in LDS and leave as four fully
//                      coalesced 1 KiB stores (16 bytes per lane, consecutive lanes consecutive addresses)
//   k_inner_geom       Ceres' inner iterations (pxr_ba_inner.hip's header comment): the nested per-point TR-LM with the
//                      reprojection residual -- one observation per lane, a point per group of 8 lanes, longer tracks in passes
#include <hip/hip_runtime.h>

#include "pxr_device.h"
#include "pxr_inner_lm.h"
#include "pxr_internal.h"

namespace pxr {

// ---- evaluation --------------------------------------------------------------------------------------------------------------
constexpr int GEOM_THREADS = 256;

__global__ __launch_bounds__(GEOM_THREADS) void geom_eval_kernel(const pxr_ba_view v, const double* __restrict__ obs_xy,
                                                                 double* __restrict__ rec, double* __restrict__ res) {
  // The records are staged per wavefront ([64][8] doubles) and stored by the wavefront as one contiguous 4 KiB stream:
  // store j of lane l is the double2 at (j * 64 + l) * 16 bytes, i.e. every global_store_dwordx4 of the wavefront covers eight
  // whole 128-byte lines.  (Four 16-byte stores per lane straight from registers are also dwordx4, but each instruction
  // then touches 64 lines a quarter at a time.)
  __shared__ double2 stage[GEOM_THREADS / 64][64 * 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * GEOM_THREADS + wave * 64;   // first observation of this wavefront
  const int64_t i = i0 + lane;
  if (i0 >= v.n_obs) return;                                           // (wavefront-uniform)
  const int n_valid = (int)min((int64_t)64, v.n_obs - i0);
  if (i < v.n_obs) {
    const int img = v.d_obs_image[i], pt = v.d_obs_point[i], cam = v.d_image_camera[img];
    const double2 o = reinterpret_cast<const double2*>(obs_xy)[i];
    double q[4], t[3], X[3], k[PXR_KPAD];
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = v.d_qvec[4 * (size_t)img + j];
#pragma unroll
    for (int j = 0; j < 3; ++j) { t[j] = v.d_tvec[3 * (size_t)img + j]; X[j] = v.d_xyz[3 * (size_t)pt + j]; }
#pragma unroll
    for (int j = 0; j < PXR_KPAD; ++j) k[j] = v.d_cam_params[(size_t)cam * PXR_KPAD + j];
    double x, y;
    world_to_pixel(v.d_cam_model[cam], k, q, t, X, x, y);
    const double rx = x - o.x, ry = y - o.y;
    double2* row = stage[wave] + 4 * lane;
    row[0] = make_double2(fma(ry, ry, rx * rx), 1.0);
    row[1] = make_double2(0.0, 1.0);
    row[2] = make_double2(rx, ry);
    row[3] = make_double2(x, y);
    if (res) reinterpret_cast<double2*>(res)[i] = make_double2(rx, ry);
  }
  __threadfence_block();                        // LDS rows of the other lanes of this wavefront
  __builtin_amdgcn_wave_barrier();
  double2* out = reinterpret_cast<double2*>(rec + (size_t)i0 * PXR_OBS_REC);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int x = j * 64 + lane;
    if (x < 4 * n_valid) out[x] = stage[wave][x];
  }
}

int geom_eval(pxr_ctx* ctx, const pxr_ba_view* view, const double* d_obs_xy, double* d_rec, double* d_res) {
  if (view->n_obs == 0) return PXR_OK;
  const unsigned blocks = (unsigned)((view->n_obs + GEOM_THREADS - 1) / GEOM_THREADS);
  hipLaunchKernelGGL(geom_eval_kernel, dim3(blocks), dim3(GEOM_THREADS), 0, ctx->stream, *view, d_obs_xy, d_rec, d_res);
  return hip_check(hipGetLastError(), "geom_eval_kernel launch");
}

// ---- inner iterations ----------------------------------------------------------------------------------------------------------
// A wavefront runs 8 points, each on 8 lanes (one DPP half-row: the sums over a point's observations are three DPP steps) with one
// observation per lane; a track of more than 8 observations takes ceil(n / 8) passes.  The nested LM evaluates the same
// observations ~10 times: their image / camera parameters and keypoints are gathered once into LDS (the first GEOM_MAXO of a
// track; the tail of a longer one reads global memory at every evaluation).  All decisions of the nested LM are taken on sums
// every lane of the group holds, so the 8 lanes of a point stay convergent and the groups of a wavefront diverge freely.
// Only the point moves: an observation is staged as the rotation matrix of its image's quaternion, the translation, the camera
// parameters and the keypoint, and the evaluation needs d(x,y)/d(u,v) of the camera model alone (camera_model_jac<false>: no
// d/dk, no d/dq -- the full world_to_pixel_jac put this kernel at 256 VGPRs + 42 AGPRs and 32 bytes of scratch).
constexpr int GEOM_PPW = 8, GEOM_MAXO = 8, GEOM_OBS = 27;   // R(9) t(3) k(12) model xy(2)

struct GeomInnerArgs {
  pxr_ba_view v;               // candidate parameters; d_xyz is updated in place
  const double* obs_xy;
  pxr_loss loss;
  const int64_t* pt_ptr; const int64_t* pt_obs; const int* pt_var;
  double* xyz_out;             // == v.d_xyz (mutable alias)
  double* cost_before;         // += the cost at the unrefined candidate (cost_pt == NULL)
  double* cost_pt;             // [n_points] the per-point costs instead, summed by the caller in a fixed order
};

// EXT: with the six fisheye / full-OpenCV / FOV models (forward-mode duals).  The host launches that instantiation only for a
// problem that uses one of them: 256 VGPRs + 46 AGPRs, one wavefront per SIMD, against 188 VGPRs and two without.
template <bool EXT>
__global__ __launch_bounds__(64) void k_inner_geom(const GeomInnerArgs a) {
  __shared__ double sh_obs[GEOM_PPW][GEOM_MAXO][GEOM_OBS];
  const int lane = threadIdx.x & 7, slot = threadIdx.x >> 3;
  const int64_t p = (int64_t)blockIdx.x * GEOM_PPW + slot;
  if (p >= a.v.n_points) return;
  const int64_t o0 = a.pt_ptr[p];
  const int n = (int)(a.pt_ptr[p + 1] - o0);
  if (n == 0) return;
  const bool variable = a.pt_var[p] != 0;
  double X[3] = {a.v.d_xyz[3 * p], a.v.d_xyz[3 * p + 1], a.v.d_xyz[3 * p + 2]};

  auto gather = [&](int oc, double* R, double* t, double* k, int& model, double& ox, double& oy) {
    const int64_t i = a.pt_obs[o0 + oc];
    const int img = a.v.d_obs_image[i], cam = a.v.d_image_camera[img];
    quat_to_rotation(a.v.d_qvec + 4 * (size_t)img, R);
#pragma unroll
    for (int j = 0; j < 3; ++j) t[j] = a.v.d_tvec[3 * (size_t)img + j];
#pragma unroll
    for (int j = 0; j < PXR_KPAD; ++j) k[j] = a.v.d_cam_params[(size_t)cam * PXR_KPAD + j];
    model = a.v.d_cam_model[cam];
    ox = a.obs_xy[2 * i]; oy = a.obs_xy[2 * i + 1];
  };
  if (lane < n) {                              // (n <= GEOM_MAXO lanes stage, one observation each)
    double* ob = sh_obs[slot][lane];
    int model;
    gather(lane, ob, ob + 9, ob + 12, model, ob[25], ob[26]);
    ob[24] = (double)model;
  }
  __threadfence_block();
  __builtin_amdgcn_wave_barrier();

  // cost (+ normal equations H (6: xx xy xz yy yz zz), g (3)) of this point at Xc; every lane of the group gets the sums
  auto eval = [&](const double* Xc, bool with_jac, double* Hn, double* gn) -> double {
    double cost = 0.0, acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int chunk = 0; chunk < n; chunk += 8) {
      const int oi = chunk + lane;
      const bool valid = oi < n;
      const int oc = valid ? oi : n - 1;
      double R[9], t[3], k[PXR_KPAD], ox, oy;
      int model;
      if (oc < GEOM_MAXO) {
        const double* ob = sh_obs[slot][oc];
#pragma unroll
        for (int j = 0; j < 9; ++j) R[j] = ob[j];
#pragma unroll
        for (int j = 0; j < 3; ++j) t[j] = ob[9 + j];
#pragma unroll
        for (int j = 0; j < PXR_KPAD; ++j) k[j] = ob[12 + j];
        model = (int)ob[24]; ox = ob[25]; oy = ob[26];
      } else {
        gather(oc, R, t, k, model, ox, oy);
      }
      const double p0 = fma(R[0], Xc[0], fma(R[1], Xc[1], fma(R[2], Xc[2], t[0])));
      const double p1 = fma(R[3], Xc[0], fma(R[4], Xc[1], fma(R[5], Xc[2], t[1])));
      const double p2 = fma(R[6], Xc[0], fma(R[7], Xc[1], fma(R[8], Xc[2], t[2])));
      const double iz = 1.0 / p2, un = p0 * iz, vn = p1 * iz;
      double x, y, Juv[2][2], PX[2][3];
      camera_model_jac<false, EXT>(model, k, un, vn, x, y, Juv, nullptr);
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const double A0 = Juv[r][0] * iz, A1 = Juv[r][1] * iz, A2 = -(Juv[r][0] * un + Juv[r][1] * vn) * iz;
#pragma unroll
        for (int m = 0; m < 3; ++m) PX[r][m] = A0 * R[m] + A1 * R[3 + m] + A2 * R[6 + m];
      }
      const double rx = x - ox, ry = y - oy;
      const double s = fma(ry, ry, rx * rx);
      double rho[3];
      loss_eval(a.loss.type, a.loss.a, 1.0, s, rho);
      if (valid) cost += 0.5 * rho[0];
      if (with_jac) {
        const double kappa = loss_corrector_kappa(s, rho);
        const double w8 = valid ? rho[1] : 0.0;
        // M~ = rho' (I - kappa r r^T), b~ = rho' r
        const double m00 = w8 * (1.0 - kappa * rx * rx), m01 = w8 * (-kappa * rx * ry), m11 = w8 * (1.0 - kappa * ry * ry);
        const double b0 = w8 * rx, b1 = w8 * ry;
        double me0[3], me1[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) { me0[j] = m00 * PX[0][j] + m01 * PX[1][j]; me1[j] = m01 * PX[0][j] + m11 * PX[1][j]; }
        acc[0] += PX[0][0] * me0[0] + PX[1][0] * me1[0];
        acc[1] += PX[0][0] * me0[1] + PX[1][0] * me1[1];
        acc[2] += PX[0][0] * me0[2] + PX[1][0] * me1[2];
        acc[3] += PX[0][1] * me0[1] + PX[1][1] * me1[1];
        acc[4] += PX[0][1] * me0[2] + PX[1][1] * me1[2];
        acc[5] += PX[0][2] * me0[2] + PX[1][2] * me1[2];
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[6 + j] += PX[0][j] * b0 + PX[1][j] * b1;
      }
    }
    cost = row8_sum(cost);
    if (with_jac) {
#pragma unroll
      for (int j = 0; j < 6; ++j) Hn[j] = row8_sum(acc[j]);
#pragma unroll
      for (int j = 0; j < 3; ++j) gn[j] = row8_sum(acc[6 + j]);
    }
    return cost;
  };

  double H[6], g[3];
  const double cost = eval(X, variable, H, g);
  if (lane == 0) { if (a.cost_pt) a.cost_pt[p] = cost; else atomicAdd(a.cost_before, cost); }
  if (!variable) return;
  if (!nested_point_lm(X, cost, H, g, eval)) return;
  if (lane == 0) { a.xyz_out[3 * p] = X[0]; a.xyz_out[3 * p + 1] = X[1]; a.xyz_out[3 * p + 2] = X[2]; }
}

// Enqueue the inner iterations on the candidate parameters `view` (xyz refined in place); d_cost_per_point [n_points] (or, when
// NULL, *d_cost_before, caller-zeroed) receives the cost at the unrefined candidate.  extended_models: a camera of the problem
// has a model id above PXR_OPENCV.
int launch_inner_geom(pxr_ctx* ctx, const pxr_ba_view* view, const double* d_obs_xy, const pxr_loss* loss, const int64_t* d_pt_ptr,
                      const int64_t* d_pt_obs, const int* d_pt_var, double* d_cost_before, double* d_cost_per_point,
                      bool extended_models) {
  const unsigned blocks = (unsigned)((view->n_points + GEOM_PPW - 1) / GEOM_PPW);
  if (blocks == 0) return PXR_OK;
  GeomInnerArgs a;
  a.v = *view; a.obs_xy = d_obs_xy; a.loss = *loss;
  a.pt_ptr = d_pt_ptr; a.pt_obs = d_pt_obs; a.pt_var = d_pt_var;
  a.xyz_out = const_cast<double*>(view->d_xyz); a.cost_before = d_cost_before; a.cost_pt = d_cost_per_point;
  if (extended_models) hipLaunchKernelGGL(k_inner_geom<true>, dim3(blocks), dim3(64), 0, ctx->stream, a);
  else hipLaunchKernelGGL(k_inner_geom<false>, dim3(blocks), dim3(64), 0, ctx->stream, a);
  return hip_check(hipGetLastError(), "k_inner_geom launch");
}

}  // namespace pxr

extern "C" int pxr_ba_geom_eval(pxr_ctx* ctx, const pxr_ba_view* view, const double* d_obs_xy, double* d_rec, double* d_res) {
  PXR_REQUIRE(ctx && view && d_rec, "pxr_ba_geom_eval: NULL argument");
  PXR_REQUIRE(view->n_obs >= 0, "pxr_ba_geom_eval: negative n_obs");
  PXR_REQUIRE(d_obs_xy || view->n_obs == 0, "pxr_ba_geom_eval: the observed keypoints are missing");
  PXR_HIP(hipSetDevice(ctx->device));
  return pxr::geom_eval(ctx, view, d_obs_xy, d_rec, d_res);
}
