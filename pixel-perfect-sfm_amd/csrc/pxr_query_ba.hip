// pxr_query_ba.hip -- the query bundle adjustment of a whole batch of queries in one launch (pxr_query_ba_solve): per query one
// image against CONSTANT 3D points, the pose on the quaternion manifold plus the translation (six tangent unknowns), the
// trust-region loop inside the kernel.
//
// One unit of work = one query = one workgroup of 256 lanes.  A residual block occupies C / 8 lanes, 8 channels each -- interp8's
// lane group, the arithmetic of pxr_ba_eval -- so a pass of the workgroup covers 16 blocks at C = 128 and 32 at C = 64; block j of
// the query belongs to lane group j mod G in pass j / G: the assignment depends on nothing but the query.
//   evaluation at a pose: per block (x, y) = WorldToPixel, the descriptor and its gradients at (x, y), r = f - ref, the six
//   dot products of pxr_ba_eval's record reduced inside the lane group; then the block's 2 x 6 projection Jacobian
//   P = d(x, y) / d(rotation tangent, t), and with G = the 2 x 2 Gram matrix of the gradients and b = their products with r:
//     J^T J = P^T G P,  J^T r = P^T b,  the robustifier's corrector on both (loss_corrector_kappa), cost = rho(|r|^2) / 2.
//   The group's first lane adds the 28 values (21 + 6 + 1) to the group's slot in LDS, pass after pass; the slots are then summed
//   in group order by one lane per value.  No atomics, no order that depends on timing: a query's sums are a function of the
//   query's own data, bit for bit, whatever else is in the batch.
//   loop: every lane takes the same 6 x 6 Cholesky step and the same decisions from the same sums ([upstream Ceres 2.1]
//   trust_region_minimizer.cc as restated in oracle/pxo_solve.c: ba_lm_run with one image and every point constant).
// The value AND the linearisation are evaluated at every trial pose and kept on acceptance (Ceres evaluates the cost first and the
// Jacobian only after acceptance: the same values, hence the same trajectory): a rejected step wastes the Jacobian's share of an
// evaluation (the 2 x 6 geometry and the gradient passes of the splines), an accepted one saves a whole second evaluation -- the
// stencil loads and both spline passes -- and most steps are accepted.
// What the loop needs between two evaluations lives in LDS (the pose, the trial pose, the intrinsics, the scaled system): an
// evaluation has the registers to itself.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "pxr_batch.h"
#include "pxr_device.h"
#include "pxr_dispatch.h"
#include "pxr_inner_lm.h"
#include "pxr_internal.h"
#include "pxr_interp.h"
#include "pxr_robust.h"

namespace pxr {

constexpr int QBA_THREADS = 256;
constexpr int QBA_D = 6;                                  // tangent unknowns: rotation (3), translation (3)
constexpr int QBA_H = QBA_D * (QBA_D + 1) / 2;            // the upper triangle of J^T J by rows
constexpr int QBA_NS = QBA_H + QBA_D + 1;                 // ... then J^T r, then the cost

struct QbaOut {                                           // what a workgroup reports of its query
  int32_t iterations, num_successful, termination, reserved;
  double initial_cost, final_cost, final_radius;
};

struct QbaArgs {
  const int64_t* offsets;
  const int32_t* order;                                   // the queries by descending number of blocks
  const int64_t* obs_patch;
  const double* xyz;
  const double* refs;
  const int32_t* query_camera;
  const int32_t* cam_model;
  const double* cam_params;
  double* qvec;
  double* tvec;
  const void* arena;
  const int32_t* corners;
  const double* scales;
  int H, W;
  int l2_normalize;
  pxr_loss loss;
  pxr_lm_options opt;
  QbaOut* out;
};

__global__ __launch_bounds__(QBA_THREADS) void k_qba_check(int64_t n_obs, const int64_t* __restrict__ obs_patch, int64_t n_patches,
                                                           int* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * QBA_THREADS + threadIdx.x;
  if (i >= n_obs) return;
  if (obs_patch[i] < 0 || obs_patch[i] >= n_patches) atomicOr(flag, 1);
}

// position of H[r][c], r <= c, in the packed upper triangle
__device__ __forceinline__ constexpr int qba_tri(int r, int c) { return r * QBA_D - r * (r - 1) / 2 + (c - r); }

// The 28 sums of a query at the pose x = (q, t) (in LDS, like the intrinsics k) into sh_tot.  Every lane of the workgroup calls it.
// A lane group beyond the query's last block of a pass evaluates that last block again and adds nothing: the control flow around
// the barriers stays uniform.
template <typename ST, int C, bool FLOAT_SIMD>
__device__ __forceinline__ void qba_evaluate(const QbaArgs& a, int64_t o0, int n, int model, const double* sh_k, const double* sh_x,
                                             double* sh_acc, double* sh_tot) {
  constexpr int LPO = C / 8, G = QBA_THREADS / LPO;
  const int tid = threadIdx.x, grp = tid / LPO, sub = tid & (LPO - 1);
  for (int i = tid; i < G * QBA_NS; i += QBA_THREADS) sh_acc[i] = 0.0;
  __syncthreads();
  const size_t patch_elems = (size_t)a.H * a.W * C;
  const ST* arena = reinterpret_cast<const ST*>(a.arena);
  for (int j0 = 0; j0 < n; j0 += G) {
    const bool mine = j0 + grp < n;
    const int64_t o = o0 + (mine ? j0 + grp : n - 1);
    const int64_t pidx = a.obs_patch[o];
    const double X[3] = {a.xyz[3 * o], a.xyz[3 * o + 1], a.xyz[3 * o + 2]};
    double x, y;
    world_to_pixel(model, sh_k, sh_x, sh_x + 4, X, x, y);
    // FeaturePatch::ToPixelCoordinates, featurepatch.h:250-255 (upsampling_factor_ = 1)
    const double sx = a.scales[2 * pidx], sy = a.scales[2 * pidx + 1];
    const double u = x * sx - 0.5 - (double)a.corners[2 * pidx];
    const double v = y * sy - 0.5 - (double)a.corners[2 * pidx + 1];
    double s = 0, gcc = 0, gcr = 0, grr = 0, bc = 0, br = 0;
    {
      double f[8], fr[8], fc[8];
      interp8<ST, LPO, true, FLOAT_SIMD>(arena + (size_t)pidx * patch_elems, a.H, a.W, C, sub, u, v, a.l2_normalize != 0, f, fr, fc);
      const double2* refp = reinterpret_cast<const double2*>(a.refs + (size_t)o * C + sub * 8);
      const double2 rf0 = refp[0], rf1 = refp[1], rf2 = refp[2], rf3 = refp[3];
      const double ref[8] = {rf0.x, rf0.y, rf1.x, rf1.y, rf2.x, rf2.y, rf3.x, rf3.y};
#pragma unroll
      for (int ch = 0; ch < 8; ++ch) {
        const double r = f[ch] - ref[ch];
        s = fma(r, r, s);
        gcc = fma(fc[ch], fc[ch], gcc);
        gcr = fma(fc[ch], fr[ch], gcr);
        grr = fma(fr[ch], fr[ch], grr);
        bc = fma(fc[ch], r, bc);
        br = fma(fr[ch], r, br);
      }
    }
    if (LPO == 16) { s = row16_sum(s); gcc = row16_sum(gcc); gcr = row16_sum(gcr); grr = row16_sum(grr); bc = row16_sum(bc); br = row16_sum(br); }
    else { s = row8_sum(s); gcc = row8_sum(gcc); gcr = row8_sum(gcr); grr = row8_sum(grr); bc = row8_sum(bc); br = row8_sum(br); }
    // Jet bridge: d/dx = dfdc * sx, d/dy = dfdr * sy (interpolation.h:130-140 + featurepatch.h:250-255)
    gcc *= sx * sx; gcr *= sx * sy; grr *= sy * sy; bc *= sx; br *= sy;
    // (check_bounds: with a reference descriptor the functor succeeds wherever the projection lands, feature_reference.h:132-136)

    // P = d(x, y) / d(rotation tangent, t): the ambient quaternion columns through QuaternionManifold::PlusJacobian, dp/dt = I
    double P[2][QBA_D];
    bool ok;
    {
      double xj, yj, A[2][3], Pq[2][4], PX[2][3], Pk[2][PXR_KPAD];
      ok = world_to_pixel_jac(model, sh_k, sh_x, sh_x + 4, X, xj, yj, A, Pq, PX, Pk);
      const double q0 = sh_x[0], q1 = sh_x[1], q2 = sh_x[2], q3 = sh_x[3];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        P[i][0] = -Pq[i][0] * q1 + Pq[i][1] * q0 - Pq[i][2] * q3 + Pq[i][3] * q2;
        P[i][1] = -Pq[i][0] * q2 + Pq[i][1] * q3 + Pq[i][2] * q0 - Pq[i][3] * q1;
        P[i][2] = -Pq[i][0] * q3 - Pq[i][1] * q2 + Pq[i][2] * q1 + Pq[i][3] * q0;
        P[i][3] = A[i][0]; P[i][4] = A[i][1]; P[i][5] = A[i][2];
      }
    }
    if (!ok) s = quiet_nan();                             // a camera model without a projection: the cost is not finite
    if (mine && sub == 0) {
      double rho[3];
      loss_eval(a.loss.type, a.loss.a, 1.0, s, rho);
      const double kappa = loss_corrector_kappa(s, rho);
      double Jr[QBA_D], M[2][QBA_D];
#pragma unroll
      for (int c = 0; c < QBA_D; ++c) {
        Jr[c] = P[0][c] * bc + P[1][c] * br;
        M[0][c] = gcc * P[0][c] + gcr * P[1][c];
        M[1][c] = gcr * P[0][c] + grr * P[1][c];
      }
      double* acc = sh_acc + grp * QBA_NS;
#pragma unroll
      for (int r = 0; r < QBA_D; ++r) {
#pragma unroll
        for (int c = r; c < QBA_D; ++c)
          acc[qba_tri(r, c)] += rho[1] * ((P[0][r] * M[0][c] + P[1][r] * M[1][c]) - kappa * (Jr[r] * Jr[c]));
        acc[QBA_H + r] += rho[1] * Jr[r];
      }
      acc[QBA_H + QBA_D] += 0.5 * rho[0];
    }
  }
  __syncthreads();
  if (tid < QBA_NS) {
    double t = 0.0;
    for (int g = 0; g < G; ++g) t += sh_acc[g * QBA_NS + tid];
    sh_tot[tid] = t;
  }
  __syncthreads();
}

// (H + diag / radius) step = -g by Cholesky on the scaled system `cur` (packed H, g); also the model's cost change
// -step.g - step.H.step / 2.  false: not positive definite, a step that is not finite, or a model that does not decrease
__device__ __forceinline__ bool qba_step(const double* cur, const double* diag, double radius, double step[QBA_D], double& model_cost_change) {
  double Hm[QBA_D][QBA_D], L[QBA_D][QBA_D];
#pragma unroll
  for (int r = 0; r < QBA_D; ++r)
#pragma unroll
    for (int c = r; c < QBA_D; ++c) { Hm[r][c] = cur[qba_tri(r, c)]; Hm[c][r] = Hm[r][c]; }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < QBA_D; ++j) {
    double d = Hm[j][j] + diag[j] / radius;
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    ok = ok && d > 0.0 && isfinite(d);
    d = sqrt(d);
    L[j][j] = d;
#pragma unroll
    for (int i = j + 1; i < QBA_D; ++i) {
      double s = Hm[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
      L[i][j] = s / d;
    }
  }
#pragma unroll
  for (int i = 0; i < QBA_D; ++i) {
    double s = -cur[QBA_H + i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= L[i][k] * step[k];
    step[i] = s / L[i][i];
  }
#pragma unroll
  for (int i = QBA_D - 1; i >= 0; --i) {
    double s = step[i];
#pragma unroll
    for (int k = i + 1; k < QBA_D; ++k) s -= L[k][i] * step[k];
    step[i] = s / L[i][i];
  }
  double dg = 0.0, dHd = 0.0;
#pragma unroll
  for (int r = 0; r < QBA_D; ++r) {
    dg += step[r] * cur[QBA_H + r];
    double hr = 0.0;
#pragma unroll
    for (int c = 0; c < QBA_D; ++c) hr += Hm[r][c] * step[c];
    dHd += step[r] * hr;
    ok = ok && isfinite(step[r]);
  }
  model_cost_change = -dg - 0.5 * dHd;
  return ok && model_cost_change > 0.0;
}

template <typename ST, int C, bool FLOAT_SIMD>
__global__ __launch_bounds__(QBA_THREADS) void k_query_ba(const QbaArgs a) {
  constexpr int G = QBA_THREADS / (C / 8);
  __shared__ double sh_acc[G * QBA_NS];                   // per lane group: its blocks' sums at the pose being evaluated
  __shared__ double sh_tot[QBA_NS];                       // their sum: the unscaled system and the cost at that pose
  __shared__ double sh_cur[QBA_NS];                       // the Jacobi-scaled system at the current pose
  __shared__ double sh_k[PXR_KPAD], sh_x[8], sh_x1[8], sh_scale[QBA_D], sh_diag[QBA_D];
  const int tid = threadIdx.x;
  const int32_t qi = a.order[blockIdx.x];
  const int64_t o0 = a.offsets[qi];
  const int n = (int)(a.offsets[qi + 1] - o0);
  const pxr_lm_options& opt = a.opt;
  QbaOut out;
  out.iterations = 0; out.num_successful = 0; out.termination = PXR_TERM_CONVERGENCE; out.reserved = 0;
  out.initial_cost = 0.0; out.final_cost = 0.0; out.final_radius = opt.initial_radius;
  if (n == 0) {                                           // nothing to refine: the pose stays
    if (tid == 0) a.out[qi] = out;
    return;
  }
  const int32_t cam = a.query_camera[qi];
  const int model = a.cam_model[cam];
  if (tid < PXR_KPAD) sh_k[tid] = a.cam_params[(size_t)cam * PXR_KPAD + tid];
  if (tid == 0) {                                         // AddImageToProblem normalises the quaternion (bundle_optimizer.h:255)
    const double* q = a.qvec + 4 * (size_t)qi;
    const double q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
    const double nn = sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
    sh_x[0] = q0 / nn; sh_x[1] = q1 / nn; sh_x[2] = q2 / nn; sh_x[3] = q3 / nn;
#pragma unroll
    for (int j = 0; j < 3; ++j) sh_x[4 + j] = a.tvec[3 * (size_t)qi + j];
  }
  __syncthreads();
  qba_evaluate<ST, C, FLOAT_SIMD>(a, o0, n, model, sh_k, sh_x, sh_acc, sh_tot);
  double cost = sh_tot[QBA_H + QBA_D];
  out.initial_cost = cost; out.final_cost = cost;
  if (!isfinite(cost)) {                                  // like Ceres when the initial evaluation fails: the pose stays
    out.termination = PXR_TERM_FAILURE;
    if (tid == 0) a.out[qi] = out;
    return;
  }
  if (tid < QBA_D) sh_scale[tid] = opt.jacobi_scaling ? 1.0 / (1.0 + sqrt(sh_tot[qba_tri(tid, tid)])) : 1.0;
  __syncthreads();
  // sh_cur = S H S, S g of the sums in sh_tot, S = the Jacobi scaling fixed at the initial linearisation
  auto scale_system = [&]() {
    if (tid < QBA_NS) {
      double w = 1.0;
      if (tid < QBA_H) {
        int r = 0, first = 0;
        while (tid >= first + (QBA_D - r)) { first += QBA_D - r; ++r; }
        w = sh_scale[r] * sh_scale[r + (tid - first)];
      } else if (tid < QBA_H + QBA_D) {
        w = sh_scale[tid - QBA_H];
      }
      sh_cur[tid] = tid < QBA_H + QBA_D ? sh_tot[tid] * w : sh_tot[tid];
    }
    __syncthreads();
  };
  scale_system();

  double radius = opt.initial_radius, decrease_factor = 2.0;
  int invalid = 0;
  bool reuse_diag = false;
  out.termination = PXR_TERM_NO_CONVERGENCE;
  while (true) {
    if (out.iterations >= opt.max_iterations) { out.termination = PXR_TERM_NO_CONVERGENCE; break; }
    if (radius < opt.min_radius) { out.termination = PXR_TERM_CONVERGENCE; break; }
    ++out.iterations;
    __syncthreads();                                      // every lane has read what this iteration overwrites (sh_x1, sh_diag)
    // LevenbergMarquardtStrategy::ComputeStep
    if (!reuse_diag) {
      if (tid < QBA_D) sh_diag[tid] = fmin(fmax(sh_cur[qba_tri(tid, tid)], opt.min_lm_diagonal), opt.max_lm_diagonal);
      __syncthreads();
    }
    double step[QBA_D], model_cost_change;
    if (!qba_step(sh_cur, sh_diag, radius, step, model_cost_change)) {   // HandleInvalidStep
      if (++invalid >= opt.max_consecutive_invalid_steps) { out.termination = PXR_TERM_FAILURE; break; }
      radius *= 0.5; reuse_diag = true;
      continue;
    }
    invalid = 0;
    if (tid == 0) {
      double delta[QBA_D], q1[4];
#pragma unroll
      for (int j = 0; j < QBA_D; ++j) delta[j] = step[j] * sh_scale[j];
      quat_plus(sh_x, delta, q1);
#pragma unroll
      for (int j = 0; j < 4; ++j) sh_x1[j] = q1[j];
#pragma unroll
      for (int j = 0; j < 3; ++j) sh_x1[4 + j] = sh_x[4 + j] + delta[3 + j];
    }
    __syncthreads();
    qba_evaluate<ST, C, FLOAT_SIMD>(a, o0, n, model, sh_k, sh_x1, sh_acc, sh_tot);
    const double cand = sh_tot[QBA_H + QBA_D];
    double step2 = 0.0, x2 = 0.0;
#pragma unroll
    for (int j = 0; j < 7; ++j) { const double d = sh_x[j] - sh_x1[j]; step2 += d * d; x2 += sh_x[j] * sh_x[j]; }
    if (sqrt(step2) <= opt.parameter_tolerance * (sqrt(x2) + opt.parameter_tolerance)) { out.termination = PXR_TERM_CONVERGENCE; break; }
    const double cost_change = cost - cand;
    if (fabs(cost_change) <= opt.function_tolerance * cost) { out.termination = PXR_TERM_CONVERGENCE; break; }
    const double rel = cost_change / model_cost_change;
    if (rel > opt.min_relative_decrease) {                // IsStepSuccessful + HandleSuccessfulStep
      double gmax = 0.0;
#pragma unroll
      for (int j = 0; j < QBA_D; ++j) gmax = fmax(gmax, fabs(sh_tot[QBA_H + j]));
      __syncthreads();                                    // every lane has read sh_x and sh_x1
      if (tid < 7) sh_x[tid] = sh_x1[tid];
      scale_system();
      cost = cand;
      ++out.num_successful;
      const double tmp = 2.0 * rel - 1.0;
      radius = fmin(radius / fmax(1.0 / 3.0, 1.0 - tmp * tmp * tmp), opt.max_radius);
      decrease_factor = 2.0; reuse_diag = false;
      if (gmax <= opt.gradient_tolerance) { out.termination = PXR_TERM_CONVERGENCE; break; }
    } else {                                              // StepRejected
      radius /= decrease_factor; decrease_factor *= 2.0; reuse_diag = true;
    }
  }
  out.final_cost = cost; out.final_radius = radius;
  if (tid == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) a.qvec[4 * (size_t)qi + j] = sh_x[j];
#pragma unroll
    for (int j = 0; j < 3; ++j) a.tvec[3 * (size_t)qi + j] = sh_x[4 + j];
    a.out[qi] = out;
  }
}

static int query_ba_solve(pxr_ctx* ctx, pxr_arena* arena, int32_t n_queries, const int64_t* d_query_offsets, int64_t n_obs,
                          const int64_t* d_obs_patch, const double* d_xyz, const double* d_refs, const int32_t* d_query_camera,
                          int32_t n_cameras, const int32_t* d_cam_model, const double* d_cam_params, double* d_qvec, double* d_tvec,
                          const pxr_interp_cfg* cfg, const pxr_loss* loss, const pxr_lm_options* opt, pxr_lm_summary* h_summaries,
                          double* h_ms) {
  const char* fn = "pxr_query_ba_solve";
  PXR_REQUIRE(ctx && arena && cfg && loss && opt, "%s: NULL argument", fn);
  PXR_REQUIRE(n_queries >= 0 && n_obs >= 0 && n_cameras >= 0, "%s: negative size", fn);
  PXR_REQUIRE(n_obs < ((int64_t)1 << 31), "%s: more than 2^31 residual blocks", fn);
  PXR_REQUIRE(n_queries == 0 || (d_query_offsets && d_query_camera && d_cam_model && d_cam_params && d_qvec && d_tvec && h_summaries),
              "%s: NULL query / camera array", fn);
  PXR_REQUIRE(n_obs == 0 || (d_obs_patch && d_xyz && d_refs), "%s: NULL residual-block array", fn);
  PXR_REQUIRE(arena->up == 1.0, "%s: an upsampling factor is a property of cost maps", fn);
  PXR_REQUIRE(opt->max_iterations >= 0 && opt->initial_radius > 0.0, "%s: option out of range", fn);
  const bool supported = (arena->dtype == PXR_F16 || arena->dtype == PXR_F32 || arena->dtype == PXR_F64) && (arena->C == 128 || arena->C == 64);
  if (!supported)
    return set_error(PXR_EUNSUPPORTED, "%s: storage type %d with CHANNELS=%d not supported (fp16 / fp32 / fp64 with 128 or 64)", fn, arena->dtype,
                     arena->C);
  if (h_ms) h_ms[0] = 0.0;
  if (n_queries == 0) {
    PXR_REQUIRE(n_obs == 0, "%s: query_offsets ends at 0, not at n_obs = %lld", fn, (long long)n_obs);
    return PXR_OK;
  }
  PXR_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int64_t T = n_queries;

  // offsets and cameras are validated on host copies; the offsets also give the processing order (the longest queries first)
  std::vector<int64_t> off;
  std::vector<int32_t> order, qcam((size_t)T);
  PXR_HIP(hipMemcpyAsync(qcam.data(), d_query_camera, sizeof(int32_t) * (size_t)T, hipMemcpyDeviceToHost, st));
  const auto camera_in_range = [&](int64_t t) {
    PXR_REQUIRE(qcam[t] >= 0 && qcam[t] < n_cameras, "%s: query %lld names a camera outside [0, n_cameras = %d)", fn, (long long)t, (int)n_cameras);
    return (int)PXR_OK;
  };
  if (int rc = batch_order(ctx, {fn, "query_offsets", "query", "n_obs"}, false, d_query_offsets, T, n_obs, off, order, camera_in_range)) return rc;

  int* flag; int32_t* d_order; QbaOut* d_out;
  Workspace ws;
  ws.take(flag, 4); ws.take(d_order, (size_t)T); ws.take(d_out, (size_t)T);
  if (int rc = ws.commit(ctx)) return rc;
  double ms = 0.0;
  StageTimer<2> timer(st, &ms);
  if (int rc = timer.create(fn)) return rc;

  // patch indices are checked on the device; the flag is back before the solve starts
  int h_flag = 0;
  int rc = hip_check(hipMemsetAsync(flag, 0, 16, st), "hipMemsetAsync");
  if (rc == PXR_OK) rc = hip_check(hipMemcpyAsync(d_order, order.data(), sizeof(int32_t) * (size_t)T, hipMemcpyHostToDevice, st), "hipMemcpyAsync");
  if (rc == PXR_OK) {
    if (n_obs > 0) hipLaunchKernelGGL(k_qba_check, blocks_for(n_obs, QBA_THREADS), dim3(QBA_THREADS), 0, st, n_obs, d_obs_patch, arena->n, flag);
    rc = hip_check(hipMemcpyAsync(&h_flag, flag, 4, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
  }
  if (rc == PXR_OK) rc = hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");      // (also: `order` may go out of scope)
  if (rc != PXR_OK) return rc;
  if (h_flag) return set_error(PXR_EINVAL, "%s: obs_patch names a patch outside the arena's %lld", fn, (long long)arena->n);

  QbaArgs a;
  a.offsets = d_query_offsets; a.order = d_order; a.obs_patch = d_obs_patch; a.xyz = d_xyz; a.refs = d_refs;
  a.query_camera = d_query_camera; a.cam_model = d_cam_model; a.cam_params = d_cam_params; a.qvec = d_qvec; a.tvec = d_tvec;
  set_arena(a, arena);
  a.l2_normalize = cfg->l2_normalize; a.loss = *loss; a.opt = *opt; a.out = d_out;
  timer.mark(0);
  for_storage<_Float16, float, double>(arena->dtype, [&](auto s) {
    using ST = typename decltype(s)::type;
    for_channels<128, 64>(arena->C, [&](auto c) {
      for_flag(cfg->use_float_simd != 0, [&](auto fs) {
        hipLaunchKernelGGL((k_query_ba<ST, decltype(c)::value, decltype(fs)::value>), dim3((unsigned)T), dim3(QBA_THREADS), 0, st, a);
      });
    });
  });
  timer.mark(1);
  rc = hip_check(hipGetLastError(), "k_query_ba launch");
  std::vector<QbaOut> out((size_t)T);
  if (rc == PXR_OK) rc = hip_check(hipMemcpyAsync(out.data(), d_out, sizeof(QbaOut) * (size_t)T, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
  const int from[1] = {0};
  if (rc == PXR_OK) rc = timer.read(from, 1);             // synchronises the stream
  if (rc != PXR_OK) return rc;
  for (int64_t t = 0; t < T; ++t) {
    pxr_lm_summary s = {};
    s.iterations = out[t].iterations; s.num_successful = out[t].num_successful; s.termination = out[t].termination;
    s.num_camera_unknowns = QBA_D; s.num_point_unknowns = 0;
    s.initial_cost = out[t].initial_cost; s.final_cost = out[t].final_cost; s.final_radius = out[t].final_radius;
    s.total_ms = ms; s.accumulation = 2;
    h_summaries[t] = s;
  }
  if (h_ms) h_ms[0] = ms;
  return PXR_OK;
}

}  // namespace pxr

extern "C" int pxr_query_ba_solve(pxr_ctx* ctx, pxr_arena* arena, int32_t n_queries, const int64_t* d_query_offsets, int64_t n_obs,
                                  const int64_t* d_obs_patch, const double* d_xyz, const double* d_refs, const int32_t* d_query_camera,
                                  int32_t n_cameras, const int32_t* d_cam_model, const double* d_cam_params, double* d_qvec,
                                  double* d_tvec, const pxr_interp_cfg* cfg, const pxr_loss* loss, const pxr_lm_options* options,
                                  pxr_lm_summary* h_summaries) {
  return pxr::query_ba_solve(ctx, arena, n_queries, d_query_offsets, n_obs, d_obs_patch, d_xyz, d_refs, d_query_camera, n_cameras,
                             d_cam_model, d_cam_params, d_qvec, d_tvec, cfg, loss, options, h_summaries, nullptr);
}

extern "C" int pxr_query_ba_solve_timed(pxr_ctx* ctx, pxr_arena* arena, int32_t n_queries, const int64_t* d_query_offsets, int64_t n_obs,
                                        const int64_t* d_obs_patch, const double* d_xyz, const double* d_refs,
                                        const int32_t* d_query_camera, int32_t n_cameras, const int32_t* d_cam_model,
                                        const double* d_cam_params, double* d_qvec, double* d_tvec, const pxr_interp_cfg* cfg,
                                        const pxr_loss* loss, const pxr_lm_options* options, pxr_lm_summary* h_summaries,
                                        double* h_kernel_ms) {
  PXR_REQUIRE(h_kernel_ms, "pxr_query_ba_solve_timed: NULL h_kernel_ms");
  return pxr::query_ba_solve(ctx, arena, n_queries, d_query_offsets, n_obs, d_obs_patch, d_xyz, d_refs, d_query_camera, n_cameras,
                             d_cam_model, d_cam_params, d_qvec, d_tvec, cfg, loss, options, h_summaries, h_kernel_ms);
}
