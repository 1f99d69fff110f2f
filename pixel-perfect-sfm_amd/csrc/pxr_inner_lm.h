// pxr_inner_lm.h -- the nested per-point trust-region LM of Ceres' inner iterations as a device template over the
// evaluation, and the robustifier's corrector.  Device-side helpers; not part of the C-ABI.
//
// [upstream Ceres 2.1 coordinate_descent_minimizer.cc -> trust_region_minimizer.cc with default options]: <= 50 iterations,
// function / gradient / parameter tolerance 1e-6 / 1e-10 / 1e-8, initial radius 1e4 (max 1e16, min 1e-32), Jacobi scaling,
// LM diagonal clamped to [1e-6, 1e32], min_relative_decrease 1e-3, <= 5 consecutive invalid steps.  The same loop, statement
// for statement, as the one written out in pxr_ba_inner.hip (inner_points_body), which keeps its own copy: the featuremetric
// kernels are tuned around their register budget and are not rebuilt on top of this header.
#pragma once
#include <hip/hip_runtime.h>

namespace pxr {

// [upstream Ceres corrector.cc]: J~^T J~ = rho' (J^T J - kappa (J^T r)(J^T r)^T), s = |r|^2, rho = (rho, rho', rho'')
__device__ __forceinline__ double loss_corrector_kappa(double s, const double rho[3]) {
  if (!(s != 0.0 && rho[2] > 0.0)) return 0.0;
  const double D = 1.0 + 2.0 * s * rho[2] / rho[1];
  const double alpha = 1.0 - sqrt(D);
  return (2.0 * alpha - alpha * alpha) / s;
}

// Step of the damped, Jacobi-scaled 3 x 3 system (H + diag / radius) st = -g by Cholesky; H = (xx xy xz yy yz zz).
// Returns false when the matrix is not positive definite.
__device__ __forceinline__ bool damped_step3(const double H[6], const double g[3], const double diag[3], double radius, double st[3]) {
  const double a00 = H[0] + diag[0] / radius, a01 = H[1], a02 = H[2], a11 = H[3] + diag[1] / radius, a12 = H[4],
               a22 = H[5] + diag[2] / radius;
  bool ok = a00 > 0.0;
  const double l00 = sqrt(a00), l10 = a01 / l00, l20 = a02 / l00;
  const double d1 = a11 - l10 * l10;
  ok = ok && d1 > 0.0;
  const double l11 = sqrt(d1), l21 = (a12 - l20 * l10) / l11;
  const double d2 = a22 - l20 * l20 - l21 * l21;
  ok = ok && d2 > 0.0;
  const double l22 = sqrt(d2);
  const double y0 = -g[0] / l00, y1 = (-g[1] - l10 * y0) / l11, y2 = (-g[2] - l20 * y0 - l21 * y1) / l22;
  st[2] = y2 / l22; st[1] = (y1 - l21 * st[2]) / l11; st[0] = (y0 - l10 * st[1] - l20 * st[2]) / l00;
  return ok;
}

// Refine the point X in place.  cost, H, g: the evaluation at X (unscaled); eval(Xc, with_jac, Hc, gc) -> cost at Xc, and the
// normal equations there when with_jac.  Every lane that cooperates in `eval` calls this with the same values.
// Returns false when the gradient at X is already below tolerance (X untouched).
template <typename Eval>
__device__ __forceinline__ bool nested_point_lm(double X[3], double cost, double H[6], double g[3], Eval&& eval) {
  double gmax = fmax(fabs(g[0]), fmax(fabs(g[1]), fabs(g[2])));
  if (gmax <= 1e-10) return false;
  const double sc[3] = {1.0 / (1.0 + sqrt(H[0])), 1.0 / (1.0 + sqrt(H[3])), 1.0 / (1.0 + sqrt(H[5]))};
  auto scale_sys = [&]() {
    H[0] *= sc[0] * sc[0]; H[1] *= sc[0] * sc[1]; H[2] *= sc[0] * sc[2];
    H[3] *= sc[1] * sc[1]; H[4] *= sc[1] * sc[2]; H[5] *= sc[2] * sc[2];
    g[0] *= sc[0]; g[1] *= sc[1]; g[2] *= sc[2];
  };
  scale_sys();
  double radius = 1e4, decrease_factor = 2.0, diag[3] = {0, 0, 0};
  int invalid = 0;
  bool reuse_diag = false;
  for (int it = 0; it < 50; ++it) {
    if (radius < 1e-32) break;
    if (!reuse_diag) {
      diag[0] = fmin(fmax(H[0], 1e-6), 1e32); diag[1] = fmin(fmax(H[3], 1e-6), 1e32); diag[2] = fmin(fmax(H[5], 1e-6), 1e32);
    }
    double st[3];
    bool ok = damped_step3(H, g, diag, radius, st);
    double mcc = 0.0;
    if (ok) {
      const double dg = st[0] * g[0] + st[1] * g[1] + st[2] * g[2];
      const double dHd = st[0] * (H[0] * st[0] + H[1] * st[1] + H[2] * st[2]) + st[1] * (H[1] * st[0] + H[3] * st[1] + H[4] * st[2]) +
                         st[2] * (H[2] * st[0] + H[4] * st[1] + H[5] * st[2]);
      mcc = -dg - 0.5 * dHd;
      if (!(mcc > 0.0) || !isfinite(st[0]) || !isfinite(st[1]) || !isfinite(st[2])) ok = false;
    }
    if (!ok) {
      if (++invalid >= 5) break;
      radius *= 0.5; reuse_diag = true;
      continue;
    }
    invalid = 0;
    const double Xc[3] = {X[0] + st[0] * sc[0], X[1] + st[1] * sc[1], X[2] + st[2] * sc[2]};
    double Hc[6], gc[3];
    const double cand = eval(Xc, true, Hc, gc);   // with Jacobians: an accepted step needs no second evaluation
    const double s2 = (Xc[0] - X[0]) * (Xc[0] - X[0]) + (Xc[1] - X[1]) * (Xc[1] - X[1]) + (Xc[2] - X[2]) * (Xc[2] - X[2]);
    const double x2 = X[0] * X[0] + X[1] * X[1] + X[2] * X[2];
    if (sqrt(s2) <= 1e-8 * (sqrt(x2) + 1e-8)) break;
    const double cost_change = cost - cand;
    if (fabs(cost_change) <= 1e-6 * cost) break;
    const double rel = cost_change / mcc;
    if (rel > 1e-3) {
      X[0] = Xc[0]; X[1] = Xc[1]; X[2] = Xc[2];
      cost = cand;
#pragma unroll
      for (int j = 0; j < 6; ++j) H[j] = Hc[j];
#pragma unroll
      for (int j = 0; j < 3; ++j) g[j] = gc[j];
      gmax = fmax(fabs(g[0]), fmax(fabs(g[1]), fabs(g[2])));
      scale_sys();
      const double tmp = 2.0 * rel - 1.0;
      radius = fmin(1e16, radius / fmax(1.0 / 3.0, 1.0 - tmp * tmp * tmp));
      decrease_factor = 2.0; reuse_diag = false;
      if (gmax <= 1e-10) break;
    } else {
      radius /= decrease_factor; decrease_factor *= 2.0; reuse_diag = true;
    }
  }
  return true;
}

}  // namespace pxr
