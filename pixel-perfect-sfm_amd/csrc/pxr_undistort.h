// pxr_undistort.h -- the inverse camera model, pixel -> normalised image coordinates, for the eleven COLMAP 3.8 models
// ([upstream COLMAP 3.8 camera_models.h] <Model>::ImageToWorld).  COLMAP undistorts each model with its own fixed-count
// iteration (IterativeUndistortion: Newton on a finite-difference Jacobian, 100 steps); here ONE Newton iteration on
//     world_to_image(u, v) - (x, y) = 0
// with the models' ANALYTIC 2 x 2 Jacobian d(x,y)/d(u,v) serves all of them: the hand-derived Juv of camera_model_jac for the
// five common models, forward-mode duals over (u, v) alone for the six fisheye / full-OpenCV / FOV models (the same formulas
// and the same partials camera_model_jac<false, true> returns, without the twelve d/dk partials it would carry along).
#pragma once
#include "pxr_device.h"

namespace pxr {

constexpr int PXR_UNDISTORT_MAX_ITERS = 32;
constexpr double PXR_UNDISTORT_STEP2 = 1e-20;   // converged once the squared Newton step falls below

// value and d(x,y)/d(u,v) of any of the eleven models at (u, v)
__device__ __forceinline__ bool camera_model_juv(int model, const double* __restrict__ k, double u, double v, double& x,
                                                 double& y, double Juv[2][2]) {
  if (model <= PXR_OPENCV) return camera_model_jac<false, false>(model, k, u, v, x, y, Juv, nullptr);
  typedef Dual<2> D;
  D kd[PXR_KPAD];
#pragma unroll
  for (int i = 0; i < PXR_KPAD; ++i) kd[i] = D(k[i]);
  D ud(u), vd(v), xd, yd;
  ud.v[0] = 1.0; vd.v[1] = 1.0;
  if (!world_to_image_ext<D>(model, kd, ud, vd, xd, yd)) return false;
  x = xd.a; y = yd.a;
  Juv[0][0] = xd.v[0]; Juv[0][1] = xd.v[1]; Juv[1][0] = yd.v[0]; Juv[1][1] = yd.v[1];
  return true;
}

// ImageToWorld: the normalised image point (u, v) whose projection is the pixel (x, y).  false (u = v = NaN): unknown model,
// singular Jacobian, non-finite iterate, or no convergence within PXR_UNDISTORT_MAX_ITERS steps.
__device__ __forceinline__ bool image_to_world(int model, const double* __restrict__ k, double x, double y, double& u, double& v) {
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  double fx, fy, cx, cy;
  switch (model) {
    case PXR_SIMPLE_PINHOLE: case PXR_SIMPLE_RADIAL: case PXR_RADIAL: case PXR_SIMPLE_RADIAL_FISHEYE: case PXR_RADIAL_FISHEYE:
      fx = fy = k[0]; cx = k[1]; cy = k[2];
      break;
    case PXR_PINHOLE: case PXR_OPENCV: case PXR_OPENCV_FISHEYE: case PXR_FULL_OPENCV: case PXR_FOV: case PXR_THIN_PRISM_FISHEYE:
      fx = k[0]; fy = k[1]; cx = k[2]; cy = k[3];
      break;
    default:
      u = v = nan;
      return false;
  }
  u = (x - cx) / fx; v = (y - cy) / fy;                     // the pinholes: closed form; the others: the starting point
  bool ok = model <= PXR_PINHOLE;
  if (!ok) {
    for (int it = 0; it < PXR_UNDISTORT_MAX_ITERS; ++it) {
      double px, py, J[2][2];
      if (!camera_model_juv(model, k, u, v, px, py, J)) break;
      const double rx = px - x, ry = py - y;
      const double det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
      if (!(fabs(det) > 0.0) || !isfinite(det)) break;       // singular (or NaN)
      const double du = (J[1][1] * rx - J[0][1] * ry) / det, dv = (J[0][0] * ry - J[1][0] * rx) / det;
      u -= du; v -= dv;
      const double step2 = du * du + dv * dv;
      if (!isfinite(step2)) break;
      if (step2 < PXR_UNDISTORT_STEP2) { ok = true; break; }
    }
  }
  ok = ok && isfinite(u) && isfinite(v);
  if (!ok) u = v = nan;
  return ok;
}

}  // namespace pxr
