// pxr_abspose.hip -- batched absolute pose estimation on gfx950: 2D-3D correspondences of many query images -> one pose each.
//
// Replaces pycolmap.absolute_pose_estimation as the reference's QueryLocalizer calls it (pixsfm/localization/main.py:458) for
// the geometry it does: undistort every pixel ([upstream COLMAP 3.8] <Model>::ImageToWorld), estimate a pose robustly from
// minimal samples (P3P), refine it on its inliers.  The estimator is NOT COLMAP's LO-RANSAC: it has no random state -- sample h
// of a query is a counter-based hash of (seed, h) -- and every choice is a comparison of keys, so the result is a function of
// the query's own correspondences alone, bit for bit, alone or inside any batch.
//
//   k_abs_bearings   one lane per correspondence: its query (binary search of the offsets), undistort -> record (u, v, X, Y, Z), usable
//   k_compact_records<5>  (pxr_robust.h) one lane per query: the usable records of a query moved to the front of its slice (in
//                    order), positions kept
//   k_abs_hypotheses the estimator's samples: one workgroup of 256 lanes per query, the first ABS_LDS_CORR records staged in LDS;
//                    a round of samples per wavefront, a sample per lane, every lane scoring its own poses against all records
//   k_abs_refine     the winner's local optimisation and the final classification, the same mapping of queries to workgroups
//
// P3P: Grunert's solution (1841; Haralick, Lee, Ottenberg, Noelle, "Review and analysis of solutions of the three point
// perspective pose estimation problem", IJCV 1994, section 2): with unit bearings f_i, distances s_i, s_2 = u s_1, s_3 = v s_1
// the law of cosines gives u = N(v) / D(v) and one quartic in v, whose coefficients are formed here as polynomial products
// N^2 - 2 cos(gamma) N D + D^2 M; real roots by Ferrari's factorisation into two quadratics, polished by Newton on the quartic.
// Where the quartic's constant coefficient outweighs its leading one the quartic of 1 / v is solved instead (a leading coefficient
// near zero is a root near infinity, which costs Ferrari's shift the other three).  Of two roots that nearly coincide while D(v)
// nearly vanishes -- N / D tends to 0 / 0, as in front of a triangle of equal sides -- u comes from the law of cosines, one of its
// two roots for each.  The three distances are then polished by Newton on the three cosine-law equations themselves, which are
// well conditioned where the quartic is not.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "pxr_batch.h"
#include "pxr_device.h"
#include "pxr_internal.h"
#include "pxr_robust.h"
#include "pxr_undistort.h"

namespace pxr {

constexpr int ABS_THREADS = 256;
constexpr int ABS_WAVES = ABS_THREADS / 64;
constexpr int ABS_REC = 5;                             // doubles per record: u, v (normalised image point), X, Y, Z
constexpr int ABS_LDS_CORR = PXR_ABSPOSE_LDS_CORR;     // records of a query staged in LDS (40 B each); the rest is read from global memory (L2)
constexpr int ABS_ACC = 28;                            // the refinement's sums: H (21, upper triangle by rows), g (6), cost
constexpr int ABS_CHUNK = 7;                           // of which this many cross the workgroup at a time (ABS_THREADS x ABS_CHUNK doubles of LDS)
constexpr int ABS_NEWTON = 3;                          // Newton steps on every quartic root
constexpr int ABS_DISTANCE_NEWTON = 3;                 // Newton steps on the three cosine-law equations in the distances
constexpr double ABS_LEAD_TOL = 1e-12;                 // the quartic's leading coefficient counts as zero below this fraction of the sum of magnitudes
constexpr double ABS_DISC_TOL = 1e-7;                  // a quadratic factor's discriminant counts as zero down to minus this fraction of its terms
constexpr double ABS_PAIR_TOL = 1e-3;                  // two roots are a close pair within this fraction of their size
constexpr double ABS_SMALL_D = 1e-3;                   // of a close pair, u is not N / D where |D(v)| is below this fraction of its terms
constexpr double ABS_STEP_TOL = 1e-12;                 // the refinement stops at a step of this norm
constexpr double ABS_COST_SLACK = 1e-12;               // a step is kept unless the cost grows by more than this fraction: below it the
                                                       // comparison is rounding noise, and refusing would stall short of the minimum

// ---- P3P -------------------------------------------------------------------------------------------------------------------------
struct P3P {
  double f1[3], f2[3], f3[3], P1[3], w1[3], w2[3], w3[3];   // unit bearings; first point; orthonormal triad of the three points
  double a2, b2, c2, cb, cg, ha, hb, hg, N0, N1, N2, D0, D1;   // squared sides; cos beta, cos gamma; 1 - cos of the three angles
  double v0, v1, v2, v3;                                    // the roots (NaN: none), of the quartic in 1 / v where rev
  bool rev;
};

__device__ __forceinline__ void abs_bearing(const double* r, double f[3]) {
  const double inv = 1.0 / sqrt(r[0] * r[0] + r[1] * r[1] + 1.0);
  f[0] = r[0] * inv; f[1] = r[1] * inv; f[2] = inv;
}
// Newton on the monic quartic; a step is kept only where it does not raise |f|: at a double root f' vanishes with f, and an unguarded
// step can land anywhere
__device__ __forceinline__ double abs_polish(double v, double B, double C, double D, double E) {
  double fv = (((v + B) * v + C) * v + D) * v + E;
#pragma unroll
  for (int it = 0; it < ABS_NEWTON; ++it) {
    const double dv = ((4.0 * v + 3.0 * B) * v + 2.0 * C) * v + D;
    if (dv == 0.0) break;
    const double vn = v - fv / dv;
    const double fn = (((vn + B) * vn + C) * vn + D) * vn + E;
    if (!(fabs(fn) <= fabs(fv))) break;
    v = vn; fv = fn;
  }
  return v;
}

// false: a degenerate sample (coincident or collinear points, no quartic, no positive resolvent root) -- zero poses
__device__ __forceinline__ bool p3p_setup(const double* r1, const double* r2, const double* r3, P3P& s) {
  abs_bearing(r1, s.f1); abs_bearing(r2, s.f2); abs_bearing(r3, s.f3);
  double e1[3], e2[3], e3[3], cr[3];
#pragma unroll
  for (int m = 0; m < 3; ++m) { s.P1[m] = r1[2 + m]; e1[m] = r2[2 + m] - r1[2 + m]; e2[m] = r3[2 + m] - r1[2 + m]; e3[m] = r3[2 + m] - r2[2 + m]; }
  const double c2 = dot3(e1, e1), b2 = dot3(e2, e2), a2 = dot3(e3, e3);
  cross3(e1, e2, cr);
  const double cr2 = dot3(cr, cr);
  s.v0 = s.v1 = s.v2 = s.v3 = quiet_nan();
  if (!(cr2 > 1e-12 * c2 * b2) || !isfinite(cr2)) return false;
  const double ic = 1.0 / sqrt(c2), icr = 1.0 / sqrt(cr2);
#pragma unroll
  for (int m = 0; m < 3; ++m) { s.w1[m] = e1[m] * ic; s.w3[m] = cr[m] * icr; }
  cross3(s.w3, s.w1, s.w2);
  const double ca = dot3(s.f2, s.f3), cb = dot3(s.f1, s.f3), cg = dot3(s.f1, s.f2);
  const double k1 = (a2 - c2) / b2, k2 = c2 / b2;
  const double N0 = k1 + 1.0, N1 = -2.0 * k1 * cb, N2 = k1 - 1.0, D0 = 2.0 * cg, D1 = -2.0 * ca;
  const double M0 = 1.0 - k2, M1 = 2.0 * k2 * cb, M2 = -k2;
  // 1 - cos = |f_i - f_j|^2 / 2: a narrow field of view has cosines that round away what separates them from 1
  double da[3], db[3], dg[3];
#pragma unroll
  for (int m = 0; m < 3; ++m) { da[m] = s.f2[m] - s.f3[m]; db[m] = s.f1[m] - s.f3[m]; dg[m] = s.f1[m] - s.f2[m]; }
  s.ha = 0.5 * dot3(da, da); s.hb = 0.5 * dot3(db, db); s.hg = 0.5 * dot3(dg, dg);
  s.a2 = a2; s.b2 = b2; s.c2 = c2; s.cb = cb; s.cg = cg; s.N0 = N0; s.N1 = N1; s.N2 = N2; s.D0 = D0; s.D1 = D1;
  // N^2 - 2 cg N D + D^2 M, ascending powers of v
  double A0 = N0 * N0 - 2.0 * cg * (N0 * D0) + D0 * D0 * M0;
  double A1 = 2.0 * N0 * N1 - 2.0 * cg * (N0 * D1 + N1 * D0) + (D0 * D0 * M1 + 2.0 * D0 * D1 * M0);
  const double A2 = (N1 * N1 + 2.0 * N0 * N2) - 2.0 * cg * (N1 * D1 + N2 * D0) + (D0 * D0 * M2 + 2.0 * D0 * D1 * M1 + D1 * D1 * M0);
  double A3 = 2.0 * N1 * N2 - 2.0 * cg * (N2 * D1) + (2.0 * D0 * D1 * M2 + D1 * D1 * M1);
  double A4 = N2 * N2 + D1 * D1 * M2;
  const double scale = fabs(A0) + fabs(A1) + fabs(A2) + fabs(A3) + fabs(A4);
  s.rev = fabs(A0) > fabs(A4);                          // the quartic of 1 / v: the same coefficients in reverse
  if (s.rev) { double x = A0; A0 = A4; A4 = x; x = A1; A1 = A3; A3 = x; }
  if (!(fabs(A4) > ABS_LEAD_TOL * scale) || !isfinite(scale)) return false;
  const double B = A3 / A4, C = A2 / A4, D = A1 / A4, E = A0 / A4;
  // Ferrari: v = y - B / 4, y^4 + p y^2 + q y + r = 0; m = the largest real root of m^3 + p m^2 + (p^2 / 4 - r) m - q^2 / 8
  const double B2 = B * B;
  const double p = C - 0.375 * B2, q = D - 0.5 * B * C + 0.125 * B2 * B;
  const double r = E - 0.25 * B * D + 0.0625 * B2 * C - (3.0 / 256.0) * B2 * B2;
  const double c1 = 0.25 * p * p - r, c0 = -0.125 * q * q;
  const double Q = (p * p - 3.0 * c1) / 9.0, R = (2.0 * p * p * p - 9.0 * p * c1 + 27.0 * c0) / 54.0;
  const double Q3 = Q * Q * Q;
  double m;
  if (R * R < Q3) {
    const double th = acos(R / sqrt(Q3));
    m = -2.0 * sqrt(Q) * cos((th + 6.283185307179586) / 3.0) - p / 3.0;
  } else {
    const double A = -copysign(cbrt(fabs(R) + sqrt(R * R - Q3)), R);
    m = A + (A != 0.0 ? Q / A : 0.0) - p / 3.0;
  }
#pragma unroll
  for (int it = 0; it < 2; ++it) {                      // Newton on the cubic
    const double fm = ((m + p) * m + c1) * m + c0, dm = (3.0 * m + 2.0 * p) * m + c1;
    if (dm != 0.0) m -= fm / dm;
  }
  if (!(m > 0.0) || !isfinite(m)) return false;
  const double sq = sqrt(2.0 * m), tq = q / (2.0 * sq);
  if (!isfinite(tq)) return false;
  const double d1 = -2.0 * m - 2.0 * p - 4.0 * tq, d2 = -2.0 * m - 2.0 * p + 4.0 * tq, off = 0.25 * B;
  const double low = -ABS_DISC_TOL * (2.0 * m + 2.0 * fabs(p) + 4.0 * fabs(tq));   // a double root's discriminant may round below zero
  if (d1 >= low) {
    const double sd = sqrt(fmax(d1, 0.0));
    s.v0 = abs_polish(0.5 * (sq + sd) - off, B, C, D, E); s.v1 = abs_polish(0.5 * (sq - sd) - off, B, C, D, E);
  }
  if (d2 >= low) {
    const double sd = sqrt(fmax(d2, 0.0));
    s.v2 = abs_polish(0.5 * (-sq + sd) - off, B, C, D, E); s.v3 = abs_polish(0.5 * (-sq - sd) - off, B, C, D, E);
  }
  return true;
}

__device__ __forceinline__ double p3p_root(const P3P& s, int root) { return root == 0 ? s.v0 : root == 1 ? s.v1 : root == 2 ? s.v2 : s.v3; }

// the pose (row-major R, t: camera = R world + t) of root `root`; false: no root, or a distance that is not positive
__device__ __forceinline__ bool p3p_pose(const P3P& s, int root, double R[9], double t[3]) {
  double v = p3p_root(s, root);
  if (!(v > 0.0) || !isfinite(v)) return false;
  int twin = -1;                                        // the first other root within ABS_PAIR_TOL of this one
#pragma unroll
  for (int j = 3; j >= 0; --j)
    if (j != root && fabs(p3p_root(s, j) - v) <= ABS_PAIR_TOL * v) twin = j;
  if (s.rev) v = 1.0 / v;
  const double g = 1.0 + v * (v - 2.0 * s.cb);
  const double den = s.D0 + s.D1 * v;
  double u;
  if (twin < 0 || fabs(den) > ABS_SMALL_D * (fabs(s.D0) + fabs(s.D1 * v))) {
    u = (s.N0 + (s.N1 + s.N2 * v) * v) / den;
  } else {                                              // N / D tends to 0 / 0: both roots of the cosine law in u are solutions
    const double h = sqrt(fmax(s.cg * s.cg - 1.0 + (s.c2 / s.b2) * g, 0.0));
    u = root < twin ? s.cg + h : s.cg - h;
  }
  if (!(u > 0.0) || !isfinite(u) || !(g > 0.0)) return false;
  double s1 = sqrt(s.b2 / g), s2 = u * s1, s3 = v * s1;
#pragma unroll
  for (int it = 0; it < ABS_DISTANCE_NEWTON; ++it) {    // Newton on (s_i - s_j)^2 + 2 s_i s_j (1 - cos) = side^2, each 3 x 3 system by Cramer's rule
    const double d23 = s2 - s3, d13 = s1 - s3, d12 = s1 - s2;
    const double F1 = d23 * d23 + 2.0 * s2 * s3 * s.ha - s.a2;
    const double F2 = d13 * d13 + 2.0 * s1 * s3 * s.hb - s.b2;
    const double F3 = d12 * d12 + 2.0 * s1 * s2 * s.hg - s.c2;
    const double j12 = 2.0 * (d23 + s3 * s.ha), j13 = 2.0 * (s2 * s.ha - d23);
    const double j21 = 2.0 * (d13 + s3 * s.hb), j23 = 2.0 * (s1 * s.hb - d13);
    const double j31 = 2.0 * (d12 + s2 * s.hg), j32 = 2.0 * (s1 * s.hg - d12);
    const double det = j12 * j23 * j31 + j13 * j21 * j32;
    const double d1 = (j12 * j23 * F3 + j13 * j32 * F2 - j23 * j32 * F1) / det;
    const double d2 = (j23 * j31 * F1 + j13 * j21 * F3 - j13 * j31 * F2) / det;
    const double d3 = (j12 * j31 * F2 + j21 * j32 * F1 - j12 * j21 * F3) / det;
    if (det != 0.0 && isfinite(d1) && isfinite(d2) && isfinite(d3)) { s1 -= d1; s2 -= d2; s3 -= d3; }
  }
  if (!(s1 > 0.0 && s2 > 0.0 && s3 > 0.0)) return false;
  double Q1[3], g1[3], g2[3], cr[3], c1[3], c2[3], c3[3];
#pragma unroll
  for (int m = 0; m < 3; ++m) { Q1[m] = s1 * s.f1[m]; g1[m] = s2 * s.f2[m] - Q1[m]; g2[m] = s3 * s.f3[m] - Q1[m]; }
  cross3(g1, g2, cr);
  const double n1 = sqrt(dot3(g1, g1)), n3 = sqrt(dot3(cr, cr));
  if (!(n1 > 0.0) || !(n3 > 0.0)) return false;
#pragma unroll
  for (int m = 0; m < 3; ++m) { c1[m] = g1[m] / n1; c3[m] = cr[m] / n3; }
  cross3(c3, c1, c2);
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) R[3 * i + j] = c1[i] * s.w1[j] + c2[i] * s.w2[j] + c3[i] * s.w3[j];
    t[i] = Q1[i] - (R[3 * i] * s.P1[0] + R[3 * i + 1] * s.P1[1] + R[3 * i + 2] * s.P1[2]);
    ok = ok && isfinite(t[i]);
  }
  return ok;
}

// ---- kernel A: records -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ABS_THREADS) void k_abs_bearings(int64_t n_corr, int32_t n_queries, const int64_t* __restrict__ offsets,
                                                              const int32_t* __restrict__ query_camera, const int32_t* __restrict__ cam_model,
                                                              const double* __restrict__ cam_params, const double* __restrict__ xy,
                                                              const double* __restrict__ xyz, double* __restrict__ rec,
                                                              uint8_t* __restrict__ valid, uint8_t* __restrict__ inlier, double* __restrict__ err) {
  const int64_t i = (int64_t)blockIdx.x * ABS_THREADS + threadIdx.x;
  if (i >= n_corr) return;
  int lo = 0, hi = n_queries;                          // the query q with offsets[q] <= i < offsets[q + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) / 2;
    if (offsets[mid] <= i) lo = mid; else hi = mid;
  }
  const int cam = query_camera[lo];
  double k[PXR_KPAD];
#pragma unroll
  for (int j = 0; j < PXR_KPAD; ++j) k[j] = cam_params[(size_t)cam * PXR_KPAD + j];
  const double x = xy[2 * i], y = xy[2 * i + 1], X = xyz[3 * i], Y = xyz[3 * i + 1], Z = xyz[3 * i + 2];
  double u, v;
  bool ok = isfinite(x) && isfinite(y) && isfinite(X) && isfinite(Y) && isfinite(Z);
  ok = image_to_world(cam_model[cam], k, x, y, u, v) && ok;
  double* r = rec + (size_t)i * ABS_REC;
  r[0] = u; r[1] = v; r[2] = X; r[3] = Y; r[4] = Z;
  valid[i] = ok ? 1 : 0;
  inlier[i] = 0;                                       // what a correspondence keeps unless its query gets a pose
  err[i] = quiet_nan();
}

// ---- kernel B: the estimator -------------------------------------------------------------------------------------------------------
struct AbsArgs {
  const int64_t* offsets; const int32_t* query_camera; const int32_t* cam_model; const double* cam_params; const double* xy;
  const int32_t* order;        // [n_queries] queries by descending correspondence count
  const double* rec;           // [n_corr][ABS_REC], compacted per query
  const int32_t* pos;          // [n_corr]
  const int32_t* n_valid;      // [n_queries]
  int32_t* winner;             // [n_queries][3] the best key: count (-1: none), sample, root
  uint8_t* mask_a; uint8_t* mask_b;                   // [n_corr] each: inlier sets of the local optimisation (by compacted position)
  pxr_abspose_options o;
  int32_t max_trials;          // o.max_num_trials rounded up to a multiple of o.round_size
  double* qvec; double* tvec; int32_t* status; int32_t* n_inliers; int32_t* n_trials; uint8_t* inlier; double* err;
};

struct AbsQuery {              // what every lane of the workgroup knows about its query
  const double* sh; const double* g; int n; int64_t o0;
  int model; double k[PXR_KPAD];
  __device__ __forceinline__ const double* rec(int j) const { return j < ABS_LDS_CORR ? sh + j * ABS_REC : g + (size_t)j * ABS_REC; }
};

// pixel error of compacted record j under (q, t): NaN behind the camera or where the model fails
__device__ __forceinline__ double abs_pixel_err(const AbsArgs& a, const AbsQuery& Q, int j, const double* q, const double* t) {
  const double* r = Q.rec(j);
  const double X[3] = {r[2], r[3], r[4]};
  double p[3], x, y;
  rotate_translate(q, t, X, p);
  if (!(p[2] > 0.0)) return quiet_nan();
  if (!world_to_image(Q.model, Q.k, p[0] / p[2], p[1] / p[2], x, y)) return quiet_nan();
  const int64_t i = Q.o0 + a.pos[Q.o0 + j];
  const double ex = x - a.xy[2 * i], ey = y - a.xy[2 * i + 1];
  return sqrt(ex * ex + ey * ey);
}

// H = sum w J^t J, g = sum w J^t r, cost = sum rho(|r|^2) over the records of `mask`, w = rho'(|r|^2), J = d r / d (rotation tangent, t).
// The projection is world_to_pixel_jac's (pxr_device.h) without its point and intrinsics blocks (camera_model_jac<false>), and with
// the rotation block taken in the tangent of abs_pose_plus directly: p(d) = R(2 d) R X + t, so dp / dd_c = 2 e_c x (R X).
__device__ __forceinline__ void abs_normal_equations(const AbsArgs& a, const AbsQuery& Q, const uint8_t* mask, const double* q,
                                                     const double* t, double (&acc)[ABS_ACC], double* sh_part, double* sh_tot) {
#pragma unroll
  for (int c = 0; c < ABS_ACC; ++c) acc[c] = 0.0;
  double R[9];
  quat_to_rotation(q, R);
  for (int j = threadIdx.x; j < Q.n; j += ABS_THREADS) {
    if (!mask[Q.o0 + j]) continue;
    const double* r = Q.rec(j);
    const double pr[3] = {R[0] * r[2] + R[1] * r[3] + R[2] * r[4], R[3] * r[2] + R[4] * r[3] + R[5] * r[4],
                          R[6] * r[2] + R[7] * r[3] + R[8] * r[4]};
    const double p[3] = {pr[0] + t[0], pr[1] + t[1], pr[2] + t[2]};
    double x, y, Juv[2][2];
    const double iz = 1.0 / p[2];
    if (!(p[2] > 0.0) || !camera_model_jac<false, true>(Q.model, Q.k, p[0] * iz, p[1] * iz, x, y, Juv, nullptr)) {
      acc[27] = pos_inf();
      continue;
    }
    const int64_t i = Q.o0 + a.pos[Q.o0 + j];
    const double res[2] = {x - a.xy[2 * i], y - a.xy[2 * i + 1]};
    double rho[3];
    loss_eval(PXR_LOSS_CAUCHY, a.o.refine_loss_scale, 1.0, res[0] * res[0] + res[1] * res[1], rho);
    double J[2][6];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const double A0 = Juv[m][0] * iz, A1 = Juv[m][1] * iz, A2 = -(Juv[m][0] * p[0] + Juv[m][1] * p[1]) * iz * iz;   // d(x, y) / dp
      J[m][0] = 2.0 * (A2 * pr[1] - A1 * pr[2]);
      J[m][1] = 2.0 * (A0 * pr[2] - A2 * pr[0]);
      J[m][2] = 2.0 * (A1 * pr[0] - A0 * pr[1]);
      J[m][3] = A0; J[m][4] = A1; J[m][5] = A2;
    }
    int c = 0;
#pragma unroll
    for (int m = 0; m < 6; ++m) {
#pragma unroll
      for (int l = m; l < 6; ++l) { acc[c] += rho[1] * (J[0][m] * J[0][l] + J[1][m] * J[1][l]); ++c; }
      acc[21 + m] += rho[1] * (J[0][m] * res[0] + J[1][m] * res[1]);
    }
    acc[27] += rho[0];
  }
  block_sum<ABS_THREADS, ABS_CHUNK>(acc, sh_part, sh_tot);
}

// x (+) d as the bundle adjustment moves a pose: QuaternionManifold::Plus [upstream Ceres manifold.cc] on q, t + d; q re-normalised
__device__ __forceinline__ void abs_pose_plus(const double* q0, const double* t0, const double* d, double q1[4], double t1[3]) {
  quat_plus(q0, d, q1);
#pragma unroll
  for (int j = 0; j < 3; ++j) t1[j] = t0[j] + d[3 + j];
}

// Levenberg-Marquardt on the records of `mask`, (q, t) refined in place.  Every lane holds the same sums, so every lane takes
// the same decisions and ends with the same pose.
__device__ __forceinline__ void abs_refine(const AbsArgs& a, const AbsQuery& Q, const uint8_t* mask, double q[4], double t[3],
                                           double* sh_part, double* sh_tot, double* sh_cur) {
  // sh_cur: the sums at (q, t), the same on every lane, parked in LDS while the trial's are formed
  double acc[ABS_ACC];
  abs_normal_equations(a, Q, mask, q, t, acc, sh_part, sh_tot);
  if (!isfinite(acc[27])) return;
  double lambda = 1e-4;
  for (int it = 0; it < a.o.refine_max_iterations; ++it) {
    double d[6], q1[4], t1[3];
    if (!solve_damped<6>(acc, lambda, d)) {
      lambda *= 10.0;
      if (lambda > 1e12) break;
      continue;
    }
    if (threadIdx.x < ABS_ACC) {
#pragma unroll
      for (int c = 0; c < ABS_ACC; ++c) if (threadIdx.x == c) sh_cur[c] = acc[c];
    }
    const double cost = acc[27];
    abs_pose_plus(q, t, d, q1, t1);
    abs_normal_equations(a, Q, mask, q1, t1, acc, sh_part, sh_tot);     // (its barriers publish sh_cur)
    if (acc[27] <= cost + ABS_COST_SLACK * cost) {
#pragma unroll
      for (int j = 0; j < 4; ++j) q[j] = q1[j];
#pragma unroll
      for (int j = 0; j < 3; ++j) t[j] = t1[j];
      lambda = fmax(lambda * 0.1, 1e-12);
    } else {
#pragma unroll
      for (int c = 0; c < ABS_ACC; ++c) acc[c] = sh_cur[c];
      lambda *= 10.0;
      if (lambda > 1e12) break;
    }
    if (sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3] + d[4] * d[4] + d[5] * d[5]) <= ABS_STEP_TOL) break;
  }
}

// what every lane of a workgroup needs of its query; false: fewer than four usable correspondences
__device__ __forceinline__ bool abs_open_query(const AbsArgs& a, int qi, double* sh_rec, AbsQuery& Q, double& thr2) {
  Q.o0 = a.offsets[qi];
  Q.n = a.n_valid[qi];
  if (Q.n < 4) return false;
  Q.g = a.rec + (size_t)Q.o0 * ABS_REC;
  Q.sh = sh_rec;
  for (int x = threadIdx.x; x < min(Q.n, ABS_LDS_CORR) * ABS_REC; x += ABS_THREADS) sh_rec[x] = Q.g[x];
  const int cam = a.query_camera[qi];
  Q.model = a.cam_model[cam];
#pragma unroll
  for (int j = 0; j < PXR_KPAD; ++j) Q.k[j] = a.cam_params[(size_t)cam * PXR_KPAD + j];
  const double thr = a.o.max_error / mean_focal(Q.model, Q.k);
  thr2 = thr * thr;
  __syncthreads();
  return true;
}

// Every branch that encloses a barrier or a cross-lane operation is uniform over the workgroup; the hypothesis loop, where the
// lanes meet different root counts, has none.
__global__ __launch_bounds__(ABS_THREADS) void k_abs_hypotheses(const AbsArgs a) {
  __shared__ double sh_rec[ABS_LDS_CORR * ABS_REC];
  __shared__ double sh_ksum[ABS_WAVES];
  __shared__ int sh_kint[ABS_WAVES][3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qi = a.order[blockIdx.x];
  AbsQuery Q;
  double thr2;
  if (!abs_open_query(a, qi, sh_rec, Q, thr2)) {
    if (tid == 0) { a.status[qi] = 1; a.n_inliers[qi] = 0; a.n_trials[qi] = 0; }
    return;
  }
  const int n = Q.n;

  // 1. hypotheses: round r (round_size samples) on wavefront r mod 4, its samples strided over the lanes
  HypKey best = {-1, 0.0, 0x7fffffff, 4};
  int done = 0;
  const auto need = [&](int cnt) {                       // the stop rule: three inliers in a sample
    const double w = (double)cnt / (double)n;
    return trials_needed(a.o.confidence, a.o.min_num_trials, a.max_trials, cnt, w * w * w);
  };
  for (int pass = 0;; ++pass) {
    const int round = pass * ABS_WAVES + wave;
    HypKey mine = {-1, 0.0, 0x7fffffff, 4};
    if ((int64_t)round * a.o.round_size < a.max_trials) {
      for (int s = lane; s < a.o.round_size; s += 64) {
        const int h = round * a.o.round_size + s;
        int i[3];
        sample_distinct<3>(a.o.seed, h, n, i);
        P3P p3;
        if (!p3p_setup(Q.rec(i[0]), Q.rec(i[1]), Q.rec(i[2]), p3)) continue;
        for (int root = 0; root < 4; ++root) {
          double R[9], t[3];
          if (!p3p_pose(p3, root, R, t)) continue;
          int cnt = 0;
          double sum = 0.0;
          for (int j = 0; j < n; ++j) {
            const double* r = Q.rec(j);
            const double pz = R[6] * r[2] + R[7] * r[3] + R[8] * r[4] + t[2];
            double e = thr2;
            if (pz > 0.0) {
              const double iz = 1.0 / pz;
              const double du = r[0] - (R[0] * r[2] + R[1] * r[3] + R[2] * r[4] + t[0]) * iz;
              const double dv = r[1] - (R[3] * r[2] + R[4] * r[3] + R[5] * r[4] + t[1]) * iz;
              const double e2 = du * du + dv * dv;
              if (e2 <= thr2) { ++cnt; e = e2; }
            }
            sum += e;
          }
          const HypKey key = {cnt, sum, h, root};
          if (key.beats(mine)) mine = key;
        }
      }
    }
    wave_best(mine);
    if (merge_rounds<ABS_WAVES>(sh_ksum, sh_kint, mine, pass, a.o.round_size, a.max_trials, best, done, need)) break;
  }
  if (tid == 0) {
    a.n_trials[qi] = done;
    a.winner[3 * (size_t)qi] = best.cnt; a.winner[3 * (size_t)qi + 1] = best.h; a.winner[3 * (size_t)qi + 2] = best.root;
    if (best.cnt < 0) { a.status[qi] = 2; a.n_inliers[qi] = 0; }
  }
}

// The second half of the estimator, in a kernel of its own: the refinement's registers (the camera models' derivatives) do not
// weigh on the occupancy of the hypothesis loop.
__global__ __launch_bounds__(ABS_THREADS) void k_abs_refine(const AbsArgs a) {
  __shared__ double sh_rec[ABS_LDS_CORR * ABS_REC];
  __shared__ double sh_part[ABS_THREADS * ABS_CHUNK];
  __shared__ double sh_tot[ABS_ACC];
  __shared__ double sh_cur[ABS_ACC];
  const int tid = threadIdx.x;
  const int qi = a.order[blockIdx.x];
  HypKey best;
  best.cnt = a.winner[3 * (size_t)qi]; best.h = a.winner[3 * (size_t)qi + 1]; best.root = a.winner[3 * (size_t)qi + 2]; best.sum = 0.0;
  AbsQuery Q;
  double thr2;
  if (!abs_open_query(a, qi, sh_rec, Q, thr2) || best.cnt < 0) return;      // status 1 or 2: written by k_abs_hypotheses
  const int n = Q.n;

  // 2. the winner's pose (its own arithmetic again, on every lane) and its inliers in the normalised image plane
  double q[4], t[3];
  {
    int i[3];
    sample_distinct<3>(a.o.seed, best.h, n, i);
    P3P p3;
    double R[9];
    p3p_setup(Q.rec(i[0]), Q.rec(i[1]), Q.rec(i[2]), p3);
    p3p_pose(p3, best.root, R, t);
    rotation_to_quat(R, q);
    for (int j = tid; j < n; j += ABS_THREADS) {
      const double* r = Q.rec(j);
      const double pz = R[6] * r[2] + R[7] * r[3] + R[8] * r[4] + t[2];
      bool in = false;
      if (pz > 0.0) {
        const double iz = 1.0 / pz;
        const double du = r[0] - (R[0] * r[2] + R[1] * r[3] + R[2] * r[4] + t[0]) * iz;
        const double dv = r[1] - (R[3] * r[2] + R[4] * r[3] + R[5] * r[4] + t[1]) * iz;
        in = du * du + dv * dv <= thr2;
      }
      a.mask_a[Q.o0 + j] = in ? 1 : 0;                  // (a lane reads back only what it wrote: j = tid mod 256)
    }
  }

  // 3. local optimisation: refine on the inliers, classify again by pixel error, until the set stands still
  uint8_t* cur = a.mask_a;
  uint8_t* nxt = a.mask_b;
  int cur_cnt = best.cnt;
  for (int lo = 0; lo < a.o.lo_rounds; ++lo) {
    double q1[4], t1[3];
#pragma unroll
    for (int j = 0; j < 4; ++j) q1[j] = q[j];
#pragma unroll
    for (int j = 0; j < 3; ++j) t1[j] = t[j];
    abs_refine(a, Q, cur, q1, t1, sh_part, sh_tot, sh_cur);
    double cc[2] = {0.0, 0.0};                          // inliers of the refined pose; how many memberships changed
    for (int j = tid; j < n; j += ABS_THREADS) {
      const bool in = abs_pixel_err(a, Q, j, q1, t1) <= a.o.max_error;
      nxt[Q.o0 + j] = in ? 1 : 0;
      cc[0] += in ? 1.0 : 0.0;
      cc[1] += (in != (cur[Q.o0 + j] != 0)) ? 1.0 : 0.0;
    }
    block_sum<ABS_THREADS, ABS_CHUNK>(cc, sh_part, sh_tot);
    if (cc[0] < (double)cur_cnt) break;                 // fewer inliers: the pose before it stays
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = q1[j];
#pragma unroll
    for (int j = 0; j < 3; ++j) t[j] = t1[j];
    uint8_t* sw = cur; cur = nxt; nxt = sw;
    cur_cnt = (int)cc[0];
    if (cc[1] == 0.0) break;
  }

  // 4. the final set: pixel error <= max_error under the pose that stays
  double fin[1] = {0.0};
  for (int j = tid; j < n; j += ABS_THREADS) fin[0] += abs_pixel_err(a, Q, j, q, t) <= a.o.max_error ? 1.0 : 0.0;
  block_sum<ABS_THREADS, ABS_CHUNK>(fin, sh_part, sh_tot);
  const int n_in = (int)fin[0];
  const int need = max(a.o.min_num_inliers, (int)ceil(a.o.min_inlier_ratio * (double)n));
  if (n_in < need) {
    if (tid == 0) { a.status[qi] = 3; a.n_inliers[qi] = 0; }
    return;
  }
  for (int j = tid; j < n; j += ABS_THREADS) {
    const double e = abs_pixel_err(a, Q, j, q, t);
    const int64_t i = Q.o0 + a.pos[Q.o0 + j];
    a.err[i] = e;
    a.inlier[i] = e <= a.o.max_error ? 1 : 0;
  }
  if (tid == 0) {
    const double sgn = q[0] < 0.0 ? -1.0 : 1.0;
    for (int j = 0; j < 4; ++j) a.qvec[4 * (size_t)qi + j] = sgn * q[j];
    for (int j = 0; j < 3; ++j) a.tvec[3 * (size_t)qi + j] = t[j];
    a.status[qi] = 0; a.n_inliers[qi] = n_in;
  }
}

static int absolute_pose(pxr_ctx* ctx, int32_t n_queries, const int64_t* d_query_offsets, int64_t n_corr, const double* d_xy,
                         const double* d_xyz, const int32_t* d_query_camera, int32_t n_cameras, const int32_t* d_cam_model,
                         const double* d_cam_params, const pxr_abspose_options* o, double* d_qvec, double* d_tvec, int32_t* d_status,
                         int32_t* d_n_inliers, int32_t* d_n_trials, uint8_t* d_inlier, double* d_err, double* h_ms) {
  const char* fn = "pxr_absolute_pose";
  PXR_REQUIRE(ctx && o, "%s: NULL argument", fn);
  PXR_REQUIRE(n_queries >= 0 && n_corr >= 0 && n_cameras >= 0, "%s: negative size", fn);
  PXR_REQUIRE(n_corr < ((int64_t)1 << 31), "%s: more than 2^31 correspondences", fn);
  PXR_REQUIRE(n_queries == 0 || (d_query_offsets && d_query_camera && d_qvec && d_tvec && d_status && d_n_inliers && d_n_trials &&
                                 d_cam_model && d_cam_params), "%s: NULL query / camera array", fn);
  PXR_REQUIRE(n_corr == 0 || (d_xy && d_xyz && d_inlier && d_err), "%s: NULL correspondence array", fn);
  PXR_REQUIRE(o->max_error > 0.0 && o->confidence > 0.0 && o->confidence < 1.0 && o->min_inlier_ratio >= 0.0 && o->min_inlier_ratio <= 1.0 &&
                  o->min_num_inliers >= 0 && o->min_num_trials >= 0 && o->max_num_trials >= 1 && o->max_num_trials <= (1 << 20) &&
                  o->round_size >= 1 && o->round_size <= (1 << 20) && o->refine_max_iterations >= 0 && o->refine_loss_scale > 0.0 &&
                  o->lo_rounds >= 0, "%s: option out of range", fn);
  if (h_ms) h_ms[0] = h_ms[1] = h_ms[2] = h_ms[3] = 0.0;
  if (n_queries == 0) {
    PXR_REQUIRE(n_corr == 0, "%s: query_offsets ends at 0, not at n_corr = %lld", fn, (long long)n_corr);
    return PXR_OK;
  }
  PXR_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int64_t T = n_queries, N = n_corr;

  // offsets and cameras are validated on a host copy, which also gives the processing order: queries by descending
  // correspondence count (a stable counting sort), so that the longest start first
  std::vector<int64_t> off;
  std::vector<int32_t> order, qcam((size_t)T);
  PXR_HIP(hipMemcpyAsync(qcam.data(), d_query_camera, sizeof(int32_t) * (size_t)T, hipMemcpyDeviceToHost, st));
  const auto camera_in_range = [&](int64_t t) {
    PXR_REQUIRE(qcam[t] >= 0 && qcam[t] < n_cameras, "%s: query %lld names a camera outside [0, n_cameras = %d)", fn, (long long)t, (int)n_cameras);
    return (int)PXR_OK;
  };
  if (int rc = batch_order(ctx, {fn, "query_offsets", "query", "n_corr"}, false, d_query_offsets, T, N, off, order, camera_in_range)) return rc;

  AbsArgs a;
  double* rec; uint8_t* valid; int32_t *pos, *n_valid, *d_order;
  Workspace ws;
  ws.take(rec, (size_t)N * ABS_REC); ws.take(valid, (size_t)N); ws.take(pos, (size_t)N);
  ws.take(a.mask_a, (size_t)N); ws.take(a.mask_b, (size_t)N); ws.take(n_valid, (size_t)T); ws.take(d_order, (size_t)T); ws.take(a.winner, (size_t)T * 3);
  if (int rc = ws.commit(ctx)) return rc;

  StageTimer<5> timer(st, h_ms);                         // bearings | compact | hypotheses | refine
  if (int rc = timer.create(fn)) return rc;

  int rc = hip_check(hipMemcpyAsync(d_order, order.data(), sizeof(int32_t) * (size_t)T, hipMemcpyHostToDevice, st), "hipMemcpyAsync");
  if (rc == PXR_OK) rc = hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");      // (`order` may go out of scope)
  if (rc != PXR_OK) return rc;
  timer.mark(0);
  if (N > 0)
    hipLaunchKernelGGL(k_abs_bearings, blocks_for(N, ABS_THREADS), dim3(ABS_THREADS), 0, st, N, n_queries, d_query_offsets, d_query_camera,
                       d_cam_model, d_cam_params, d_xy, d_xyz, rec, valid, d_inlier, d_err);
  timer.mark(1);
  hipLaunchKernelGGL(k_compact_records<ABS_REC>, blocks_for(T, ABS_THREADS), dim3(ABS_THREADS), 0, st, T, d_query_offsets, rec, valid, pos, n_valid);
  timer.mark(2);
  a.offsets = d_query_offsets; a.query_camera = d_query_camera; a.cam_model = d_cam_model; a.cam_params = d_cam_params; a.xy = d_xy;
  a.order = d_order; a.rec = rec; a.pos = pos; a.n_valid = n_valid;
  a.o = *o;
  a.max_trials = (int32_t)(((int64_t)o->max_num_trials + o->round_size - 1) / o->round_size * o->round_size);
  a.qvec = d_qvec; a.tvec = d_tvec; a.status = d_status; a.n_inliers = d_n_inliers; a.n_trials = d_n_trials; a.inlier = d_inlier; a.err = d_err;
  hipLaunchKernelGGL(k_abs_hypotheses, dim3((unsigned)T), dim3(ABS_THREADS), 0, st, a);
  timer.mark(3);
  hipLaunchKernelGGL(k_abs_refine, dim3((unsigned)T), dim3(ABS_THREADS), 0, st, a);
  timer.mark(4);
  rc = hip_check(hipGetLastError(), "k_abs_refine launch");
  const int from[4] = {0, 1, 2, 3};
  return rc == PXR_OK ? timer.read(from, 4) : rc;
}

}  // namespace pxr

extern "C" void pxr_abspose_default_options(pxr_abspose_options* o) {
  if (!o) return;
  o->max_error = 12.0; o->min_inlier_ratio = 0.01; o->confidence = 0.99999; o->refine_loss_scale = 1.0;
  o->seed = 0; o->min_num_inliers = 4; o->min_num_trials = 64; o->max_num_trials = 4096; o->round_size = 64;
  o->refine_max_iterations = 100; o->lo_rounds = 4;
}

extern "C" int pxr_absolute_pose(pxr_ctx* ctx, int32_t n_queries, const int64_t* d_query_offsets, int64_t n_corr, const double* d_xy,
                                 const double* d_xyz, const int32_t* d_query_camera, int32_t n_cameras, const int32_t* d_cam_model,
                                 const double* d_cam_params, const pxr_abspose_options* options, double* d_qvec, double* d_tvec,
                                 int32_t* d_status, int32_t* d_n_inliers, int32_t* d_n_trials, uint8_t* d_inlier, double* d_err) {
  return pxr::absolute_pose(ctx, n_queries, d_query_offsets, n_corr, d_xy, d_xyz, d_query_camera, n_cameras, d_cam_model, d_cam_params,
                            options, d_qvec, d_tvec, d_status, d_n_inliers, d_n_trials, d_inlier, d_err, nullptr);
}

extern "C" int pxr_absolute_pose_timed(pxr_ctx* ctx, int32_t n_queries, const int64_t* d_query_offsets, int64_t n_corr, const double* d_xy,
                                       const double* d_xyz, const int32_t* d_query_camera, int32_t n_cameras, const int32_t* d_cam_model,
                                       const double* d_cam_params, const pxr_abspose_options* options, double* d_qvec, double* d_tvec,
                                       int32_t* d_status, int32_t* d_n_inliers, int32_t* d_n_trials, uint8_t* d_inlier, double* d_err,
                                       double* h_kernel_ms) {
  PXR_REQUIRE(h_kernel_ms, "pxr_absolute_pose_timed: NULL h_kernel_ms");
  return pxr::absolute_pose(ctx, n_queries, d_query_offsets, n_corr, d_xy, d_xyz, d_query_camera, n_cameras, d_cam_model, d_cam_params,
                            options, d_qvec, d_tvec, d_status, d_n_inliers, d_n_trials, d_inlier, d_err, h_kernel_ms);
}
