// pxr_fundamental.hip -- batched fundamental-matrix estimation on gfx950: the matches of many image pairs -> one fundamental
// matrix and one inlier mask each.
//
// The uncalibrated half of COLMAP's two-view geometry estimation (pycolmap.verify_matches estimates F next to E, or F alone for a
// camera without a prior focal length): undistort both pixels of every match with the cameras given -- for an uncalibrated pair
// these are conditioning transforms -- estimate a fundamental matrix of the two normalised planes robustly from minimal samples
// (seven points), refine it on its inliers over a parametrisation that is rank 2 by construction.  Records, the opening of a
// pair, the local optimisation and the host side of a call are those of pxr_pairs.h; what is here is the fundamental matrix's own
// (DESIGN.md section 23).
//
//   k_fm_hypotheses  one workgroup of 256 lanes per pair, the first PAIR_LDS records staged in LDS; a round of samples per
//                    wavefront, a sample per lane, every lane scoring its own fundamental matrices (one per real root of the
//                    cubic, one at a time) against all records
//   k_fm_refine      the winner's local optimisation and the final classification
//
// Where the solver's state lives: the 7 x 9 system is a private array indexed by pivot rows and columns, i.e. scratch memory, and
// so is the Sturm chain of the cubic (4 polynomials); the fundamental matrix itself is in registers for the scoring walk (figures:
// DESIGN.md section 23).
#include <hip/hip_runtime.h>

#include <cmath>

#include "pxr_device.h"
#include "pxr_pairs.h"

namespace pxr {

constexpr int FM_ACC = 36;                             // the refinement's sums: J^t J (28, upper triangle by rows), g (7), cost
constexpr int FM_CHUNK = 9;                            // of which this many cross the workgroup at a time (PAIR_THREADS x FM_CHUNK doubles of LDS)
constexpr int FM_DEG = 3;                              // degree of det(x A + B)
constexpr int FM_BISECT = 64;                          // bisection steps per root
constexpr int FM_NEWTON = 4;                           // Newton steps per root, each kept only inside the bisection's last interval
constexpr double FM_PIVOT_TOL = 1e-12;                 // a pivot counts as zero below this fraction of the system's largest entry
constexpr double FM_LEAD_TOL = 1e-9;                   // the leading coefficient counts as zero below this fraction of the largest one
constexpr double FM_TRIM_TOL = 1e-12;                  // so does the leading coefficient of a rescaled Sturm remainder
constexpr double FM_RSQRT2 = 0.70710678118654752440;   // 1 / sqrt 2, rounded to double

// ---- the seven-point solver --------------------------------------------------------------------------------------------------------
struct FmSolver {
  double A[9], B[9];           // F = x A + B, row-major
  double c[FM_DEG + 1];        // det(x A + B), ascending powers, scaled to a largest coefficient of 1
  double chain[FM_DEG + 1][FM_DEG + 1];  // the Sturm chain, ascending powers
  int deg[FM_DEG + 1];
  int n_chain;
  double bound;                // Cauchy's: every real root in (-bound, bound)
  int v_low;                   // sign changes at -bound
  int n_roots;
};

__device__ inline int fm_sign_changes(const FmSolver& s, double x) {
  int changes = 0, prev = 0;
  for (int i = 0; i < s.n_chain; ++i) {
    double v = s.chain[i][s.deg[i]];
    for (int k = s.deg[i] - 1; k >= 0; --k) v = v * x + s.chain[i][k];
    const int sg = (v > 0.0) - (v < 0.0);
    if (sg != 0) {
      if (prev != 0 && sg != prev) ++changes;
      prev = sg;
    }
  }
  return changes;
}

// rec: the records (x1, y1, x2, y2) of a sample.  false: no hypothesis (vanishing pivot or leading coefficient, a value that is
// not finite).
__device__ inline bool fm_solver_setup(const double* const* rec, FmSolver& s) {
  // 1. the null space of the epipolar system x2^t F x1 = 0, F row-major: Gauss-Jordan with full pivoting -> [I | C] in permuted
  //    columns, vector k = (-C[:, k], e_k); orthonormalised (modified Gram-Schmidt, k = 0, 1); mixed into A = (N0 + N1) / sqrt 2
  //    and B = (N0 - N1) / sqrt 2, so that neither null vector being the answer on its own sends a root of det(x A + B) to infinity
  {
    double M[7 * 9];
    int perm[9];
    for (int m = 0; m < 7; ++m) {
      const double u1 = rec[m][0], v1 = rec[m][1], u2 = rec[m][2], v2 = rec[m][3];
      double* a = M + m * 9;
      a[0] = u2 * u1; a[1] = u2 * v1; a[2] = u2; a[3] = v2 * u1; a[4] = v2 * v1; a[5] = v2; a[6] = u1; a[7] = v1; a[8] = 1.0;
    }
    double S = 0.0;
    for (int x = 0; x < 63; ++x) S = fmax(S, fabs(M[x]));
    if (!isfinite(S)) return false;
    for (int k = 0; k < 9; ++k) perm[k] = k;
    for (int c = 0; c < 7; ++c) {
      int pr = c, pc = c;
      double pa = fabs(M[c * 9 + c]);
      for (int r = c; r < 7; ++r)
        for (int k = c; k < 9; ++k) {
          const double v = fabs(M[r * 9 + k]);
          if (v > pa) { pa = v; pr = r; pc = k; }
        }
      if (!(pa > FM_PIVOT_TOL * S)) return false;
      if (pr != c)
        for (int k = 0; k < 9; ++k) { const double v = M[c * 9 + k]; M[c * 9 + k] = M[pr * 9 + k]; M[pr * 9 + k] = v; }
      if (pc != c) {
        for (int r = 0; r < 7; ++r) { const double v = M[r * 9 + c]; M[r * 9 + c] = M[r * 9 + pc]; M[r * 9 + pc] = v; }
        const int v = perm[c]; perm[c] = perm[pc]; perm[pc] = v;
      }
      const double p = M[c * 9 + c];
      for (int k = c; k < 9; ++k) M[c * 9 + k] = M[c * 9 + k] / p;
      for (int r = 0; r < 7; ++r) {
        if (r == c) continue;
        const double f = M[r * 9 + c];
        for (int k = c + 1; k < 9; ++k) M[r * 9 + k] = M[r * 9 + k] - f * M[c * 9 + k];
        M[r * 9 + c] = 0.0;
      }
    }
    double u[2][9];
    for (int k = 0; k < 2; ++k) {
      for (int r = 0; r < 7; ++r) u[k][perm[r]] = -M[r * 9 + 7 + k];
      for (int j = 0; j < 2; ++j) u[k][perm[7 + j]] = j == k ? 1.0 : 0.0;
      for (int j = 0; j < k; ++j) {
        double d = 0.0;
        for (int m = 0; m < 9; ++m) d += u[k][m] * u[j][m];
        for (int m = 0; m < 9; ++m) u[k][m] = u[k][m] - d * u[j][m];
      }
      double d = 0.0;
      for (int m = 0; m < 9; ++m) d += u[k][m] * u[k][m];
      const double nrm = sqrt(d);
      if (!(nrm > 0.0) || !isfinite(nrm)) return false;
      for (int m = 0; m < 9; ++m) u[k][m] = u[k][m] / nrm;
    }
    for (int m = 0; m < 9; ++m) {
      s.A[m] = (u[0][m] + u[1][m]) * FM_RSQRT2;
      s.B[m] = (u[0][m] - u[1][m]) * FM_RSQRT2;
    }
  }
  // 2. det(x A + B) = sum_a (x A[0][a] + B[0][a]) (q2 x^2 + q1 x + q0), the minor of rows 1, 2 and columns b = a + 1, cc = a + 2 (mod 3)
  double c[FM_DEG + 1] = {0.0, 0.0, 0.0, 0.0};
  for (int a = 0; a < 3; ++a) {
    const int b = (a + 1) % 3, cc = (a + 2) % 3;
    const double a1b = s.A[3 + b], a1c = s.A[3 + cc], a2b = s.A[6 + b], a2c = s.A[6 + cc];
    const double b1b = s.B[3 + b], b1c = s.B[3 + cc], b2b = s.B[6 + b], b2c = s.B[6 + cc];
    const double q2 = a1b * a2c - a1c * a2b;
    const double q1 = (a1b * b2c + b1b * a2c) - (a1c * b2b + b1c * a2b);
    const double q0 = b1b * b2c - b1c * b2b;
    const double a0 = s.A[a], b0 = s.B[a];
    c[3] = c[3] + a0 * q2;
    c[2] = c[2] + (a0 * q1 + b0 * q2);
    c[1] = c[1] + (a0 * q0 + b0 * q1);
    c[0] = c[0] + b0 * q0;
  }
  double big = 0.0;
  for (int k = 0; k <= FM_DEG; ++k) big = fmax(big, fabs(c[k]));
  if (!(big > 0.0) || !isfinite(big)) return false;
  for (int k = 0; k <= FM_DEG; ++k) { c[k] = c[k] / big; s.c[k] = c[k]; }
  if (!(fabs(c[FM_DEG]) > FM_LEAD_TOL)) return false;
  double ratio = 0.0;
  for (int k = 0; k < FM_DEG; ++k) ratio = fmax(ratio, fabs(c[k] / c[FM_DEG]));
  s.bound = 1.0 + ratio;
  // 3. the Sturm chain: p, p', then minus the remainder of the two before, each scaled to a largest coefficient of 1
  for (int k = 0; k <= FM_DEG; ++k) { s.chain[0][k] = c[k]; s.chain[1][k] = k < FM_DEG ? (double)(k + 1) * c[k + 1] : 0.0; }
  s.deg[0] = FM_DEG; s.deg[1] = FM_DEG - 1;
  s.n_chain = 2;
  while (s.n_chain <= FM_DEG && s.deg[s.n_chain - 1] > 0) {
    const int ia = s.n_chain - 2, ib = s.n_chain - 1, da = s.deg[ia], db = s.deg[ib];
    double* r = s.chain[s.n_chain];
    for (int k = 0; k <= FM_DEG; ++k) r[k] = k <= da ? s.chain[ia][k] : 0.0;
    for (int k = da; k >= db; --k) {
      const double q = r[k] / s.chain[ib][db];
      for (int j = 0; j < db; ++j) r[k - db + j] = r[k - db + j] - q * s.chain[ib][j];
      r[k] = 0.0;
    }
    double m = 0.0;
    for (int k = 0; k < db; ++k) m = fmax(m, fabs(r[k]));
    if (!isfinite(m)) return false;
    if (!(m > 0.0)) break;                               // the chain ends at a common divisor
    int d = db - 1;
    for (int k = 0; k < db; ++k) r[k] = -(r[k] / m);
    while (d > 0 && !(fabs(r[d]) > FM_TRIM_TOL)) { r[d] = 0.0; --d; }
    s.deg[s.n_chain] = d;
    ++s.n_chain;
  }
  s.v_low = fm_sign_changes(s, -s.bound);
  s.n_roots = min(max(s.v_low - fm_sign_changes(s, s.bound), 0), FM_DEG);
  return true;
}

// the k-th real root in ascending order (k < s.n_roots)
__device__ inline double fm_root(const FmSolver& s, int k) {
  double lo = -s.bound, hi = s.bound;
  for (int it = 0; it < FM_BISECT; ++it) {
    const double mid = 0.5 * (lo + hi);
    if (s.v_low - fm_sign_changes(s, mid) >= k + 1) hi = mid; else lo = mid;
  }
  double z = 0.5 * (lo + hi);
  for (int it = 0; it < FM_NEWTON; ++it) {
    double p = s.c[FM_DEG], dp = 0.0;
    for (int j = FM_DEG - 1; j >= 0; --j) { dp = dp * z + p; p = p * z + s.c[j]; }
    const double zn = z - p / dp;
    if (zn >= lo && zn <= hi) z = zn;
  }
  return z;
}

// F (row-major, Frobenius norm 1) of root x.  false: a value that is not finite, or F = 0.
__device__ inline bool fm_fundamental(const FmSolver& s, double x, double F[9]) {
  double d = 0.0;
  for (int m = 0; m < 9; ++m) {
    F[m] = x * s.A[m] + s.B[m];
    d += F[m] * F[m];
  }
  const double nrm = sqrt(d);
  if (!(nrm > 0.0) || !isfinite(nrm)) return false;
  for (int m = 0; m < 9; ++m) F[m] = F[m] / nrm;
  return true;
}

// squared Sampson error of record r under F (NaN where the denominator vanishes)
__device__ __forceinline__ double fm_sampson(const double* F, const double* r) {
  const double u1 = r[0], v1 = r[1], u2 = r[2], v2 = r[3];
  const double a0 = (F[0] * u1 + F[1] * v1) + F[2], a1 = (F[3] * u1 + F[4] * v1) + F[5], a2 = (F[6] * u1 + F[7] * v1) + F[8];
  const double b0 = (F[0] * u2 + F[3] * v2) + F[6], b1 = (F[1] * u2 + F[4] * v2) + F[7];
  const double N = (u2 * a0 + v2 * a1) + a2;
  const double D = ((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1;
  return (N * N) / D;
}

// ---- kernel B: the estimator -------------------------------------------------------------------------------------------------------
struct FmArgs {
  const int64_t* offsets; const int32_t* pair_camera; const int32_t* cam_model; const double* cam_params;
  const int32_t* order;        // [n_pairs] pairs by descending match count
  const double* rec;           // [n_matches][PAIR_REC], compacted per pair
  const int32_t* pos;          // [n_matches]
  const int32_t* n_valid;      // [n_pairs]
  int32_t* winner;             // [n_pairs][3] the best key: count (-1: none), sample, root
  double* winner_F;            // [n_pairs][9] its fundamental matrix
  uint8_t* mask_a; uint8_t* mask_b;                   // [n_matches] each: inlier sets of the local optimisation (by compacted position)
  pxr_fundamental_options o;
  int32_t max_trials;          // o.max_num_trials rounded up to a multiple of o.round_size
  double* F; int32_t* status; int32_t* n_inliers; int32_t* n_trials; uint8_t* inlier; double* err;
};

// Every branch that encloses a barrier or a cross-lane operation is uniform over the workgroup; the hypothesis loop, where the
// lanes meet different root counts, has none.
__global__ __launch_bounds__(PAIR_THREADS, 2) void k_fm_hypotheses(const FmArgs a) {
  __shared__ double sh_rec[PAIR_LDS * PAIR_REC];
  __shared__ double sh_ksum[PAIR_WAVES];
  __shared__ int sh_kint[PAIR_WAVES][3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pi = a.order[blockIdx.x];
  PairRecords P;
  if (!open_pair<PairThreshold::BothCameras>(a, pi, 7, sh_rec, P)) {
    if (tid == 0) { a.status[pi] = 1; a.n_inliers[pi] = 0; a.n_trials[pi] = 0; }
    return;
  }
  const int n = P.n;
  const double thr2 = P.thr2;

  // hypotheses: round r (round_size samples) on wavefront r mod 4, its samples strided over the lanes
  HypKey best = {-1, 0.0, 0x7fffffff, FM_DEG};
  int done = 0;
  const auto need = [&](int cnt) {                       // the stop rule: seven inliers in a sample
    const double w = (double)cnt / (double)n;
    const double w2 = w * w;
    return trials_needed(a.o.confidence, a.o.min_num_trials, a.max_trials, cnt, (w2 * w2) * (w2 * w));
  };
  for (int pass = 0;; ++pass) {
    const int round = pass * PAIR_WAVES + wave;
    HypKey mine = {-1, 0.0, 0x7fffffff, FM_DEG};
    if ((int64_t)round * a.o.round_size < a.max_trials) {
      for (int s = lane; s < a.o.round_size; s += 64) {
        const int h = round * a.o.round_size + s;
        int idx[7];
        sample_distinct<7>(a.o.seed, h, n, idx);
        const double* seven[7] = {P.rec(idx[0]), P.rec(idx[1]), P.rec(idx[2]), P.rec(idx[3]), P.rec(idx[4]), P.rec(idx[5]), P.rec(idx[6])};
        FmSolver sv;
        if (!fm_solver_setup(seven, sv)) continue;
        for (int root = 0; root < sv.n_roots; ++root) {
          double F[9];
          if (!fm_fundamental(sv, fm_root(sv, root), F)) continue;
          int cnt = 0;
          double sum = 0.0;
          for (int j = 0; j < n; ++j) {
            const double e2 = fm_sampson(F, P.rec(j));
            double e = thr2;
            if (e2 <= thr2) { ++cnt; e = e2; }
            sum += e;
          }
          const HypKey key = {cnt, sum, h, root};
          if (key.beats(mine)) mine = key;
        }
      }
    }
    wave_best(mine);
    if (merge_rounds<PAIR_WAVES>(sh_ksum, sh_kint, mine, pass, a.o.round_size, a.max_trials, best, done, need)) break;
  }
  if (tid == 0) {
    a.n_trials[pi] = done;
    a.winner[3 * (size_t)pi] = best.cnt; a.winner[3 * (size_t)pi + 1] = best.h; a.winner[3 * (size_t)pi + 2] = best.root;
    if (best.cnt < 0) {
      a.status[pi] = 2; a.n_inliers[pi] = 0;
    } else {                                             // the winner's fundamental matrix: its own arithmetic again, on one lane
      int idx[7];
      sample_distinct<7>(a.o.seed, best.h, n, idx);
      const double* seven[7] = {P.rec(idx[0]), P.rec(idx[1]), P.rec(idx[2]), P.rec(idx[3]), P.rec(idx[4]), P.rec(idx[5]), P.rec(idx[6])};
      FmSolver sv;
      double F[9];
      fm_solver_setup(seven, sv);
      fm_fundamental(sv, fm_root(sv, best.root), F);
      for (int m = 0; m < 9; ++m) a.winner_F[9 * (size_t)pi + m] = F[m];
    }
  }
}

// ---- kernel C: local optimisation, classification ----------------------------------------------------------------------------------
// The rank-2 parametrisation: columns ci, ck of F (the pair (0,1), (0,2), (1,2) with the largest cross product) and the third
// column cl = alpha c_ci + beta c_ck.  x = (c_ci (3), c_ck (3), alpha, beta).
struct FmColumns { int ci, ck, cl; };

// false: every cross product vanishes (or is not finite): no parametrisation
__device__ __forceinline__ bool fm_parametrise(const double* F, FmColumns& col, double x[8]) {
  double best = 0.0;
  col.ci = 0; col.ck = 1; col.cl = 2;
  bool have = false;
  for (int i = 0; i < 2; ++i)
    for (int k = i + 1; k < 3; ++k) {                    // (0,1) (0,2) (1,2)
      const double a[3] = {F[i], F[3 + i], F[6 + i]}, b[3] = {F[k], F[3 + k], F[6 + k]};
      double c[3];
      cross3(a, b, c);
      const double d = dot3(c, c);
      if (d > best) { best = d; col.ci = i; col.ck = k; col.cl = 3 - i - k; have = true; }
    }
  if (!have || !isfinite(best)) return false;
  const double a[3] = {F[col.ci], F[3 + col.ci], F[6 + col.ci]}, b[3] = {F[col.ck], F[3 + col.ck], F[6 + col.ck]};
  const double l[3] = {F[col.cl], F[3 + col.cl], F[6 + col.cl]};
  const double g11 = dot3(a, a), g12 = dot3(a, b), g22 = dot3(b, b), r1 = dot3(a, l), r2 = dot3(b, l);
  const double det = g11 * g22 - g12 * g12;
  if (!(det > 0.0) || !isfinite(det)) return false;
#pragma unroll
  for (int r = 0; r < 3; ++r) { x[r] = a[r]; x[3 + r] = b[r]; }
  x[6] = (r1 * g22 - r2 * g12) / det;
  x[7] = (g11 * r2 - g12 * r1) / det;
  return true;
}

__device__ __forceinline__ void fm_build(const FmColumns& col, const double* x, double F[9]) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    F[3 * r + col.ci] = x[r];
    F[3 * r + col.ck] = x[3 + r];
    F[3 * r + col.cl] = x[6] * x[r] + x[7] * x[3 + r];
  }
}

// sums of J^t J, J^t r and r^2 over the records of `mask`; r = x2^t F x1 / sqrt(D) the signed Sampson residual of F = fm_build(x),
// J = dr / d(the seven entries of x other than `fixed`, in index order).  A record whose denominator is not positive makes the
// cost +inf.
__device__ __forceinline__ void fm_normal_equations(const PairRecords& P, const uint8_t* mask, const FmColumns& col, const double* x, int fixed,
                                                    double (&acc)[FM_ACC], double* sh_part, double* sh_tot) {
#pragma unroll
  for (int c = 0; c < FM_ACC; ++c) acc[c] = 0.0;
  double F[9], dF[8][9];
  fm_build(col, x, F);
#pragma unroll
  for (int m = 0; m < 8; ++m)
#pragma unroll
    for (int j = 0; j < 9; ++j) dF[m][j] = 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    dF[r][3 * r + col.ci] = 1.0; dF[r][3 * r + col.cl] = x[6];
    dF[3 + r][3 * r + col.ck] = 1.0; dF[3 + r][3 * r + col.cl] = x[7];
    dF[6][3 * r + col.cl] = x[r];
    dF[7][3 * r + col.cl] = x[3 + r];
  }
  for (int j = threadIdx.x; j < P.n; j += PAIR_THREADS) {
    if (!mask[P.o0 + j]) continue;
    const double* r = P.rec(j);
    const double u1 = r[0], v1 = r[1], u2 = r[2], v2 = r[3];
    const double a0 = (F[0] * u1 + F[1] * v1) + F[2], a1 = (F[3] * u1 + F[4] * v1) + F[5], a2 = (F[6] * u1 + F[7] * v1) + F[8];
    const double c0 = (F[0] * u2 + F[3] * v2) + F[6], c1 = (F[1] * u2 + F[4] * v2) + F[7];
    const double N = (u2 * a0 + v2 * a1) + a2;
    const double D = ((a0 * a0 + a1 * a1) + c0 * c0) + c1 * c1;
    if (!(D > 0.0) || !isfinite(D)) { acc[35] = pos_inf(); continue; }
    const double sD = sqrt(D), res = N / sD;
    double J[8], K[7];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const double* G = dF[c];
      const double f0 = (G[0] * u1 + G[1] * v1) + G[2], f1 = (G[3] * u1 + G[4] * v1) + G[5], f2 = (G[6] * u1 + G[7] * v1) + G[8];
      const double g0 = (G[0] * u2 + G[3] * v2) + G[6], g1 = (G[1] * u2 + G[4] * v2) + G[7];
      const double dN = (u2 * f0 + v2 * f1) + f2;
      const double dD = 2.0 * (((a0 * f0 + a1 * f1) + c0 * g0) + c1 * g1);
      J[c] = dN / sD - 0.5 * res * dD / D;
    }
#pragma unroll
    for (int m = 0; m < 7; ++m) K[m] = m < fixed ? J[m] : J[m + 1];
    int xx = 0;
#pragma unroll
    for (int m = 0; m < 7; ++m) {
#pragma unroll
      for (int l = m; l < 7; ++l) { acc[xx] += K[m] * K[l]; ++xx; }
      acc[28 + m] += K[m] * res;
    }
    acc[35] += res * res;
  }
  block_sum<PAIR_THREADS, FM_CHUNK>(acc, sh_part, sh_tot);
}

__global__ __launch_bounds__(PAIR_THREADS) void k_fm_refine(const FmArgs a) {
  __shared__ double sh_rec[PAIR_LDS * PAIR_REC];
  __shared__ double sh_part[PAIR_THREADS * FM_CHUNK];
  __shared__ double sh_tot[FM_ACC];
  const int tid = threadIdx.x;
  const int pi = a.order[blockIdx.x];
  PairRecords P;
  if (!open_pair<PairThreshold::BothCameras>(a, pi, 7, sh_rec, P)) return;   // status 1: written by k_fm_hypotheses
  if (a.winner[3 * (size_t)pi] < 0) return;              // status 2: written by k_fm_hypotheses
  const int n = P.n;
  const double thr2 = P.thr2;
  double F[9];
#pragma unroll
  for (int m = 0; m < 9; ++m) F[m] = a.winner_F[9 * (size_t)pi + m];

  // 1-2. the winner's inliers, then the local optimisation: refine on the inliers, classify again, until the set stands still
  uint8_t* cur = a.mask_a;
  uint8_t* nxt = a.mask_b;
  const int cur_cnt = local_optimisation<FM_CHUNK>(
      P, a.o.lo_rounds, F, cur, nxt, [](const double* M, const double* r) { return fm_sampson(M, r); },
      [&](const double* F0, const uint8_t* mask, double (&F1)[9]) {
        FmColumns col;
        double x[8];
        if (!fm_parametrise(F0, col, x)) return false;
        int fixed = 0;                                   // of the six column entries, the one of largest magnitude, the first of equals
#pragma unroll
        for (int m = 1; m < 6; ++m) if (fabs(x[m]) > fabs(x[fixed])) fixed = m;
        lm_refine<7, 8>(a.o.refine_max_iterations, x,
                        [&](const double* y, double (&acc)[FM_ACC]) { fm_normal_equations(P, mask, col, y, fixed, acc, sh_part, sh_tot); },
                        [&](const double* y, const double* d, double* y1) {
#pragma unroll
                          for (int m = 0; m < 8; ++m) y1[m] = m == fixed ? y[m] : y[m] + d[m < fixed ? m : m - 1];
                        });
        fm_build(col, x, F1);
        return true;
      },
      sh_part, sh_tot);

  // 3. the final set (`cur`: the classification under the F that stays) and the success rule
  const int need = max(a.o.min_num_inliers, (int)ceil(a.o.min_inlier_ratio * (double)n));
  if (cur_cnt < need) {
    if (tid == 0) { a.status[pi] = 3; a.n_inliers[pi] = 0; }
    return;
  }
  const double to_px = a.o.max_error / P.thr;
  for (int j = tid; j < n; j += PAIR_THREADS) {
    const double e2 = fm_sampson(F, P.rec(j));
    const int64_t i = P.o0 + a.pos[P.o0 + j];
    a.err[i] = sqrt(e2) * to_px;
    a.inlier[i] = e2 <= thr2 ? 1 : 0;
  }
  if (tid == 0) {
    int big = 0;                                         // the entry of largest magnitude comes out positive, the first of equals
    for (int m = 1; m < 9; ++m) if (fabs(F[m]) > fabs(F[big])) big = m;
    const double sgn = F[big] < 0.0 ? -1.0 : 1.0;
    for (int j = 0; j < 9; ++j) a.F[9 * (size_t)pi + j] = sgn * F[j];
    a.status[pi] = 0; a.n_inliers[pi] = cur_cnt;
  }
}

static int fundamental(pxr_ctx* ctx, int32_t n_pairs, const int64_t* d_pair_offsets, int64_t n_matches, const double* d_xy1,
                       const double* d_xy2, const int32_t* d_pair_camera, int32_t n_cameras, const int32_t* d_cam_model,
                       const double* d_cam_params, const pxr_fundamental_options* o, double* d_F, int32_t* d_status,
                       int32_t* d_n_inliers, int32_t* d_n_trials, uint8_t* d_inlier, double* d_err, double* h_ms) {
  const PairCall c = {"pxr_fundamental", ctx, n_pairs, d_pair_offsets, n_matches, d_xy1, d_xy2, d_pair_camera, n_cameras, d_cam_model,
                      d_cam_params, o, d_status, d_n_inliers, d_n_trials, d_inlier, d_err, h_ms};
  PairBatch b;
  if (int rc = open_pair_batch(c, d_F != nullptr, nullptr, 3, b)) return rc;
  if (n_pairs == 0) return PXR_OK;
  FmArgs a;
  fill_pair_args(a, c, b);
  a.winner_F = b.winner_model;
  a.F = d_F;
  hipLaunchKernelGGL(k_fm_hypotheses, dim3((unsigned)n_pairs), dim3(PAIR_THREADS), 0, ctx->stream, a);
  b.timer->mark(3);
  hipLaunchKernelGGL(k_fm_refine, dim3((unsigned)n_pairs), dim3(PAIR_THREADS), 0, ctx->stream, a);
  return close_pair_batch(b, "k_fm_refine launch");
}

}  // namespace pxr

extern "C" void pxr_fundamental_default_options(pxr_fundamental_options* o) { pxr::pair_default_options(o); }

extern "C" int pxr_fundamental(pxr_ctx* ctx, int32_t n_pairs, const int64_t* d_pair_offsets, int64_t n_matches, const double* d_xy1,
                               const double* d_xy2, const int32_t* d_pair_camera, int32_t n_cameras, const int32_t* d_cam_model,
                               const double* d_cam_params, const pxr_fundamental_options* options, double* d_F, int32_t* d_status,
                               int32_t* d_n_inliers, int32_t* d_n_trials, uint8_t* d_inlier, double* d_err) {
  return pxr::fundamental(ctx, n_pairs, d_pair_offsets, n_matches, d_xy1, d_xy2, d_pair_camera, n_cameras, d_cam_model, d_cam_params,
                          options, d_F, d_status, d_n_inliers, d_n_trials, d_inlier, d_err, nullptr);
}

extern "C" int pxr_fundamental_timed(pxr_ctx* ctx, int32_t n_pairs, const int64_t* d_pair_offsets, int64_t n_matches, const double* d_xy1,
                                     const double* d_xy2, const int32_t* d_pair_camera, int32_t n_cameras, const int32_t* d_cam_model,
                                     const double* d_cam_params, const pxr_fundamental_options* options, double* d_F, int32_t* d_status,
                                     int32_t* d_n_inliers, int32_t* d_n_trials, uint8_t* d_inlier, double* d_err, double* h_kernel_ms) {
  PXR_REQUIRE(h_kernel_ms, "pxr_fundamental_timed: NULL h_kernel_ms");
  return pxr::fundamental(ctx, n_pairs, d_pair_offsets, n_matches, d_xy1, d_xy2, d_pair_camera, n_cameras, d_cam_model, d_cam_params,
                          options, d_F, d_status, d_n_inliers, d_n_trials, d_inlier, d_err, h_kernel_ms);
}
