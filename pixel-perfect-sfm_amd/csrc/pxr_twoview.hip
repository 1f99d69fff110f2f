// pxr_twoview.hip -- batched two-view geometry on gfx950: the matches of many image pairs -> one relative pose and one inlier
// mask each.
//
// Replaces pycolmap.verify_matches / COLMAP's two-view geometry estimation as the reference's pipelines call it between matching
// and everything that reads the match graph (examples/refine_sift_aachen.py:51, hloc's reconstruction and triangulation), for the
// calibrated case: undistort both pixels of every match, estimate an essential matrix robustly from minimal samples (five
// points), decompose it, refine the pose on its inliers.  Like the absolute-pose estimator (pxr_abspose.hip, DESIGN.md section
// 19) it has no random state -- sample h of a pair is a counter-based hash of (seed, h) -- and every choice is a comparison of
// keys, so the result is a function of the pair's own matches alone, bit for bit, alone or inside any batch.
// Records, the opening of a pair and the host side of a call are those of pxr_pairs.h, shared with the homography and
// fundamental-matrix estimators.
//
//   k_tv_hypotheses  the estimator's samples: one workgroup of 256 lanes per pair, the first PAIR_LDS records staged in LDS; a round
//                    of samples per wavefront, a sample per lane, every lane scoring its own essential matrices against all records
//   k_tv_refine      the winner's decomposition, local optimisation and final classification; with a pose prior, only the last
//
// Five-point solver: Nister, "An efficient solution to the five-point relative pose problem", PAMI 2004.  The null space of the
// 5 x 9 epipolar system by Gauss-Jordan (orthonormalised and mixed), E = x X + y Y + z Z + W; the ten cubic constraints det E = 0, (E E^t - tr(E E^t) / 2) E = 0
// formed as polynomial products into a 10 x 20 matrix in Nister's monomial order; Gauss-Jordan on its first ten columns; the
// 3 x 3 matrix polynomial B(z) of the rows (x^2 z) - z (x^2), (y^2 z) - z (y^2), (x y z) - z (x y); det B(z) of degree ten.  Its
// real roots by a Sturm chain and bisection on the sign-change count, with + - x / only.  Pose of E: Horn, "Recovering baseline
// and orientation from essential matrix", 1990 -- no SVD.
//
// Where the solver's state lives: the 10 x 20 system, the Sturm chain (11 polynomials) and the 5 x 9 system are private arrays
// indexed by loop counters and pivot rows, i.e. scratch memory (figures: DESIGN.md section 21); one essential matrix at a time
// is in registers for the scoring walk, which is the larger share of the work from a few hundred matches on.
#include <hip/hip_runtime.h>

#include <cmath>

#include "pxr_device.h"
#include "pxr_pairs.h"

namespace pxr {

constexpr int TV_ACC = 21;                             // the refinement's sums: H (15, upper triangle by rows), g (5), cost
constexpr int TV_CHUNK = 7;                            // of which this many cross the workgroup at a time (PAIR_THREADS x TV_CHUNK doubles of LDS)
constexpr int TV_DEG = 10;                             // degree of the polynomial in z
constexpr int TV_BISECT = 64;                          // bisection steps per root
constexpr int TV_NEWTON = 4;                           // Newton steps per root, each kept only inside the bisection's last interval
constexpr int TV_POLISH = 8;                           // at most this many Gauss-Newton steps per hypothesis on the ten cubic constraints over (x, y, z)
constexpr double TV_POLISH_TOL = 1e-10;                // the last step: one of at most this size relative to max(1, |x|, |y|, |z|)
constexpr double TV_PIVOT_TOL = 1e-12;                 // a pivot counts as zero below this fraction of the system's largest entry
constexpr double TV_LEAD_TOL = 1e-9;                   // the leading coefficient counts as zero below this fraction of the largest one
constexpr double TV_TRIM_TOL = 1e-12;                  // so does the leading coefficient of a rescaled Sturm remainder
constexpr double TV_STEP_TOL = 1e-12;                  // the refinement stops at a step of this norm
constexpr double TV_COST_SLACK = 1e-12;                // a step is kept unless the cost grows by more than this fraction

// ---- the five-point solver ---------------------------------------------------------------------------------------------------------
// Gauss-Jordan with partial pivoting on the first `rows` columns of M (rows x cols, row-major): M -> [I | C].  false: a pivot
// not above TV_PIVOT_TOL times the largest entry M started with (or not a number).
__device__ inline bool tv_gauss_jordan(double* M, int rows, int cols) {
  double S = 0.0;
  for (int x = 0; x < rows * cols; ++x) S = fmax(S, fabs(M[x]));
  if (!isfinite(S)) return false;
  for (int c = 0; c < rows; ++c) {
    int pr = c;
    double pa = fabs(M[c * cols + c]);
    for (int r = c + 1; r < rows; ++r) {
      const double v = fabs(M[r * cols + c]);
      if (v > pa) { pa = v; pr = r; }
    }
    if (!(pa > TV_PIVOT_TOL * S)) return false;
    if (pr != c)
      for (int k = c; k < cols; ++k) { const double v = M[c * cols + k]; M[c * cols + k] = M[pr * cols + k]; M[pr * cols + k] = v; }
    const double p = M[c * cols + c];
    for (int k = c; k < cols; ++k) M[c * cols + k] = M[c * cols + k] / p;
    for (int r = 0; r < rows; ++r) {
      if (r == c) continue;
      const double f = M[r * cols + c];
      for (int k = c + 1; k < cols; ++k) M[r * cols + k] = M[r * cols + k] - f * M[c * cols + k];
      M[r * cols + c] = 0.0;
    }
  }
  return true;
}

// polynomials in (x, y, z, 1) = variables 0 .. 3: degree 1 as 4 coefficients, degree 2 as 10 (pairs i <= j in lexicographic
// order), degree 3 as 20 (triples i <= j <= k in lexicographic order)
__device__ __forceinline__ constexpr int tv_pair(int i, int j) { return i * 4 - i * (i - 1) / 2 + (j - i); }
__device__ __forceinline__ constexpr int tv_triple(int a, int b, int c) {
  int idx = 0;
  for (int i = 0; i < 4; ++i)
    for (int j = i; j < 4; ++j)
      for (int k = j; k < 4; ++k) {
        if (i == a && j == b && k == c) return idx;
        ++idx;
      }
  return -1;
}
// Nister's column of a monomial: x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x | yz^2 yz y | z^3 z^2 z 1
__device__ __forceinline__ constexpr int tv_column(int lex) {
  constexpr int col[20] = {0, 2, 4, 5, 3, 8, 9, 10, 11, 12, 1, 6, 7, 13, 14, 15, 16, 17, 18, 19};
  return col[lex];
}
// out (degree 2) += a b
__device__ __forceinline__ void tv_mul11(const double* a, const double* b, double* out) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) out[tv_pair(i < j ? i : j, i < j ? j : i)] += a[i] * b[j];
}
// row (degree 3, in Nister's column order) += p (degree 2) a
__device__ __forceinline__ void tv_mul21(const double* p, const double* a, double* row) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = i; j < 4; ++j)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int lo = k < i ? k : i, hi = k > j ? k : j, mid = i + j + k - lo - hi;
        row[tv_column(tv_triple(lo, mid, hi))] += p[tv_pair(i, j)] * a[k];
      }
}

struct TvSolver {
  double basis[9][4];          // E[m] = x basis[m][0] + y basis[m][1] + z basis[m][2] + basis[m][3]
  double bx[3][4], by[3][4], bw[3][5];   // B(z): row r = (bx[r](z), by[r](z), bw[r](z)), ascending powers
  double c[TV_DEG + 1];        // det B(z), scaled to a largest coefficient of 1
  double chain[TV_DEG + 1][TV_DEG + 1];  // the Sturm chain, ascending powers
  int deg[TV_DEG + 1];
  int n_chain;
  double bound;                // Cauchy's: every real root in (-bound, bound)
  int v_low;                   // sign changes at -bound
  int n_roots;
};

__device__ inline int tv_sign_changes(const TvSolver& s, double x) {
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

// r1 .. r5: the records (u1, v1, u2, v2) of a sample.  false: no hypothesis (degenerate sample, vanishing pivot or leading
// coefficient, a value that is not finite).
__device__ inline bool tv_solver_setup(const double* const* rec, TvSolver& s) {
  // 1. the null space of the epipolar system x2^t E x1 = 0, E row-major: Gauss-Jordan with full pivoting -> [I | C] in permuted
  //    columns, vector k = (-C[:, k], e_k); orthonormalised (modified Gram-Schmidt, k = 0 .. 3); mixed by the 4 x 4 Hadamard matrix
  //    / 2, so that no single entry of E decides the size of the constant term W
  {
    double A[5 * 9];
    int perm[9];
    for (int m = 0; m < 5; ++m) {
      const double u1 = rec[m][0], v1 = rec[m][1], u2 = rec[m][2], v2 = rec[m][3];
      double* a = A + m * 9;
      a[0] = u2 * u1; a[1] = u2 * v1; a[2] = u2; a[3] = v2 * u1; a[4] = v2 * v1; a[5] = v2; a[6] = u1; a[7] = v1; a[8] = 1.0;
    }
    double S = 0.0;
    for (int x = 0; x < 45; ++x) S = fmax(S, fabs(A[x]));
    if (!isfinite(S)) return false;
    for (int k = 0; k < 9; ++k) perm[k] = k;
    for (int c = 0; c < 5; ++c) {
      int pr = c, pc = c;
      double pa = fabs(A[c * 9 + c]);
      for (int r = c; r < 5; ++r)
        for (int k = c; k < 9; ++k) {
          const double v = fabs(A[r * 9 + k]);
          if (v > pa) { pa = v; pr = r; pc = k; }
        }
      if (!(pa > TV_PIVOT_TOL * S)) return false;
      if (pr != c)
        for (int k = 0; k < 9; ++k) { const double v = A[c * 9 + k]; A[c * 9 + k] = A[pr * 9 + k]; A[pr * 9 + k] = v; }
      if (pc != c) {
        for (int r = 0; r < 5; ++r) { const double v = A[r * 9 + c]; A[r * 9 + c] = A[r * 9 + pc]; A[r * 9 + pc] = v; }
        const int v = perm[c]; perm[c] = perm[pc]; perm[pc] = v;
      }
      const double p = A[c * 9 + c];
      for (int k = c; k < 9; ++k) A[c * 9 + k] = A[c * 9 + k] / p;
      for (int r = 0; r < 5; ++r) {
        if (r == c) continue;
        const double f = A[r * 9 + c];
        for (int k = c + 1; k < 9; ++k) A[r * 9 + k] = A[r * 9 + k] - f * A[c * 9 + k];
        A[r * 9 + c] = 0.0;
      }
    }
    double u[4][9];
    for (int k = 0; k < 4; ++k) {
      for (int r = 0; r < 5; ++r) u[k][perm[r]] = -A[r * 9 + 5 + k];
      for (int j = 0; j < 4; ++j) u[k][perm[5 + j]] = j == k ? 1.0 : 0.0;
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
      s.basis[m][0] = 0.5 * (((u[0][m] + u[1][m]) + u[2][m]) + u[3][m]);
      s.basis[m][1] = 0.5 * (((u[0][m] - u[1][m]) + u[2][m]) - u[3][m]);
      s.basis[m][2] = 0.5 * (((u[0][m] + u[1][m]) - u[2][m]) - u[3][m]);
      s.basis[m][3] = 0.5 * (((u[0][m] - u[1][m]) - u[2][m]) + u[3][m]);
    }
  }
  // 2. the ten cubic constraints
  double M[10 * 20];
  {
    double EEt[6][10];                                   // (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
    int x = 0;
    for (int a = 0; a < 3; ++a)
      for (int b = a; b < 3; ++b) {
        for (int k = 0; k < 10; ++k) EEt[x][k] = 0.0;
        for (int cc = 0; cc < 3; ++cc) tv_mul11(s.basis[3 * a + cc], s.basis[3 * b + cc], EEt[x]);
        ++x;
      }
    for (int k = 0; k < 10; ++k) {
      const double half_tr = 0.5 * ((EEt[0][k] + EEt[3][k]) + EEt[5][k]);
      EEt[0][k] -= half_tr; EEt[3][k] -= half_tr; EEt[5][k] -= half_tr;
    }
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) {
        double row[20];
        for (int k = 0; k < 20; ++k) row[k] = 0.0;
        for (int cc = 0; cc < 3; ++cc) {
          const int lo = a < cc ? a : cc, hi = a < cc ? cc : a;
          tv_mul21(EEt[lo == 0 ? hi : lo == 1 ? 2 + hi : 5], s.basis[3 * cc + b], row);
        }
        for (int k = 0; k < 20; ++k) M[(3 * a + b) * 20 + k] = row[k];
      }
    double row[20];
    for (int k = 0; k < 20; ++k) row[k] = 0.0;
    for (int a = 0; a < 3; ++a) {                        // det E = sum_a E[0][a] (E[1][a+1] E[2][a+2] - E[1][a+2] E[2][a+1])
      const int b = (a + 1) % 3, cc = (a + 2) % 3;
      double pos[10], neg[10];
      for (int k = 0; k < 10; ++k) pos[k] = neg[k] = 0.0;
      tv_mul11(s.basis[3 + b], s.basis[6 + cc], pos);
      tv_mul11(s.basis[3 + cc], s.basis[6 + b], neg);
      for (int k = 0; k < 10; ++k) pos[k] -= neg[k];
      tv_mul21(pos, s.basis[a], row);
    }
    for (int k = 0; k < 20; ++k) M[9 * 20 + k] = row[k];
  }
  if (!tv_gauss_jordan(M, 10, 20)) return false;
  // 3. B(z): rows (4) - z (5), (6) - z (7), (8) - z (9) of [I | C]; columns 10-12 x (z^2, z, 1), 13-15 y, 16-19 1 (z^3 .. 1)
  for (int r = 0; r < 3; ++r) {
    const double* e = M + (4 + 2 * r) * 20;
    const double* f = M + (5 + 2 * r) * 20;
    s.bx[r][0] = e[12]; s.bx[r][1] = e[11] - f[12]; s.bx[r][2] = e[10] - f[11]; s.bx[r][3] = -f[10];
    s.by[r][0] = e[15]; s.by[r][1] = e[14] - f[15]; s.by[r][2] = e[13] - f[14]; s.by[r][3] = -f[13];
    s.bw[r][0] = e[19]; s.bw[r][1] = e[18] - f[19]; s.bw[r][2] = e[17] - f[18]; s.bw[r][3] = e[16] - f[17]; s.bw[r][4] = -f[16];
  }
  // 4. det B = bx0 (by1 bw2 - bw1 by2) - by0 (bx1 bw2 - bw1 bx2) + bw0 (bx1 by2 - by1 bx2)
  double c[TV_DEG + 1];
  for (int k = 0; k <= TV_DEG; ++k) c[k] = 0.0;
  {
    double m0[8], m1[8], m2[7];
    for (int k = 0; k < 8; ++k) m0[k] = m1[k] = 0.0;
    for (int k = 0; k < 7; ++k) m2[k] = 0.0;
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 5; ++j) {
        m0[i + j] += s.by[1][i] * s.bw[2][j] - s.by[2][i] * s.bw[1][j];
        m1[i + j] += s.bx[1][i] * s.bw[2][j] - s.bx[2][i] * s.bw[1][j];
      }
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) m2[i + j] += s.bx[1][i] * s.by[2][j] - s.by[1][i] * s.bx[2][j];
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 8; ++j) c[i + j] += s.bx[0][i] * m0[j] - s.by[0][i] * m1[j];
    for (int i = 0; i < 5; ++i)
      for (int j = 0; j < 7; ++j) c[i + j] += s.bw[0][i] * m2[j];
  }
  double big = 0.0;
  for (int k = 0; k <= TV_DEG; ++k) big = fmax(big, fabs(c[k]));
  if (!(big > 0.0) || !isfinite(big)) return false;
  for (int k = 0; k <= TV_DEG; ++k) { c[k] = c[k] / big; s.c[k] = c[k]; }
  if (!(fabs(c[TV_DEG]) > TV_LEAD_TOL)) return false;
  double ratio = 0.0;
  for (int k = 0; k < TV_DEG; ++k) ratio = fmax(ratio, fabs(c[k] / c[TV_DEG]));
  s.bound = 1.0 + ratio;
  // 5. the Sturm chain: p, p', then minus the remainder of the two before, each scaled to a largest coefficient of 1
  for (int k = 0; k <= TV_DEG; ++k) { s.chain[0][k] = c[k]; s.chain[1][k] = k < TV_DEG ? (double)(k + 1) * c[k + 1] : 0.0; }
  s.deg[0] = TV_DEG; s.deg[1] = TV_DEG - 1;
  s.n_chain = 2;
  while (s.n_chain <= TV_DEG && s.deg[s.n_chain - 1] > 0) {
    const int ia = s.n_chain - 2, ib = s.n_chain - 1, da = s.deg[ia], db = s.deg[ib];
    double* r = s.chain[s.n_chain];
    for (int k = 0; k <= TV_DEG; ++k) r[k] = k <= da ? s.chain[ia][k] : 0.0;
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
    while (d > 0 && !(fabs(r[d]) > TV_TRIM_TOL)) { r[d] = 0.0; --d; }
    s.deg[s.n_chain] = d;
    ++s.n_chain;
  }
  s.v_low = tv_sign_changes(s, -s.bound);
  s.n_roots = min(max(s.v_low - tv_sign_changes(s, s.bound), 0), TV_DEG);
  return true;
}

// the k-th real root in ascending order (k < s.n_roots)
__device__ inline double tv_root(const TvSolver& s, int k) {
  double lo = -s.bound, hi = s.bound;
  for (int it = 0; it < TV_BISECT; ++it) {
    const double mid = 0.5 * (lo + hi);
    if (s.v_low - tv_sign_changes(s, mid) >= k + 1) hi = mid; else lo = mid;
  }
  double z = 0.5 * (lo + hi);
  for (int it = 0; it < TV_NEWTON; ++it) {
    double p = s.c[TV_DEG], dp = 0.0;
    for (int j = TV_DEG - 1; j >= 0; --j) { dp = dp * z + p; p = p * z + s.c[j]; }
    const double zn = z - p / dp;
    if (zn >= lo && zn <= hi) z = zn;
  }
  return z;
}

// the cofactor matrix of the row-major 3 x 3 matrix E: d det(E) / dE
__device__ __forceinline__ void tv_cofactors(const double* E, double* c) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
      c[3 * i + j] = E[3 * i1 + j1] * E[3 * i2 + j2] - E[3 * i1 + j2] * E[3 * i2 + j1];
    }
}

// Up to TV_POLISH Gauss-Newton steps (until one is no larger than TV_POLISH_TOL: convergence is quadratic, what is left is
// rounding; a root that the elimination misplaced by the matrix's own size needs six) on 2 E E^t E - tr(E E^t) E = 0, det E = 0 of E = x N0 + y N1 + z N2 + N3 over (x, y, z): the
// constraints are evaluated on the 3 x 3 matrix itself, which is well conditioned where the elimination to det B(z) is not (the
// elimination loses up to eleven digits on ordinary samples and whole roots at low parallax).  The 3 x 3
// normal equations of a step by the adjugate; a step is skipped where their determinant vanishes or the step is not finite.
__device__ inline void tv_polish(const TvSolver& s, double& x, double& y, double& z) {
  for (int it = 0; it < TV_POLISH; ++it) {
    double E[9], M[9], G[9], ME[9], cof[9], r[10], J[3][10];
    for (int m = 0; m < 9; ++m) E[m] = ((x * s.basis[m][0] + y * s.basis[m][1]) + z * s.basis[m][2]) + s.basis[m][3];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        double m = 0.0, g = 0.0;
        for (int k = 0; k < 3; ++k) { m += E[3 * i + k] * E[3 * j + k]; g += E[3 * k + i] * E[3 * k + j]; }
        M[3 * i + j] = m; G[3 * i + j] = g;
      }
    const double tr = M[0] + M[4] + M[8];
    tv_cofactors(E, cof);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        double v = 0.0;
        for (int k = 0; k < 3; ++k) v += M[3 * i + k] * E[3 * k + j];
        ME[3 * i + j] = v;
        r[3 * i + j] = 2.0 * v - tr * E[3 * i + j];
      }
    r[9] = E[0] * cof[0] + E[1] * cof[1] + E[2] * cof[2];
    for (int c = 0; c < 3; ++c) {                        // the derivative along N_c: D = basis[.][c]
      double ED = 0.0, cD = 0.0, DtE[9];
      for (int m = 0; m < 9; ++m) { ED += E[m] * s.basis[m][c]; cD += cof[m] * s.basis[m][c]; }
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
          double v = 0.0;
          for (int k = 0; k < 3; ++k) v += s.basis[3 * k + i][c] * E[3 * k + j];
          DtE[3 * i + j] = v;
        }
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
          double dg = 0.0, ede = 0.0, md = 0.0;
          for (int k = 0; k < 3; ++k) {
            dg += s.basis[3 * i + k][c] * G[3 * k + j]; ede += E[3 * i + k] * DtE[3 * k + j]; md += M[3 * i + k] * s.basis[3 * k + j][c];
          }
          J[c][3 * i + j] = 2.0 * ((dg + ede) + md) - 2.0 * ED * E[3 * i + j] - tr * s.basis[3 * i + j][c];
        }
      J[c][9] = cD;
    }
    double A[9], g[3], adj[9];
    for (int a = 0; a < 3; ++a) {
      for (int b = 0; b < 3; ++b) {
        double v = 0.0;
        for (int m = 0; m < 10; ++m) v += J[a][m] * J[b][m];
        A[3 * a + b] = v;
      }
      double v = 0.0;
      for (int m = 0; m < 10; ++m) v += J[a][m] * r[m];
      g[a] = v;
    }
    tv_cofactors(A, adj);                                // A is symmetric: its cofactor matrix is its adjugate
    const double dA = A[0] * adj[0] + A[1] * adj[1] + A[2] * adj[2];
    const double d0 = (adj[0] * g[0] + adj[1] * g[1] + adj[2] * g[2]) / dA, d1 = (adj[3] * g[0] + adj[4] * g[1] + adj[5] * g[2]) / dA,
                 d2 = (adj[6] * g[0] + adj[7] * g[1] + adj[8] * g[2]) / dA;
    if (!(dA != 0.0 && isfinite(d0) && isfinite(d1) && isfinite(d2))) break;      // (a skipped step would only repeat itself)
    x -= d0; y -= d1; z -= d2;
    if (fmax(fmax(fabs(d0), fabs(d1)), fabs(d2)) <= TV_POLISH_TOL * fmax(fmax(1.0, fabs(x)), fmax(fabs(y), fabs(z)))) break;
  }
}

// E (row-major) of root z: (x, y, 1) spans the null space of B(z) -- the cross product of two of its rows, the pair with the
// largest third component.  false: none, or a value that is not finite.
__device__ inline bool tv_essential(const TvSolver& s, double z, double E[9]) {   // (z: a copy, polished with x and y)
  double B[3][3];
  for (int r = 0; r < 3; ++r) {
    B[r][0] = ((s.bx[r][3] * z + s.bx[r][2]) * z + s.bx[r][1]) * z + s.bx[r][0];
    B[r][1] = ((s.by[r][3] * z + s.by[r][2]) * z + s.by[r][1]) * z + s.by[r][0];
    B[r][2] = (((s.bw[r][4] * z + s.bw[r][3]) * z + s.bw[r][2]) * z + s.bw[r][1]) * z + s.bw[r][0];
  }
  double best[3] = {0.0, 0.0, 0.0};
  for (int a = 0; a < 2; ++a)
    for (int b = a + 1; b < 3; ++b) {                    // (0,1) (0,2) (1,2)
      const double w = B[a][0] * B[b][1] - B[a][1] * B[b][0];
      if (fabs(w) > fabs(best[2])) {
        best[0] = B[a][1] * B[b][2] - B[a][2] * B[b][1]; best[1] = B[a][2] * B[b][0] - B[a][0] * B[b][2]; best[2] = w;
      }
    }
  if (!(fabs(best[2]) > 0.0)) return false;
  double x = best[0] / best[2], y = best[1] / best[2];
  bool ok = isfinite(x) && isfinite(y);
  if (ok) tv_polish(s, x, y, z);
  for (int m = 0; m < 9; ++m) {
    E[m] = ((x * s.basis[m][0] + y * s.basis[m][1]) + z * s.basis[m][2]) + s.basis[m][3];
    ok = ok && isfinite(E[m]);
  }
  return ok;
}

// squared Sampson error of record r under E (NaN where the denominator vanishes)
__device__ __forceinline__ double tv_sampson(const double* E, const double* r) {
  const double u1 = r[0], v1 = r[1], u2 = r[2], v2 = r[3];
  const double a0 = (E[0] * u1 + E[1] * v1) + E[2], a1 = (E[3] * u1 + E[4] * v1) + E[5], a2 = (E[6] * u1 + E[7] * v1) + E[8];
  const double b0 = (E[0] * u2 + E[3] * v2) + E[6], b1 = (E[1] * u2 + E[4] * v2) + E[7];
  const double N = (u2 * a0 + v2 * a1) + a2;
  const double D = ((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1;
  return (N * N) / D;
}

// ---- kernel B: the estimator -------------------------------------------------------------------------------------------------------
struct TvArgs {
  const int64_t* offsets; const int32_t* pair_camera; const int32_t* cam_model; const double* cam_params;
  const double* prior_qvec; const double* prior_tvec;   // both null: estimate; else [n_pairs][4] / [n_pairs][3]
  const int32_t* order;        // [n_pairs] pairs by descending match count
  const double* rec;           // [n_matches][PAIR_REC], compacted per pair
  const int32_t* pos;          // [n_matches]
  const int32_t* n_valid;      // [n_pairs]
  int32_t* winner;             // [n_pairs][3] the best key: count (-1: none), sample, root
  double* winner_E;            // [n_pairs][9] its essential matrix
  uint8_t* mask_a; uint8_t* mask_b;                   // [n_matches] each: inlier sets of the local optimisation (by compacted position)
  pxr_two_view_options o;
  int32_t max_trials;          // o.max_num_trials rounded up to a multiple of o.round_size
  double* qvec; double* tvec; double* E; int32_t* status; int32_t* n_inliers; int32_t* n_trials; uint8_t* inlier; double* err;
};

// Every branch that encloses a barrier or a cross-lane operation is uniform over the workgroup; the hypothesis loop, where the
// lanes meet different root counts, has none.
__global__ __launch_bounds__(PAIR_THREADS) void k_tv_hypotheses(const TvArgs a) {
  __shared__ double sh_rec[PAIR_LDS * PAIR_REC];
  __shared__ double sh_ksum[PAIR_WAVES];
  __shared__ int sh_kint[PAIR_WAVES][3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pi = a.order[blockIdx.x];
  PairRecords P;
  if (!open_pair<PairThreshold::BothCameras>(a, pi, 5, sh_rec, P)) {
    if (tid == 0) { a.status[pi] = 1; a.n_inliers[pi] = 0; a.n_trials[pi] = 0; }
    return;
  }
  const int n = P.n;
  const double thr2 = P.thr2;

  // 1. hypotheses: round r (round_size samples) on wavefront r mod 4, its samples strided over the lanes
  HypKey best = {-1, 0.0, 0x7fffffff, TV_DEG};
  int done = 0;
  const auto need = [&](int cnt) {                       // the stop rule: five inliers in a sample
    const double w = (double)cnt / (double)n;
    return trials_needed(a.o.confidence, a.o.min_num_trials, a.max_trials, cnt, (w * w) * (w * w) * w);
  };
  for (int pass = 0;; ++pass) {
    const int round = pass * PAIR_WAVES + wave;
    HypKey mine = {-1, 0.0, 0x7fffffff, TV_DEG};
    if ((int64_t)round * a.o.round_size < a.max_trials) {
      for (int s = lane; s < a.o.round_size; s += 64) {
        const int h = round * a.o.round_size + s;
        int idx[5];
        sample_distinct<5>(a.o.seed, h, n, idx);
        const double* five[5] = {P.rec(idx[0]), P.rec(idx[1]), P.rec(idx[2]), P.rec(idx[3]), P.rec(idx[4])};
        TvSolver sv;
        if (!tv_solver_setup(five, sv)) continue;
        for (int root = 0; root < sv.n_roots; ++root) {
          double E[9];
          if (!tv_essential(sv, tv_root(sv, root), E)) continue;
          int cnt = 0;
          double sum = 0.0;
          for (int j = 0; j < n; ++j) {
            const double e2 = tv_sampson(E, P.rec(j));
            double e = thr2;
            if (e2 <= thr2) { ++cnt; e = e2; }
            sum += e;
          }
          const HypKey key = {cnt, sum, h, root};
          if (key.beats(mine)) mine = key;
        }
      }
    }
    // wave_best and merge_rounds (pxr_robust.h) written out: called as functions, the same statements leave this kernel -- at
    // 256 VGPRs with spills -- two spill registers fewer (186 AGPRs for 188), and its resource table is kept as it was
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      HypKey other;
      other.cnt = __shfl_xor(mine.cnt, off, 64); other.sum = __shfl_xor(mine.sum, off, 64);
      other.h = __shfl_xor(mine.h, off, 64); other.root = __shfl_xor(mine.root, off, 64);
      if (other.beats(mine)) mine = other;
    }
    if (lane == 0) { sh_ksum[wave] = mine.sum; sh_kint[wave][0] = mine.cnt; sh_kint[wave][1] = mine.h; sh_kint[wave][2] = mine.root; }
    __syncthreads();
    bool stop = false;
    for (int w = 0; w < PAIR_WAVES && !stop; ++w) {       // the rounds in order; the stop rule at every round boundary
      if ((int64_t)(pass * PAIR_WAVES + w) * a.o.round_size >= a.max_trials) { stop = true; break; }
      const HypKey key = {sh_kint[w][0], sh_ksum[w], sh_kint[w][1], sh_kint[w][2]};
      if (key.beats(best)) best = key;
      done = (pass * PAIR_WAVES + w + 1) * a.o.round_size;
      stop = (double)done >= need(best.cnt);
    }
    __syncthreads();
    if (stop) break;
  }
  if (tid == 0) {
    a.n_trials[pi] = done;
    a.winner[3 * (size_t)pi] = best.cnt; a.winner[3 * (size_t)pi + 1] = best.h; a.winner[3 * (size_t)pi + 2] = best.root;
    if (best.cnt < 0) {
      a.status[pi] = 2; a.n_inliers[pi] = 0;
    } else {                                             // the winner's essential matrix: its own arithmetic again, on one lane
      int idx[5];
      sample_distinct<5>(a.o.seed, best.h, n, idx);
      const double* five[5] = {P.rec(idx[0]), P.rec(idx[1]), P.rec(idx[2]), P.rec(idx[3]), P.rec(idx[4])};
      TvSolver sv;
      double E[9];
      tv_solver_setup(five, sv);
      tv_essential(sv, tv_root(sv, best.root), E);
      for (int m = 0; m < 9; ++m) a.winner_E[9 * (size_t)pi + m] = E[m];
    }
  }
}

// ---- kernel C: decomposition, local optimisation, classification -------------------------------------------------------------------
// E = [t]x R, row-major: column j of E = t x (column j of R)
__device__ __forceinline__ void tv_essential_of_pose(const double* R, const double* t, double E[9]) {
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    E[j] = t[1] * R[6 + j] - t[2] * R[3 + j];
    E[3 + j] = t[2] * R[j] - t[0] * R[6 + j];
    E[6 + j] = t[0] * R[3 + j] - t[1] * R[j];
  }
}

// Horn 1990: t t^t = tr(E E^t) / 2 I - E E^t (t from the row of the largest diagonal entry, unit length); |t|^2 R = Cof(E) -+ [t]x E
// with Cof(E) the matrix of cofactors (row i = row i+1 x row i+2 of E).  Ra goes with -, Rb (the twisted pair) with +.
// false: E = 0 or a value that is not finite.
__device__ __forceinline__ bool tv_horn(const double* E, double t[3], double Ra[9], double Rb[9]) {
  const double d0 = dot3(E, E), d1 = dot3(E + 3, E + 3), d2 = dot3(E + 6, E + 6);
  const double half_tr = 0.5 * ((d0 + d1) + d2);
  const double T[3][3] = {{half_tr - d0, -dot3(E, E + 3), -dot3(E, E + 6)},
                          {-dot3(E + 3, E), half_tr - d1, -dot3(E + 3, E + 6)},
                          {-dot3(E + 6, E), -dot3(E + 6, E + 3), half_tr - d2}};
  int m = 0;
  if (T[1][1] > T[m][m]) m = 1;
  if (T[2][2] > T[m][m]) m = 2;
  if (!(T[m][m] > 0.0) || !isfinite(half_tr)) return false;
  const double nt = sqrt((T[m][0] * T[m][0] + T[m][1] * T[m][1]) + T[m][2] * T[m][2]);
  if (!(nt > 0.0)) return false;
#pragma unroll
  for (int j = 0; j < 3; ++j) t[j] = T[m][j] / nt;
  // with |t| = 1 and E scaled to tr(E E^t) = 2: R = Cof(E) - [t]x E
  const double sc = 1.0 / sqrt(half_tr);
  double En[9], C[9], tE[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) En[j] = E[j] * sc;
  cross3(En + 3, En + 6, C); cross3(En + 6, En, C + 3); cross3(En, En + 3, C + 6);
  tv_essential_of_pose(En, t, tE);                       // [t]x En, column by column
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 9; ++j) { Ra[j] = C[j] - tE[j]; Rb[j] = C[j] + tE[j]; ok = ok && isfinite(Ra[j]) && isfinite(Rb[j]); }
  return ok;
}

// whether record r lies in front of both cameras under (R, t): lambda2 x2 = lambda1 R x1 + t with both lambdas positive
__device__ __forceinline__ bool tv_in_front(const double* R, const double* t, const double* r) {
  const double x2[3] = {r[2], r[3], 1.0};
  const double a[3] = {(R[0] * r[0] + R[1] * r[1]) + R[2], (R[3] * r[0] + R[4] * r[1]) + R[5], (R[6] * r[0] + R[7] * r[1]) + R[8]};
  double c[3], d[3];
  cross3(x2, a, c); cross3(x2, t, d);
  const double s1 = -dot3(c, d), cc = dot3(c, c);
  const double p[3] = {s1 * a[0] + cc * t[0], s1 * a[1] + cc * t[1], s1 * a[2] + cc * t[2]};
  return s1 > 0.0 && dot3(p, x2) > 0.0;
}

// the tangent basis of the unit sphere at t: m = the axis of the smallest |t_m| (the first of equals), b1 = t x e_m / |t x e_m|,
// b2 = t x b1
__device__ __forceinline__ void tv_tangent_basis(const double* t, double b1[3], double b2[3]) {
  int m = 0;
  if (fabs(t[1]) < fabs(t[m])) m = 1;
  if (fabs(t[2]) < fabs(t[m])) m = 2;
  const double e[3] = {m == 0 ? 1.0 : 0.0, m == 1 ? 1.0 : 0.0, m == 2 ? 1.0 : 0.0};
  cross3(t, e, b1);
  const double inv = 1.0 / sqrt(dot3(b1, b1));
#pragma unroll
  for (int j = 0; j < 3; ++j) b1[j] *= inv;
  cross3(t, b1, b2);
}

// H = sum J^t J, g = sum J^t r, cost = sum r^2 over the records of `mask`; r = x2^t E x1 / sqrt(D) the signed Sampson residual of
// E = [t]x R(q), J = dr / d(rotation tangent (3), a, b): R(d) = R(2 d) R, t(a, b) = (t + a b1 + b b2) / |.|
__device__ __forceinline__ void tv_normal_equations(const PairRecords& P, const uint8_t* mask, const double* q, const double* t,
                                                    double (&acc)[TV_ACC], double* sh_part, double* sh_tot) {
#pragma unroll
  for (int c = 0; c < TV_ACC; ++c) acc[c] = 0.0;
  double R[9], E[9], dE[5][9], b1[3], b2[3];
  quat_to_rotation(q, R);
  tv_essential_of_pose(R, t, E);
  tv_tangent_basis(t, b1, b2);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double G[9];                                         // 2 [e_c]x R: column j = 2 e_c x (column j of R)
    const double e[3] = {c == 0 ? 2.0 : 0.0, c == 1 ? 2.0 : 0.0, c == 2 ? 2.0 : 0.0};
    tv_essential_of_pose(R, e, G);
    tv_essential_of_pose(G, t, dE[c]);
  }
  tv_essential_of_pose(R, b1, dE[3]);
  tv_essential_of_pose(R, b2, dE[4]);
  for (int j = threadIdx.x; j < P.n; j += PAIR_THREADS) {
    if (!mask[P.o0 + j]) continue;
    const double* r = P.rec(j);
    const double u1 = r[0], v1 = r[1], u2 = r[2], v2 = r[3];
    const double a0 = (E[0] * u1 + E[1] * v1) + E[2], a1 = (E[3] * u1 + E[4] * v1) + E[5], a2 = (E[6] * u1 + E[7] * v1) + E[8];
    const double c0 = (E[0] * u2 + E[3] * v2) + E[6], c1 = (E[1] * u2 + E[4] * v2) + E[7];
    const double N = (u2 * a0 + v2 * a1) + a2;
    const double D = ((a0 * a0 + a1 * a1) + c0 * c0) + c1 * c1;
    if (!(D > 0.0) || !isfinite(D)) { acc[20] = pos_inf(); continue; }
    const double sD = sqrt(D), res = N / sD;
    double J[5];
#pragma unroll
    for (int c = 0; c < 5; ++c) {
      const double* F = dE[c];
      const double f0 = (F[0] * u1 + F[1] * v1) + F[2], f1 = (F[3] * u1 + F[4] * v1) + F[5], f2 = (F[6] * u1 + F[7] * v1) + F[8];
      const double g0 = (F[0] * u2 + F[3] * v2) + F[6], g1 = (F[1] * u2 + F[4] * v2) + F[7];
      const double dN = (u2 * f0 + v2 * f1) + f2;
      const double dD = 2.0 * (((a0 * f0 + a1 * f1) + c0 * g0) + c1 * g1);
      J[c] = dN / sD - 0.5 * res * dD / D;
    }
    int x = 0;
#pragma unroll
    for (int m = 0; m < 5; ++m) {
#pragma unroll
      for (int l = m; l < 5; ++l) { acc[x] += J[m] * J[l]; ++x; }
      acc[15 + m] += J[m] * res;
    }
    acc[20] += res * res;
  }
  block_sum<PAIR_THREADS, TV_CHUNK>(acc, sh_part, sh_tot);
}

// x (+) d: QuaternionManifold::Plus [upstream Ceres manifold.cc] on q as section 19 moves it (q re-normalised); t along its
// tangent basis and back onto the sphere
__device__ __forceinline__ void tv_pose_plus(const double* q0, const double* t0, const double* d, double q1[4], double t1[3]) {
  quat_plus(q0, d, q1);
  double b1[3], b2[3];
  tv_tangent_basis(t0, b1, b2);
#pragma unroll
  for (int j = 0; j < 3; ++j) t1[j] = (t0[j] + d[3] * b1[j]) + d[4] * b2[j];
  const double it = 1.0 / sqrt(dot3(t1, t1));
#pragma unroll
  for (int j = 0; j < 3; ++j) t1[j] *= it;
}

// Levenberg-Marquardt on the records of `mask`, (q, t) refined in place.  Every lane holds the same sums, so every lane takes
// the same decisions and ends with the same pose.
__device__ __forceinline__ void tv_refine(const TvArgs& a, const PairRecords& P, const uint8_t* mask, double q[4], double t[3],
                                          double* sh_part, double* sh_tot) {
  double acc[TV_ACC];
  tv_normal_equations(P, mask, q, t, acc, sh_part, sh_tot);
  if (!isfinite(acc[20])) return;
  double lambda = 1e-4;
  for (int it = 0; it < a.o.refine_max_iterations; ++it) {
    double d[5], q1[4], t1[3];
    if (!solve_damped<5>(acc, lambda, d)) {
      lambda *= 10.0;
      if (lambda > 1e12) break;
      continue;
    }
    double cur[TV_ACC];                                   // the sums at (q, t), kept while the trial's are formed
#pragma unroll
    for (int c = 0; c < TV_ACC; ++c) cur[c] = acc[c];
    const double cost = acc[20];
    tv_pose_plus(q, t, d, q1, t1);
    tv_normal_equations(P, mask, q1, t1, acc, sh_part, sh_tot);
    if (acc[20] <= cost + TV_COST_SLACK * cost) {
#pragma unroll
      for (int j = 0; j < 4; ++j) q[j] = q1[j];
#pragma unroll
      for (int j = 0; j < 3; ++j) t[j] = t1[j];
      lambda = fmax(lambda * 0.1, 1e-12);
    } else {
#pragma unroll
      for (int c = 0; c < TV_ACC; ++c) acc[c] = cur[c];
      lambda *= 10.0;
      if (lambda > 1e12) break;
    }
    if (sqrt((((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + d[3] * d[3]) + d[4] * d[4]) <= TV_STEP_TOL) break;
  }
}

__global__ __launch_bounds__(PAIR_THREADS) void k_tv_refine(const TvArgs a) {
  __shared__ double sh_rec[PAIR_LDS * PAIR_REC];
  __shared__ double sh_part[PAIR_THREADS * TV_CHUNK];
  __shared__ double sh_tot[TV_ACC];
  const int tid = threadIdx.x;
  const int pi = a.order[blockIdx.x];
  const bool prior = a.prior_qvec != nullptr;
  PairRecords P;
  if (!open_pair<PairThreshold::BothCameras>(a, pi, 5, sh_rec, P)) {   // status 1: written by k_tv_hypotheses unless that did not run
    if (prior && tid == 0) { a.status[pi] = 1; a.n_inliers[pi] = 0; a.n_trials[pi] = 0; }
    return;
  }
  const int n = P.n;
  const double thr2 = P.thr2;
  double q[4], t[3], R[9], E[9];

  if (prior) {
    // the pose is given: no sample, no refinement
    double nq = 0.0, nt = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { q[j] = a.prior_qvec[4 * (size_t)pi + j]; nq += q[j] * q[j]; }
#pragma unroll
    for (int j = 0; j < 3; ++j) { t[j] = a.prior_tvec[3 * (size_t)pi + j]; nt += t[j] * t[j]; }
    if (tid == 0) a.n_trials[pi] = 0;
    if (!(nq > 0.0) || !(nt > 0.0) || !isfinite(nq) || !isfinite(nt)) {
      if (tid == 0) { a.status[pi] = 2; a.n_inliers[pi] = 0; }
      return;
    }
    const double it = 1.0 / sqrt(nt);
#pragma unroll
    for (int j = 0; j < 3; ++j) t[j] *= it;
  } else {
    if (a.winner[3 * (size_t)pi] < 0) return;            // status 2: written by k_tv_hypotheses
    // 2. the winner's inliers, its four poses, the one with the most inliers in front of both cameras
    double E0[9], Ra[9], Rb[9];
#pragma unroll
    for (int m = 0; m < 9; ++m) E0[m] = a.winner_E[9 * (size_t)pi + m];
    const bool have = tv_horn(E0, t, Ra, Rb);
    double front[5] = {0.0, 0.0, 0.0, 0.0, 0.0};         // poses (Ra, t) (Ra, -t) (Rb, t) (Rb, -t); the inlier count
    const double tm[3] = {-t[0], -t[1], -t[2]};
    for (int j = tid; j < n; j += PAIR_THREADS) {
      const double* r = P.rec(j);
      const bool in = tv_sampson(E0, r) <= thr2;
      a.mask_a[P.o0 + j] = in ? 1 : 0;                   // (a lane reads back only what it wrote: j = tid mod 256)
      if (in && have) {
        front[0] += tv_in_front(Ra, t, r) ? 1.0 : 0.0; front[1] += tv_in_front(Ra, tm, r) ? 1.0 : 0.0;
        front[2] += tv_in_front(Rb, t, r) ? 1.0 : 0.0; front[3] += tv_in_front(Rb, tm, r) ? 1.0 : 0.0;
      }
      front[4] += in ? 1.0 : 0.0;
    }
    block_sum<PAIR_THREADS, TV_CHUNK>(front, sh_part, sh_tot);
    if (!have) {
      if (tid == 0) { a.status[pi] = 3; a.n_inliers[pi] = 0; }
      return;
    }
    int pick = 0;
#pragma unroll
    for (int m = 1; m < 4; ++m) if (front[m] > front[pick]) pick = m;
    rotation_to_quat(pick < 2 ? Ra : Rb, q);
    if (pick & 1) { t[0] = tm[0]; t[1] = tm[1]; t[2] = tm[2]; }

    // 3. local optimisation: refine on the inliers, classify again, until the set stands still
    uint8_t* cur = a.mask_a;
    uint8_t* nxt = a.mask_b;
    int cur_cnt = (int)front[4];
    for (int lo = 0; lo < a.o.lo_rounds; ++lo) {
      double q1[4], t1[3], R1[9], E1[9];
#pragma unroll
      for (int j = 0; j < 4; ++j) q1[j] = q[j];
#pragma unroll
      for (int j = 0; j < 3; ++j) t1[j] = t[j];
      tv_refine(a, P, cur, q1, t1, sh_part, sh_tot);
      quat_to_rotation(q1, R1);
      tv_essential_of_pose(R1, t1, E1);
      double cc[2] = {0.0, 0.0};                          // inliers of the refined pose; how many memberships changed
      for (int j = tid; j < n; j += PAIR_THREADS) {
        const bool in = tv_sampson(E1, P.rec(j)) <= thr2;
        nxt[P.o0 + j] = in ? 1 : 0;
        cc[0] += in ? 1.0 : 0.0;
        cc[1] += (in != (cur[P.o0 + j] != 0)) ? 1.0 : 0.0;
      }
      block_sum<PAIR_THREADS, TV_CHUNK>(cc, sh_part, sh_tot);
      if (cc[0] < (double)cur_cnt) break;                 // fewer inliers: the pose before it stays
#pragma unroll
      for (int j = 0; j < 4; ++j) q[j] = q1[j];
#pragma unroll
      for (int j = 0; j < 3; ++j) t[j] = t1[j];
      uint8_t* sw = cur; cur = nxt; nxt = sw;
      cur_cnt = (int)cc[0];
      if (cc[1] == 0.0) break;
    }
  }

  // 4. the final set: Sampson error <= thr^2 under E = [t]x R of the pose that stays
  quat_to_rotation(q, R);
  tv_essential_of_pose(R, t, E);
  double fin[1] = {0.0};
  for (int j = tid; j < n; j += PAIR_THREADS) fin[0] += tv_sampson(E, P.rec(j)) <= thr2 ? 1.0 : 0.0;
  block_sum<PAIR_THREADS, TV_CHUNK>(fin, sh_part, sh_tot);
  const int n_in = (int)fin[0];
  const int need = max(a.o.min_num_inliers, (int)ceil(a.o.min_inlier_ratio * (double)n));
  if (n_in < need) {
    if (tid == 0) { a.status[pi] = 3; a.n_inliers[pi] = 0; }
    return;
  }
  const double to_px = a.o.max_error / P.thr;
  for (int j = tid; j < n; j += PAIR_THREADS) {
    const double e2 = tv_sampson(E, P.rec(j));
    const int64_t i = P.o0 + a.pos[P.o0 + j];
    a.err[i] = sqrt(e2) * to_px;
    a.inlier[i] = e2 <= thr2 ? 1 : 0;
  }
  if (tid == 0) {
    if (prior) {                                          // returned as it came
      for (int j = 0; j < 4; ++j) a.qvec[4 * (size_t)pi + j] = a.prior_qvec[4 * (size_t)pi + j];
      for (int j = 0; j < 3; ++j) a.tvec[3 * (size_t)pi + j] = a.prior_tvec[3 * (size_t)pi + j];
    } else {
      const double sgn = q[0] < 0.0 ? -1.0 : 1.0;
      for (int j = 0; j < 4; ++j) a.qvec[4 * (size_t)pi + j] = sgn * q[j];
      for (int j = 0; j < 3; ++j) a.tvec[3 * (size_t)pi + j] = t[j];
    }
    for (int j = 0; j < 9; ++j) a.E[9 * (size_t)pi + j] = E[j];
    a.status[pi] = 0; a.n_inliers[pi] = n_in;
  }
}

static int two_view_geometry(pxr_ctx* ctx, int32_t n_pairs, const int64_t* d_pair_offsets, int64_t n_matches, const double* d_xy1,
                             const double* d_xy2, const int32_t* d_pair_camera, int32_t n_cameras, const int32_t* d_cam_model,
                             const double* d_cam_params, const double* d_prior_qvec, const double* d_prior_tvec,
                             const pxr_two_view_options* o, double* d_qvec, double* d_tvec, double* d_E, int32_t* d_status,
                             int32_t* d_n_inliers, int32_t* d_n_trials, uint8_t* d_inlier, double* d_err, double* h_ms) {
  const PairCall c = {"pxr_two_view_geometry", ctx, n_pairs, d_pair_offsets, n_matches, d_xy1, d_xy2, d_pair_camera, n_cameras, d_cam_model,
                      d_cam_params, o, d_status, d_n_inliers, d_n_trials, d_inlier, d_err, h_ms};
  const bool priors_paired = (d_prior_qvec == nullptr) == (d_prior_tvec == nullptr);
  PairBatch b;
  if (int rc = open_pair_batch(c, d_qvec && d_tvec && d_E, priors_paired ? nullptr : "prior_qvec and prior_tvec go together", 3, b)) return rc;
  if (n_pairs == 0) return PXR_OK;
  TvArgs a;
  fill_pair_args(a, c, b);
  a.winner_E = b.winner_model;
  a.prior_qvec = d_prior_qvec; a.prior_tvec = d_prior_tvec;
  a.qvec = d_qvec; a.tvec = d_tvec; a.E = d_E;
  if (!d_prior_qvec) hipLaunchKernelGGL(k_tv_hypotheses, dim3((unsigned)n_pairs), dim3(PAIR_THREADS), 0, ctx->stream, a);
  b.timer->mark(3);
  hipLaunchKernelGGL(k_tv_refine, dim3((unsigned)n_pairs), dim3(PAIR_THREADS), 0, ctx->stream, a);
  return close_pair_batch(b, "k_tv_refine launch");
}

}  // namespace pxr

extern "C" void pxr_two_view_default_options(pxr_two_view_options* o) { pxr::pair_default_options(o); }

extern "C" int pxr_two_view_geometry(pxr_ctx* ctx, int32_t n_pairs, const int64_t* d_pair_offsets, int64_t n_matches, const double* d_xy1,
                                     const double* d_xy2, const int32_t* d_pair_camera, int32_t n_cameras, const int32_t* d_cam_model,
                                     const double* d_cam_params, const double* d_prior_qvec, const double* d_prior_tvec,
                                     const pxr_two_view_options* options, double* d_qvec, double* d_tvec, double* d_E, int32_t* d_status,
                                     int32_t* d_n_inliers, int32_t* d_n_trials, uint8_t* d_inlier, double* d_err) {
  return pxr::two_view_geometry(ctx, n_pairs, d_pair_offsets, n_matches, d_xy1, d_xy2, d_pair_camera, n_cameras, d_cam_model, d_cam_params,
                                d_prior_qvec, d_prior_tvec, options, d_qvec, d_tvec, d_E, d_status, d_n_inliers, d_n_trials, d_inlier,
                                d_err, nullptr);
}

extern "C" int pxr_two_view_geometry_timed(pxr_ctx* ctx, int32_t n_pairs, const int64_t* d_pair_offsets, int64_t n_matches,
                                           const double* d_xy1, const double* d_xy2, const int32_t* d_pair_camera, int32_t n_cameras,
                                           const int32_t* d_cam_model, const double* d_cam_params, const double* d_prior_qvec,
                                           const double* d_prior_tvec, const pxr_two_view_options* options, double* d_qvec, double* d_tvec,
                                           double* d_E, int32_t* d_status, int32_t* d_n_inliers, int32_t* d_n_trials, uint8_t* d_inlier,
                                           double* d_err, double* h_kernel_ms) {
  PXR_REQUIRE(h_kernel_ms, "pxr_two_view_geometry_timed: NULL h_kernel_ms");
  return pxr::two_view_geometry(ctx, n_pairs, d_pair_offsets, n_matches, d_xy1, d_xy2, d_pair_camera, n_cameras, d_cam_model, d_cam_params,
                                d_prior_qvec, d_prior_tvec, options, d_qvec, d_tvec, d_E, d_status, d_n_inliers, d_n_trials, d_inlier,
                                d_err, h_kernel_ms);
}
