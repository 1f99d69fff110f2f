// pxr_homography.hip -- batched homography estimation on gfx950: the matches of many image pairs -> one homography, one
// rotation-only model and one inlier mask each.
//
// The planar / panoramic half of COLMAP's two-view geometry estimation (pycolmap.verify_matches classifies a pair from the ratio
// of homography inliers to essential-matrix inliers), for calibrated cameras: undistort both pixels of every match, estimate a
// homography of the normalised plane robustly from minimal samples (four points), refine it on its inliers, then fit the
// rotation-only model H = R to those inliers and count who agrees with it.  Built from the shared core of pxr_robust.h and
// pxr_batch.h like the essential-matrix estimator (pxr_twoview.hip): no random state -- sample h of a pair
// is a counter-based hash of (seed, h) -- and every choice is a comparison of keys, so the result is a function of the pair's own
// matches alone, bit for bit, alone or inside any batch.
//
//   k_hg_records     one lane per match: its pair (binary search of the offsets), undistort both sides -> record (x1, y1, x2, y2)
//   k_compact_records<4>  (pxr_robust.h) one lane per pair: the usable records of a pair moved to the front of its slice
//   k_hg_hypotheses  one workgroup of 256 lanes per pair, the first HG_LDS records staged in LDS; a round of samples per
//                    wavefront, a sample per lane, every lane scoring its own homography against all records
//   k_hg_refine      the winner's local optimisation, the final classification and the rotation-only model
//
// Where the solver's state lives: the 8 x 9 system is a private array indexed by pivot rows and columns, i.e. scratch memory
// (figures: DESIGN.md section 22); the homography itself is in registers for the scoring walk.
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

constexpr int HG_THREADS = 256;
constexpr int HG_WAVES = HG_THREADS / 64;
constexpr int HG_REC = 4;                              // doubles per record: x1, y1, x2, y2 (normalised image points)
constexpr int HG_LDS = PXR_TWOVIEW_LDS_MATCHES;        // records of a pair staged in LDS (32 B each); the rest is read from global memory (L2)
constexpr int HG_ACC = 45;                             // the refinement's sums: J^t J (36, upper triangle by rows), g (8), cost
constexpr int HG_ROT_ACC = 10;                         // those of the rotation-only model: 6, 3, cost
constexpr int HG_CHUNK = 9;                            // of which this many cross the workgroup at a time (HG_THREADS x HG_CHUNK doubles of LDS)
constexpr double HG_PIVOT_TOL = 1e-12;                 // a pivot counts as zero below this fraction of the system's largest entry
constexpr double HG_ROW_TOL = 1e-12;                   // a Gram-Schmidt row counts as zero at this norm
constexpr double HG_STEP_TOL = 1e-12;                  // a refinement stops at a step of this norm
constexpr double HG_COST_SLACK = 1e-12;                // a step is kept unless the cost grows by more than this fraction

// ---- the four-point solver ---------------------------------------------------------------------------------------------------------
// rec: the records (x1, y1, x2, y2) of a sample.  H (row-major, Frobenius norm 1) with H[2] . (x1, y1, 1) > 0 on all four.
// false: no hypothesis (vanishing pivot, a value that is not finite, third components of mixed sign or zero).
__device__ inline bool hg_four_point(const double* const* rec, double H[9]) {
  double A[8 * 9];
  int perm[9];
  for (int m = 0; m < 4; ++m) {
    const double x1 = rec[m][0], y1 = rec[m][1], x2 = rec[m][2], y2 = rec[m][3];
    double* a = A + 2 * m * 9;
    a[0] = 0.0; a[1] = 0.0; a[2] = 0.0; a[3] = -x1; a[4] = -y1; a[5] = -1.0; a[6] = y2 * x1; a[7] = y2 * y1; a[8] = y2;
    a += 9;
    a[0] = x1; a[1] = y1; a[2] = 1.0; a[3] = 0.0; a[4] = 0.0; a[5] = 0.0; a[6] = -(x2 * x1); a[7] = -(x2 * y1); a[8] = -x2;
  }
  double S = 0.0;
  for (int x = 0; x < 72; ++x) S = fmax(S, fabs(A[x]));
  if (!isfinite(S)) return false;
  for (int k = 0; k < 9; ++k) perm[k] = k;
  for (int c = 0; c < 8; ++c) {                          // Gauss-Jordan with full pivoting -> [I | C] in permuted columns
    int pr = c, pc = c;
    double pa = fabs(A[c * 9 + c]);
    for (int r = c; r < 8; ++r)
      for (int k = c; k < 9; ++k) {
        const double v = fabs(A[r * 9 + k]);
        if (v > pa) { pa = v; pr = r; pc = k; }
      }
    if (!(pa > HG_PIVOT_TOL * S)) return false;
    if (pr != c)
      for (int k = 0; k < 9; ++k) { const double v = A[c * 9 + k]; A[c * 9 + k] = A[pr * 9 + k]; A[pr * 9 + k] = v; }
    if (pc != c) {
      for (int r = 0; r < 8; ++r) { const double v = A[r * 9 + c]; A[r * 9 + c] = A[r * 9 + pc]; A[r * 9 + pc] = v; }
      const int v = perm[c]; perm[c] = perm[pc]; perm[pc] = v;
    }
    const double p = A[c * 9 + c];
    for (int k = c; k < 9; ++k) A[c * 9 + k] = A[c * 9 + k] / p;
    for (int r = 0; r < 8; ++r) {
      if (r == c) continue;
      const double f = A[r * 9 + c];
      for (int k = c + 1; k < 9; ++k) A[r * 9 + k] = A[r * 9 + k] - f * A[c * 9 + k];
      A[r * 9 + c] = 0.0;
    }
  }
  double v[9];
  for (int r = 0; r < 8; ++r) v[perm[r]] = -A[r * 9 + 8];
  v[perm[8]] = 1.0;
  double d = 0.0;
  for (int m = 0; m < 9; ++m) d += v[m] * v[m];
  const double nrm = sqrt(d);
  if (!(nrm > 0.0) || !isfinite(nrm)) return false;
  for (int m = 0; m < 9; ++m) H[m] = v[m] / nrm;
  int pos = 0, neg = 0;
  for (int m = 0; m < 4; ++m) {
    const double w = (H[6] * rec[m][0] + H[7] * rec[m][1]) + H[8];
    pos += w > 0.0 ? 1 : 0;
    neg += w < 0.0 ? 1 : 0;
  }
  if (neg == 4) {
    for (int m = 0; m < 9; ++m) H[m] = -H[m];
  } else if (pos != 4) {
    return false;
  }
  return true;
}

// squared forward transfer error of record r under H, in image 2: |pi(H x1) - x2|^2; +inf where the third component is <= 0
// (NaN where it is not a number)
__device__ __forceinline__ double hg_transfer(const double* H, const double* r) {
  const double x1 = r[0], y1 = r[1];
  const double X = (H[0] * x1 + H[1] * y1) + H[2], Y = (H[3] * x1 + H[4] * y1) + H[5], W = (H[6] * x1 + H[7] * y1) + H[8];
  if (W <= 0.0) return pos_inf();
  const double dx = X / W - r[2], dy = Y / W - r[3];
  return dx * dx + dy * dy;
}

// ---- kernel A: records -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HG_THREADS) void k_hg_records(int64_t n_matches, int32_t n_pairs, const int64_t* __restrict__ offsets,
                                                           const int32_t* __restrict__ pair_camera, const int32_t* __restrict__ cam_model,
                                                           const double* __restrict__ cam_params, const double* __restrict__ xy1,
                                                           const double* __restrict__ xy2, double* __restrict__ rec,
                                                           uint8_t* __restrict__ valid, uint8_t* __restrict__ inlier, double* __restrict__ err) {
  const int64_t i = (int64_t)blockIdx.x * HG_THREADS + threadIdx.x;
  if (i >= n_matches) return;
  int lo = 0, hi = n_pairs;                            // the pair p with offsets[p] <= i < offsets[p + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) / 2;
    if (offsets[mid] <= i) lo = mid; else hi = mid;
  }
  double uv[4];
  bool ok = true;
#pragma unroll
  for (int side = 0; side < 2; ++side) {
    const int cam = pair_camera[2 * (size_t)lo + side];
    double k[PXR_KPAD];
#pragma unroll
    for (int j = 0; j < PXR_KPAD; ++j) k[j] = cam_params[(size_t)cam * PXR_KPAD + j];
    const double* xy = side == 0 ? xy1 : xy2;
    const double x = xy[2 * i], y = xy[2 * i + 1];
    ok = isfinite(x) && isfinite(y) && ok;
    ok = image_to_world(cam_model[cam], k, x, y, uv[2 * side], uv[2 * side + 1]) && ok;
  }
  double* r = rec + (size_t)i * HG_REC;
  r[0] = uv[0]; r[1] = uv[1]; r[2] = uv[2]; r[3] = uv[3];
  valid[i] = ok ? 1 : 0;
  inlier[i] = 0;                                       // what a match keeps unless its pair gets a homography
  err[i] = quiet_nan();
}

// ---- kernel B: the estimator -------------------------------------------------------------------------------------------------------
struct HgArgs {
  const int64_t* offsets; const int32_t* pair_camera; const int32_t* cam_model; const double* cam_params;
  const int32_t* order;        // [n_pairs] pairs by descending match count
  const double* rec;           // [n_matches][HG_REC], compacted per pair
  const int32_t* pos;          // [n_matches]
  const int32_t* n_valid;      // [n_pairs]
  int32_t* winner;             // [n_pairs][2] the best key: count (-1: none), sample
  double* winner_H;            // [n_pairs][9] its homography
  uint8_t* mask_a; uint8_t* mask_b;                   // [n_matches] each: inlier sets of the local optimisation (by compacted position)
  pxr_homography_options o;
  int32_t max_trials;          // o.max_num_trials rounded up to a multiple of o.round_size
  double* H; double* rot_qvec; int32_t* status; int32_t* n_inliers; int32_t* n_rot_inliers; int32_t* n_trials; uint8_t* inlier; double* err;
};

struct HgPair {                // what every lane of the workgroup knows about its pair
  const double* sh; const double* g; int n; int64_t o0;
  double thr, thr2;
  int need;                    // inliers the success rule asks for
  __device__ __forceinline__ const double* rec(int j) const { return j < HG_LDS ? sh + j * HG_REC : g + (size_t)j * HG_REC; }
};

// what every lane of a workgroup needs of its pair; false: fewer than four usable matches
__device__ __forceinline__ bool hg_open_pair(const HgArgs& a, int pi, double* sh_rec, HgPair& P) {
  P.o0 = a.offsets[pi];
  P.n = a.n_valid[pi];
  if (P.n < 4) return false;
  P.g = a.rec + (size_t)P.o0 * HG_REC;
  P.sh = sh_rec;
  for (int x = threadIdx.x; x < min(P.n, HG_LDS) * HG_REC; x += HG_THREADS) sh_rec[x] = P.g[x];
  const int cam2 = a.pair_camera[2 * (size_t)pi + 1];
  P.thr = a.o.max_error / mean_focal(a.cam_model[cam2], a.cam_params + (size_t)cam2 * PXR_KPAD);
  P.thr2 = P.thr * P.thr;
  P.need = max(a.o.min_num_inliers, (int)ceil(a.o.min_inlier_ratio * (double)P.n));
  __syncthreads();
  return true;
}

// Every branch that encloses a barrier or a cross-lane operation is uniform over the workgroup.
__global__ __launch_bounds__(HG_THREADS) void k_hg_hypotheses(const HgArgs a) {
  __shared__ double sh_rec[HG_LDS * HG_REC];
  __shared__ double sh_ksum[HG_WAVES];
  __shared__ int sh_kint[HG_WAVES][3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pi = a.order[blockIdx.x];
  HgPair P;
  if (!hg_open_pair(a, pi, sh_rec, P)) {
    if (tid == 0) { a.status[pi] = 1; a.n_inliers[pi] = 0; a.n_rot_inliers[pi] = 0; a.n_trials[pi] = 0; }
    return;
  }
  const int n = P.n;
  const double thr2 = P.thr2;

  // hypotheses: round r (round_size samples) on wavefront r mod 4, its samples strided over the lanes
  HypKey best = {-1, 0.0, 0x7fffffff, 0};
  int done = 0;
  const int floor_cnt = P.need;
  const auto need = [&](int cnt) {                       // the stop rule: four inliers in a sample, at no fewer inliers than success asks for
    const int eff = max(cnt, floor_cnt);
    double w = (double)eff / (double)n;
    if (w > 1.0) w = 1.0;
    return trials_needed(a.o.confidence, a.o.min_num_trials, a.max_trials, eff, (w * w) * (w * w));
  };
  for (int pass = 0;; ++pass) {
    const int round = pass * HG_WAVES + wave;
    HypKey mine = {-1, 0.0, 0x7fffffff, 0};
    if ((int64_t)round * a.o.round_size < a.max_trials) {
      for (int s = lane; s < a.o.round_size; s += 64) {
        const int h = round * a.o.round_size + s;
        int idx[4];
        sample_distinct<4>(a.o.seed, h, n, idx);
        const double* four[4] = {P.rec(idx[0]), P.rec(idx[1]), P.rec(idx[2]), P.rec(idx[3])};
        double H[9];
        if (!hg_four_point(four, H)) continue;
        int cnt = 0;
        double sum = 0.0;
        for (int j = 0; j < n; ++j) {
          const double e2 = hg_transfer(H, P.rec(j));
          double e = thr2;
          if (e2 <= thr2) { ++cnt; e = e2; }
          sum += e;
        }
        const HypKey key = {cnt, sum, h, 0};
        if (key.beats(mine)) mine = key;
      }
    }
    wave_best(mine);
    if (merge_rounds<HG_WAVES>(sh_ksum, sh_kint, mine, pass, a.o.round_size, a.max_trials, best, done, need)) break;
  }
  if (tid == 0) {
    a.n_trials[pi] = done;
    a.winner[2 * (size_t)pi] = best.cnt; a.winner[2 * (size_t)pi + 1] = best.h;
    if (best.cnt < 0) {
      a.status[pi] = 2; a.n_inliers[pi] = 0; a.n_rot_inliers[pi] = 0;
    } else {                                             // the winner's homography: its own arithmetic again, on one lane
      int idx[4];
      sample_distinct<4>(a.o.seed, best.h, n, idx);
      const double* four[4] = {P.rec(idx[0]), P.rec(idx[1]), P.rec(idx[2]), P.rec(idx[3])};
      double H[9];
      hg_four_point(four, H);
      for (int m = 0; m < 9; ++m) a.winner_H[9 * (size_t)pi + m] = H[m];
    }
  }
}

// ---- kernel C: local optimisation, classification, the rotation-only model ----------------------------------------------------------
// sums of J^t J, J^t r and r^2 over the records of `mask`; r = pi(H x1) - x2 (two residuals per record), J = dr / d(the eight
// entries of H other than `fixed`, in index order).  A record whose third component is not positive makes the cost +inf.
__device__ __forceinline__ void hg_normal_equations(const HgPair& P, const uint8_t* mask, const double* H, int fixed,
                                                    double (&acc)[HG_ACC], double* sh_part, double* sh_tot) {
#pragma unroll
  for (int c = 0; c < HG_ACC; ++c) acc[c] = 0.0;
  for (int j = threadIdx.x; j < P.n; j += HG_THREADS) {
    if (!mask[P.o0 + j]) continue;
    const double* r = P.rec(j);
    const double x1 = r[0], y1 = r[1];
    const double X = (H[0] * x1 + H[1] * y1) + H[2], Y = (H[3] * x1 + H[4] * y1) + H[5], W = (H[6] * x1 + H[7] * y1) + H[8];
    if (!(W > 0.0) || !isfinite(W)) { acc[44] = pos_inf(); continue; }
    const double px = X / W, py = Y / W;
    const double r0 = px - r[2], r1 = py - r[3];
    const double a0 = x1 / W, a1 = y1 / W, a2 = 1.0 / W;
    const double J0[9] = {a0, a1, a2, 0.0, 0.0, 0.0, -(px * a0), -(px * a1), -(px * a2)};
    const double J1[9] = {0.0, 0.0, 0.0, a0, a1, a2, -(py * a0), -(py * a1), -(py * a2)};
    double K0[8], K1[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) { K0[m] = m < fixed ? J0[m] : J0[m + 1]; K1[m] = m < fixed ? J1[m] : J1[m + 1]; }
    int x = 0;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
#pragma unroll
      for (int l = m; l < 8; ++l) { acc[x] += K0[m] * K0[l] + K1[m] * K1[l]; ++x; }
      acc[36 + m] += K0[m] * r0 + K1[m] * r1;
    }
    acc[44] += r0 * r0 + r1 * r1;
  }
  block_sum<HG_THREADS, HG_CHUNK>(acc, sh_part, sh_tot);
}

// the same for H = R(q) over the rotation tangent (3): R(d) = R(2 d) R, so dp / dd_c = 2 e_c x p with p = R x1
__device__ __forceinline__ void hg_rot_normal_equations(const HgPair& P, const uint8_t* mask, const double* q,
                                                        double (&acc)[HG_ROT_ACC], double* sh_part, double* sh_tot) {
#pragma unroll
  for (int c = 0; c < HG_ROT_ACC; ++c) acc[c] = 0.0;
  double R[9];
  quat_to_rotation(q, R);
  for (int j = threadIdx.x; j < P.n; j += HG_THREADS) {
    if (!mask[P.o0 + j]) continue;
    const double* r = P.rec(j);
    const double x1 = r[0], y1 = r[1];
    const double X = (R[0] * x1 + R[1] * y1) + R[2], Y = (R[3] * x1 + R[4] * y1) + R[5], W = (R[6] * x1 + R[7] * y1) + R[8];
    if (!(W > 0.0) || !isfinite(W)) { acc[9] = pos_inf(); continue; }
    const double px = X / W, py = Y / W;
    const double r0 = px - r[2], r1 = py - r[3];
    const double iw = 1.0 / W;
    // dr0 / dp = (1, 0, -px) / W, dr1 / dp = (0, 1, -py) / W; 2 e_c x p = (0, -2 W, 2 Y), (2 W, 0, -2 X), (-2 Y, 2 X, 0)
    const double J0[3] = {-(px * (2.0 * Y)) * iw, (2.0 * W + px * (2.0 * X)) * iw, -(2.0 * Y) * iw};
    const double J1[3] = {-(2.0 * W + py * (2.0 * Y)) * iw, (py * (2.0 * X)) * iw, (2.0 * X) * iw};
    int x = 0;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
#pragma unroll
      for (int l = m; l < 3; ++l) { acc[x] += J0[m] * J0[l] + J1[m] * J1[l]; ++x; }
      acc[6 + m] += J0[m] * r0 + J1[m] * r1;
    }
    acc[9] += r0 * r0 + r1 * r1;
  }
  block_sum<HG_THREADS, HG_CHUNK>(acc, sh_part, sh_tot);
}

// Levenberg-Marquardt over D parameters on a state of NS doubles, refined in place: sums(x, acc) forms the normal equations at
// x, plus(x, d, x1) moves it.  The lambda schedule and the keep / refuse rule of sections 19 and 21.  Every lane holds the same
// sums, so every lane takes the same decisions and ends with the same state.
template <int D, int NS, class Sums, class Plus>
__device__ __forceinline__ void hg_lm(int max_iterations, double (&x)[NS], Sums sums, Plus plus) {
  constexpr int NA = D * (D + 1) / 2 + D + 1;
  double acc[NA];
  sums(x, acc);
  if (!isfinite(acc[NA - 1])) return;
  double lambda = 1e-4;
  for (int it = 0; it < max_iterations; ++it) {
    double d[D], x1[NS];
    if (!solve_damped<D>(acc, lambda, d)) {
      lambda *= 10.0;
      if (lambda > 1e12) break;
      continue;
    }
    double cur[NA];                                       // the sums at x, kept while the trial's are formed
#pragma unroll
    for (int c = 0; c < NA; ++c) cur[c] = acc[c];
    const double cost = acc[NA - 1];
    plus(x, d, x1);
    sums(x1, acc);
    if (acc[NA - 1] <= cost + HG_COST_SLACK * cost) {
#pragma unroll
      for (int j = 0; j < NS; ++j) x[j] = x1[j];
      lambda = fmax(lambda * 0.1, 1e-12);
    } else {
#pragma unroll
      for (int c = 0; c < NA; ++c) acc[c] = cur[c];
      lambda *= 10.0;
      if (lambda > 1e12) break;
    }
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < D; ++j) s += d[j] * d[j];
    if (sqrt(s) <= HG_STEP_TOL) break;
  }
}

__global__ __launch_bounds__(HG_THREADS) void k_hg_refine(const HgArgs a) {
  __shared__ double sh_rec[HG_LDS * HG_REC];
  __shared__ double sh_part[HG_THREADS * HG_CHUNK];
  __shared__ double sh_tot[HG_ACC];
  const int tid = threadIdx.x;
  const int pi = a.order[blockIdx.x];
  HgPair P;
  if (!hg_open_pair(a, pi, sh_rec, P)) return;           // status 1: written by k_hg_hypotheses
  if (a.winner[2 * (size_t)pi] < 0) return;              // status 2: written by k_hg_hypotheses
  const int n = P.n;
  const double thr2 = P.thr2;
  double H[9];
#pragma unroll
  for (int m = 0; m < 9; ++m) H[m] = a.winner_H[9 * (size_t)pi + m];

  // 1. the winner's inliers
  uint8_t* cur = a.mask_a;
  uint8_t* nxt = a.mask_b;
  double first[1] = {0.0};
  for (int j = tid; j < n; j += HG_THREADS) {
    const bool in = hg_transfer(H, P.rec(j)) <= thr2;
    cur[P.o0 + j] = in ? 1 : 0;                          // (a lane reads back only what it wrote: j = tid mod 256)
    first[0] += in ? 1.0 : 0.0;
  }
  block_sum<HG_THREADS, HG_CHUNK>(first, sh_part, sh_tot);
  int cur_cnt = (int)first[0];

  // 2. local optimisation: refine on the inliers, classify again, until the set stands still
  for (int lo = 0; lo < a.o.lo_rounds; ++lo) {
    double H1[9];
    int fixed = 0;                                       // the entry of largest magnitude, the first of equals
#pragma unroll
    for (int m = 0; m < 9; ++m) { H1[m] = H[m]; if (fabs(H[m]) > fabs(H[fixed])) fixed = m; }
    const uint8_t* mask = cur;
    hg_lm<8, 9>(a.o.refine_max_iterations, H1,
                [&](const double* x, double (&acc)[HG_ACC]) { hg_normal_equations(P, mask, x, fixed, acc, sh_part, sh_tot); },
                [&](const double* x, const double* d, double* x1) {
#pragma unroll
                  for (int m = 0; m < 9; ++m) x1[m] = m == fixed ? x[m] : x[m] + d[m < fixed ? m : m - 1];
                });
    double s = 0.0;
#pragma unroll
    for (int m = 0; m < 9; ++m) s += H1[m] * H1[m];
    const double nrm = sqrt(s);
#pragma unroll
    for (int m = 0; m < 9; ++m) H1[m] = H1[m] / nrm;
    double cc[2] = {0.0, 0.0};                            // inliers of the refined homography; how many memberships changed
    for (int j = tid; j < n; j += HG_THREADS) {
      const bool in = hg_transfer(H1, P.rec(j)) <= thr2;
      nxt[P.o0 + j] = in ? 1 : 0;
      cc[0] += in ? 1.0 : 0.0;
      cc[1] += (in != (cur[P.o0 + j] != 0)) ? 1.0 : 0.0;
    }
    block_sum<HG_THREADS, HG_CHUNK>(cc, sh_part, sh_tot);
    if (!(cc[0] >= (double)cur_cnt)) break;               // fewer inliers: the homography before it stays
#pragma unroll
    for (int m = 0; m < 9; ++m) H[m] = H1[m];
    uint8_t* sw = cur; cur = nxt; nxt = sw;
    cur_cnt = (int)cc[0];
    if (cc[1] == 0.0) break;
  }

  // 3. the final set (`cur`: the classification under the H that stays) and the success rule
  if (cur_cnt < P.need) {
    if (tid == 0) { a.status[pi] = 3; a.n_inliers[pi] = 0; a.n_rot_inliers[pi] = 0; }
    return;
  }
  const double to_px = a.o.max_error / P.thr;
  for (int j = tid; j < n; j += HG_THREADS) {
    const double e2 = hg_transfer(H, P.rec(j));
    const int64_t i = P.o0 + a.pos[P.o0 + j];
    a.err[i] = isfinite(e2) ? sqrt(e2) * to_px : quiet_nan();
    a.inlier[i] = e2 <= thr2 ? 1 : 0;
  }

  // 4. the rotation-only model: H with a positive determinant -> R0 by modified Gram-Schmidt on its rows -> refined on the
  //    inliers of H -> all n classified under R
  const double det = (H[0] * (H[4] * H[8] - H[5] * H[7]) - H[1] * (H[3] * H[8] - H[5] * H[6])) + H[2] * (H[3] * H[7] - H[4] * H[6]);
  const double sg = det < 0.0 ? -1.0 : 1.0;
  double R0[9], q[4];
  const double g0[3] = {sg * H[0], sg * H[1], sg * H[2]};
  double g1[3] = {sg * H[3], sg * H[4], sg * H[5]};
  const double n0 = sqrt(dot3(g0, g0));
  bool have = n0 > HG_ROW_TOL;
  if (have) {
#pragma unroll
    for (int j = 0; j < 3; ++j) R0[j] = g0[j] / n0;
    const double d01 = dot3(g1, R0);
#pragma unroll
    for (int j = 0; j < 3; ++j) g1[j] = g1[j] - d01 * R0[j];
    const double n1 = sqrt(dot3(g1, g1));
    have = n1 > HG_ROW_TOL;
    if (have) {
#pragma unroll
      for (int j = 0; j < 3; ++j) R0[3 + j] = g1[j] / n1;
      cross3(R0, R0 + 3, R0 + 6);
    }
  }
  int n_rot = 0;
  if (have) {                                            // (uniform: every lane holds the same H)
    rotation_to_quat(R0, q);
    const uint8_t* mask = cur;
    hg_lm<3, 4>(a.o.refine_max_iterations, q,
                [&](const double* x, double (&acc)[HG_ROT_ACC]) { hg_rot_normal_equations(P, mask, x, acc, sh_part, sh_tot); },
                [&](const double* x, const double* d, double* x1) { quat_plus(x, d, x1); });
    double R[9];
    quat_to_rotation(q, R);
    double rc[1] = {0.0};
    for (int j = tid; j < n; j += HG_THREADS) rc[0] += hg_transfer(R, P.rec(j)) <= thr2 ? 1.0 : 0.0;
    block_sum<HG_THREADS, HG_CHUNK>(rc, sh_part, sh_tot);
    n_rot = (int)rc[0];
  }
  if (tid == 0) {
    for (int j = 0; j < 9; ++j) a.H[9 * (size_t)pi + j] = H[j];
    if (have) {
      const double sgn = q[0] < 0.0 ? -1.0 : 1.0;
      for (int j = 0; j < 4; ++j) a.rot_qvec[4 * (size_t)pi + j] = sgn * q[j];
    }
    a.status[pi] = 0; a.n_inliers[pi] = cur_cnt; a.n_rot_inliers[pi] = n_rot;
  }
}

static int homography(pxr_ctx* ctx, int32_t n_pairs, const int64_t* d_pair_offsets, int64_t n_matches, const double* d_xy1,
                      const double* d_xy2, const int32_t* d_pair_camera, int32_t n_cameras, const int32_t* d_cam_model,
                      const double* d_cam_params, const pxr_homography_options* o, double* d_H, double* d_rot_qvec, int32_t* d_status,
                      int32_t* d_n_inliers, int32_t* d_n_rot_inliers, int32_t* d_n_trials, uint8_t* d_inlier, double* d_err, double* h_ms) {
  const char* fn = "pxr_homography";
  PXR_REQUIRE(ctx && o, "%s: NULL argument", fn);
  PXR_REQUIRE(n_pairs >= 0 && n_matches >= 0 && n_cameras >= 0, "%s: negative size", fn);
  PXR_REQUIRE(n_matches < ((int64_t)1 << 31), "%s: more than 2^31 matches", fn);
  PXR_REQUIRE(n_pairs == 0 || (d_pair_offsets && d_pair_camera && d_H && d_rot_qvec && d_status && d_n_inliers && d_n_rot_inliers &&
                               d_n_trials && d_cam_model && d_cam_params), "%s: NULL pair / camera array", fn);
  PXR_REQUIRE(n_matches == 0 || (d_xy1 && d_xy2 && d_inlier && d_err), "%s: NULL match array", fn);
  PXR_REQUIRE(o->max_error > 0.0 && o->confidence > 0.0 && o->confidence < 1.0 && o->min_inlier_ratio >= 0.0 && o->min_inlier_ratio <= 1.0 &&
                  o->min_num_inliers >= 0 && o->min_num_trials >= 0 && o->max_num_trials >= 1 && o->max_num_trials <= (1 << 20) &&
                  o->round_size >= 1 && o->round_size <= (1 << 20) && o->refine_max_iterations >= 0 && o->lo_rounds >= 0,
              "%s: option out of range", fn);
  if (h_ms) h_ms[0] = h_ms[1] = h_ms[2] = h_ms[3] = 0.0;
  if (n_pairs == 0) {
    PXR_REQUIRE(n_matches == 0, "%s: pair_offsets ends at 0, not at n_matches = %lld", fn, (long long)n_matches);
    return PXR_OK;
  }
  PXR_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int64_t T = n_pairs, N = n_matches;

  // offsets and cameras are validated on a host copy, which also gives the processing order: pairs by descending match count
  std::vector<int64_t> off;
  std::vector<int32_t> order, pcam((size_t)T * 2);
  PXR_HIP(hipMemcpyAsync(pcam.data(), d_pair_camera, sizeof(int32_t) * (size_t)T * 2, hipMemcpyDeviceToHost, st));
  const auto cameras_in_range = [&](int64_t t) {
    for (int side = 0; side < 2; ++side)
      PXR_REQUIRE(pcam[2 * t + side] >= 0 && pcam[2 * t + side] < n_cameras, "%s: pair %lld names a camera outside [0, n_cameras = %d)", fn,
                  (long long)t, (int)n_cameras);
    return (int)PXR_OK;
  };
  if (int rc = batch_order(ctx, {fn, "pair_offsets", "pair", "n_matches"}, false, d_pair_offsets, T, N, off, order, cameras_in_range)) return rc;

  Carver cv;
  const size_t o_rec = cv.take((size_t)N * HG_REC, 8), o_valid = cv.take((size_t)N, 1), o_pos = cv.take((size_t)N, 4);
  const size_t o_ma = cv.take((size_t)N, 1), o_mb = cv.take((size_t)N, 1), o_nv = cv.take((size_t)T, 4), o_order = cv.take((size_t)T, 4);
  const size_t o_win = cv.take((size_t)T * 2, 4), o_winH = cv.take((size_t)T * 9, 8);
  if (int rc = grow_workspace(ctx, cv.bytes)) return rc;
  char* ws = static_cast<char*>(ctx->d_workspace);
  double* rec = (double*)(ws + o_rec);
  uint8_t* valid = (uint8_t*)(ws + o_valid);
  int32_t* pos = (int32_t*)(ws + o_pos);
  int32_t* n_valid = (int32_t*)(ws + o_nv);
  int32_t* d_order = (int32_t*)(ws + o_order);

  StageTimer<5> timer(st, h_ms);                         // records | compact | hypotheses | refine
  if (int rc = timer.create(fn)) return rc;

  auto blocks = [](int64_t n, int per) { return dim3((unsigned)((n + per - 1) / per)); };
  int rc = hip_check(hipMemcpyAsync(d_order, order.data(), sizeof(int32_t) * (size_t)T, hipMemcpyHostToDevice, st), "hipMemcpyAsync");
  if (rc == PXR_OK) rc = hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");      // (`order` may go out of scope)
  if (rc != PXR_OK) return rc;
  timer.mark(0);
  if (N > 0)
    hipLaunchKernelGGL(k_hg_records, blocks(N, HG_THREADS), dim3(HG_THREADS), 0, st, N, n_pairs, d_pair_offsets, d_pair_camera,
                       d_cam_model, d_cam_params, d_xy1, d_xy2, rec, valid, d_inlier, d_err);
  timer.mark(1);
  hipLaunchKernelGGL(k_compact_records<HG_REC>, blocks(T, HG_THREADS), dim3(HG_THREADS), 0, st, T, d_pair_offsets, rec, valid, pos, n_valid);
  timer.mark(2);
  HgArgs a;
  a.offsets = d_pair_offsets; a.pair_camera = d_pair_camera; a.cam_model = d_cam_model; a.cam_params = d_cam_params;
  a.order = d_order; a.rec = rec; a.pos = pos; a.n_valid = n_valid; a.mask_a = (uint8_t*)(ws + o_ma); a.mask_b = (uint8_t*)(ws + o_mb);
  a.o = *o;
  a.max_trials = (int32_t)(((int64_t)o->max_num_trials + o->round_size - 1) / o->round_size * o->round_size);
  a.H = d_H; a.rot_qvec = d_rot_qvec; a.status = d_status; a.n_inliers = d_n_inliers; a.n_rot_inliers = d_n_rot_inliers;
  a.n_trials = d_n_trials; a.inlier = d_inlier; a.err = d_err;
  a.winner = (int32_t*)(ws + o_win); a.winner_H = (double*)(ws + o_winH);
  hipLaunchKernelGGL(k_hg_hypotheses, dim3((unsigned)T), dim3(HG_THREADS), 0, st, a);
  timer.mark(3);
  hipLaunchKernelGGL(k_hg_refine, dim3((unsigned)T), dim3(HG_THREADS), 0, st, a);
  timer.mark(4);
  rc = hip_check(hipGetLastError(), "k_hg_refine launch");
  const int from[4] = {0, 1, 2, 3};
  return rc == PXR_OK ? timer.read(from, 4) : rc;
}

}  // namespace pxr

extern "C" void pxr_homography_default_options(pxr_homography_options* o) {
  if (!o) return;
  o->max_error = 4.0; o->min_inlier_ratio = 0.25; o->confidence = 0.999;
  o->seed = 0; o->min_num_inliers = 15; o->min_num_trials = 64; o->max_num_trials = 10000; o->round_size = 64;
  o->refine_max_iterations = 100; o->lo_rounds = 4;
}

extern "C" int pxr_homography(pxr_ctx* ctx, int32_t n_pairs, const int64_t* d_pair_offsets, int64_t n_matches, const double* d_xy1,
                              const double* d_xy2, const int32_t* d_pair_camera, int32_t n_cameras, const int32_t* d_cam_model,
                              const double* d_cam_params, const pxr_homography_options* options, double* d_H, double* d_rot_qvec,
                              int32_t* d_status, int32_t* d_n_inliers, int32_t* d_n_rot_inliers, int32_t* d_n_trials, uint8_t* d_inlier,
                              double* d_err) {
  return pxr::homography(ctx, n_pairs, d_pair_offsets, n_matches, d_xy1, d_xy2, d_pair_camera, n_cameras, d_cam_model, d_cam_params,
                         options, d_H, d_rot_qvec, d_status, d_n_inliers, d_n_rot_inliers, d_n_trials, d_inlier, d_err, nullptr);
}

extern "C" int pxr_homography_timed(pxr_ctx* ctx, int32_t n_pairs, const int64_t* d_pair_offsets, int64_t n_matches, const double* d_xy1,
                                    const double* d_xy2, const int32_t* d_pair_camera, int32_t n_cameras, const int32_t* d_cam_model,
                                    const double* d_cam_params, const pxr_homography_options* options, double* d_H, double* d_rot_qvec,
                                    int32_t* d_status, int32_t* d_n_inliers, int32_t* d_n_rot_inliers, int32_t* d_n_trials,
                                    uint8_t* d_inlier, double* d_err, double* h_kernel_ms) {
  PXR_REQUIRE(h_kernel_ms, "pxr_homography_timed: NULL h_kernel_ms");
  return pxr::homography(ctx, n_pairs, d_pair_offsets, n_matches, d_xy1, d_xy2, d_pair_camera, n_cameras, d_cam_model, d_cam_params,
                         options, d_H, d_rot_qvec, d_status, d_n_inliers, d_n_rot_inliers, d_n_trials, d_inlier, d_err, h_kernel_ms);
}
