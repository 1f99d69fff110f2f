// pxr_homography.hip -- batched homography estimation on gfx950: the matches of many image pairs -> one homography, one
// rotation-only model and one inlier mask each.
//
// The planar / panoramic half of COLMAP's two-view geometry estimation (pycolmap.verify_matches classifies a pair from the ratio
// of homography inliers to essential-matrix inliers), for calibrated cameras: undistort both pixels of every match, estimate a
// homography of the normalised plane robustly from minimal samples (four points), refine it on its inliers, then fit the
// rotation-only model H = R to those inliers and count who agrees with it.  Records, the opening of a pair, the local
// optimisation and the host side of a call are those of pxr_pairs.h; what is here is the homography's own.
//
//   k_hg_hypotheses  one workgroup of 256 lanes per pair, the first PAIR_LDS records staged in LDS; a round of samples per
//                    wavefront, a sample per lane, every lane scoring its own homography against all records
//   k_hg_refine      the winner's local optimisation, the final classification and the rotation-only model
//
// Where the solver's state lives: the 8 x 9 system is a private array indexed by pivot rows and columns, i.e. scratch memory
// (figures: DESIGN.md section 22); the homography itself is in registers for the scoring walk.
#include <hip/hip_runtime.h>

#include <cmath>

#include "pxr_device.h"
#include "pxr_pairs.h"

namespace pxr {

constexpr int HG_ACC = 45;                             // the refinement's sums: J^t J (36, upper triangle by rows), g (8), cost
constexpr int HG_ROT_ACC = 10;                         // those of the rotation-only model: 6, 3, cost
constexpr int HG_CHUNK = 9;                            // of which this many cross the workgroup at a time (PAIR_THREADS x HG_CHUNK doubles of LDS)
constexpr double HG_PIVOT_TOL = 1e-12;                 // a pivot counts as zero below this fraction of the system's largest entry
constexpr double HG_ROW_TOL = 1e-12;                   // a Gram-Schmidt row counts as zero at this norm

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

// ---- kernel B: the estimator -------------------------------------------------------------------------------------------------------
struct HgArgs {
  const int64_t* offsets; const int32_t* pair_camera; const int32_t* cam_model; const double* cam_params;
  const int32_t* order;        // [n_pairs] pairs by descending match count
  const double* rec;           // [n_matches][PAIR_REC], compacted per pair
  const int32_t* pos;          // [n_matches]
  const int32_t* n_valid;      // [n_pairs]
  int32_t* winner;             // [n_pairs][2] the best key: count (-1: none), sample
  double* winner_H;            // [n_pairs][9] its homography
  uint8_t* mask_a; uint8_t* mask_b;                   // [n_matches] each: inlier sets of the local optimisation (by compacted position)
  pxr_homography_options o;
  int32_t max_trials;          // o.max_num_trials rounded up to a multiple of o.round_size
  double* H; double* rot_qvec; int32_t* status; int32_t* n_inliers; int32_t* n_rot_inliers; int32_t* n_trials; uint8_t* inlier; double* err;
};

// inliers the success rule asks for of a pair with n usable matches
__device__ __forceinline__ int hg_need(const HgArgs& a, int n) { return max(a.o.min_num_inliers, (int)ceil(a.o.min_inlier_ratio * (double)n)); }

// Every branch that encloses a barrier or a cross-lane operation is uniform over the workgroup.
__global__ __launch_bounds__(PAIR_THREADS) void k_hg_hypotheses(const HgArgs a) {
  __shared__ double sh_rec[PAIR_LDS * PAIR_REC];
  __shared__ double sh_ksum[PAIR_WAVES];
  __shared__ int sh_kint[PAIR_WAVES][3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pi = a.order[blockIdx.x];
  PairRecords P;
  int floor_cnt;
  if (!open_pair<PairThreshold::Camera2>(a, pi, 4, sh_rec, P, [&] { floor_cnt = hg_need(a, P.n); })) {
    if (tid == 0) { a.status[pi] = 1; a.n_inliers[pi] = 0; a.n_rot_inliers[pi] = 0; a.n_trials[pi] = 0; }
    return;
  }
  const int n = P.n;
  const double thr2 = P.thr2;

  // hypotheses: round r (round_size samples) on wavefront r mod 4, its samples strided over the lanes
  HypKey best = {-1, 0.0, 0x7fffffff, 0};
  int done = 0;
  const auto need = [&](int cnt) {                       // the stop rule: four inliers in a sample, at no fewer inliers than success asks for
    const int eff = max(cnt, floor_cnt);
    double w = (double)eff / (double)n;
    if (w > 1.0) w = 1.0;
    return trials_needed(a.o.confidence, a.o.min_num_trials, a.max_trials, eff, (w * w) * (w * w));
  };
  for (int pass = 0;; ++pass) {
    const int round = pass * PAIR_WAVES + wave;
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
    if (merge_rounds<PAIR_WAVES>(sh_ksum, sh_kint, mine, pass, a.o.round_size, a.max_trials, best, done, need)) break;
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
__device__ __forceinline__ void hg_normal_equations(const PairRecords& P, const uint8_t* mask, const double* H, int fixed,
                                                    double (&acc)[HG_ACC], double* sh_part, double* sh_tot) {
#pragma unroll
  for (int c = 0; c < HG_ACC; ++c) acc[c] = 0.0;
  for (int j = threadIdx.x; j < P.n; j += PAIR_THREADS) {
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
  block_sum<PAIR_THREADS, HG_CHUNK>(acc, sh_part, sh_tot);
}

// the same for H = R(q) over the rotation tangent (3): R(d) = R(2 d) R, so dp / dd_c = 2 e_c x p with p = R x1
__device__ __forceinline__ void hg_rot_normal_equations(const PairRecords& P, const uint8_t* mask, const double* q,
                                                        double (&acc)[HG_ROT_ACC], double* sh_part, double* sh_tot) {
#pragma unroll
  for (int c = 0; c < HG_ROT_ACC; ++c) acc[c] = 0.0;
  double R[9];
  quat_to_rotation(q, R);
  for (int j = threadIdx.x; j < P.n; j += PAIR_THREADS) {
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
  block_sum<PAIR_THREADS, HG_CHUNK>(acc, sh_part, sh_tot);
}

__global__ __launch_bounds__(PAIR_THREADS) void k_hg_refine(const HgArgs a) {
  __shared__ double sh_rec[PAIR_LDS * PAIR_REC];
  __shared__ double sh_part[PAIR_THREADS * HG_CHUNK];
  __shared__ double sh_tot[HG_ACC];
  const int tid = threadIdx.x;
  const int pi = a.order[blockIdx.x];
  PairRecords P;
  int need;
  // status 1 and status 2 are written by k_hg_hypotheses
  if (!open_pair<PairThreshold::Camera2>(a, pi, 4, sh_rec, P, [&] { need = hg_need(a, P.n); })) return;
  if (a.winner[2 * (size_t)pi] < 0) return;
  const int n = P.n;
  const double thr2 = P.thr2;
  double H[9];
#pragma unroll
  for (int m = 0; m < 9; ++m) H[m] = a.winner_H[9 * (size_t)pi + m];

  // 1-2. the winner's inliers, then the local optimisation: refine on the inliers, classify again, until the set stands still
  uint8_t* cur = a.mask_a;
  uint8_t* nxt = a.mask_b;
  const int cur_cnt = local_optimisation<HG_CHUNK>(
      P, a.o.lo_rounds, H, cur, nxt, [](const double* M, const double* r) { return hg_transfer(M, r); },
      [&](const double* H0, const uint8_t* mask, double (&H1)[9]) {
        int fixed = 0;                                   // the entry of largest magnitude, the first of equals
#pragma unroll
        for (int m = 0; m < 9; ++m) { H1[m] = H0[m]; if (fabs(H0[m]) > fabs(H0[fixed])) fixed = m; }
        lm_refine<8, 9>(a.o.refine_max_iterations, H1,
                        [&](const double* x, double (&acc)[HG_ACC]) { hg_normal_equations(P, mask, x, fixed, acc, sh_part, sh_tot); },
                        [&](const double* x, const double* d, double* x1) {
#pragma unroll
                          for (int m = 0; m < 9; ++m) x1[m] = m == fixed ? x[m] : x[m] + d[m < fixed ? m : m - 1];
                        });
        return true;
      },
      sh_part, sh_tot);

  // 3. the final set (`cur`: the classification under the H that stays) and the success rule
  if (cur_cnt < need) {
    if (tid == 0) { a.status[pi] = 3; a.n_inliers[pi] = 0; a.n_rot_inliers[pi] = 0; }
    return;
  }
  const double to_px = a.o.max_error / P.thr;
  for (int j = tid; j < n; j += PAIR_THREADS) {
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
    lm_refine<3, 4>(a.o.refine_max_iterations, q,
                [&](const double* x, double (&acc)[HG_ROT_ACC]) { hg_rot_normal_equations(P, mask, x, acc, sh_part, sh_tot); },
                [&](const double* x, const double* d, double* x1) { quat_plus(x, d, x1); });
    double R[9];
    quat_to_rotation(q, R);
    double rc[1] = {0.0};
    for (int j = tid; j < n; j += PAIR_THREADS) rc[0] += hg_transfer(R, P.rec(j)) <= thr2 ? 1.0 : 0.0;
    block_sum<PAIR_THREADS, HG_CHUNK>(rc, sh_part, sh_tot);
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
  const PairCall c = {"pxr_homography", ctx, n_pairs, d_pair_offsets, n_matches, d_xy1, d_xy2, d_pair_camera, n_cameras, d_cam_model,
                      d_cam_params, o, d_status, d_n_inliers, d_n_trials, d_inlier, d_err, h_ms};
  PairBatch b;
  if (int rc = open_pair_batch(c, d_H && d_rot_qvec && d_n_rot_inliers, nullptr, 2, b)) return rc;
  if (n_pairs == 0) return PXR_OK;
  HgArgs a;
  fill_pair_args(a, c, b);
  a.winner_H = b.winner_model;
  a.H = d_H; a.rot_qvec = d_rot_qvec; a.n_rot_inliers = d_n_rot_inliers;
  hipLaunchKernelGGL(k_hg_hypotheses, dim3((unsigned)n_pairs), dim3(PAIR_THREADS), 0, ctx->stream, a);
  b.timer->mark(3);
  hipLaunchKernelGGL(k_hg_refine, dim3((unsigned)n_pairs), dim3(PAIR_THREADS), 0, ctx->stream, a);
  return close_pair_batch(b, "k_hg_refine launch");
}

}  // namespace pxr

extern "C" void pxr_homography_default_options(pxr_homography_options* o) { pxr::pair_default_options(o); }

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
