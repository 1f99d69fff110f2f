// pxr_robust.h -- the device core the batched robust estimators share (pxr_abspose.hip, pxr_twoview.hip, pxr_homography.hip,
// pxr_fundamental.hip; pxr_triangulate.hip takes the constants and the compaction kernel): the counter-hash samples, the
// hypothesis key and its selection across a workgroup, the stop rule, the fixed-order workgroup sum, the damped Cholesky solve,
// the Levenberg-Marquardt loop, the quaternion update and the compaction of usable records.
// Everything here is a function of its arguments alone -- no random state, every choice a comparison of keys -- which is what
// makes an estimator built from it a function of the item's own data, bit for bit, alone or inside any batch (DESIGN.md sections
// 19 and 21).  __shared__ arrays are declared by the kernels and handed down as pointers.
// Not here: the Levenberg-Marquardt and local-optimisation loops of k_abs_refine and k_tv_refine.  Both kernels sit at 256 VGPRs
// with spills, and either loop taken from a template over the estimator's pieces costs each of them spill registers (DESIGN.md
// section 21, "the shared core"); their loops are built from block_sum, solve_damped and quat_plus below and stay written out in
// their kernels.  k_hg_refine and k_fm_refine take lm_refine from here and their local optimisation from pxr_pairs.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pixsfm_hip.h"

namespace pxr {

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ double pos_inf() { return __longlong_as_double(0x7ff0000000000000ll); }

// ---- samples: splitmix64's output function [Steele, Lea, Flood, "Fast splittable pseudorandom number generators", 2014] ---------
__device__ __forceinline__ uint64_t splitmix(uint64_t z) {
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
constexpr int SAMPLE_MAX_DRAWS = 256;                  // draws of one sample before the smallest unused indices complete it

// sample h of an item with n > K usable records: K distinct indices, ascending.  draw d = mix(mix(seed + G (h + 1)) + G (d + 1))
// mod n, the counter d shared by the K indices; a repeated index is drawn again
template <int K>
__device__ __forceinline__ void sample_distinct(uint64_t seed, int64_t h, int n, int idx[K]) {
  const uint64_t G = 0x9E3779B97F4A7C15ull;
  const uint64_t a = splitmix(seed + G * (uint64_t)(h + 1));
  int draw = 0;
  for (int m = 0; m < K; ++m) {
    int c = 0;
    bool fresh = false;
    while (!fresh && draw < SAMPLE_MAX_DRAWS) {
      ++draw;
      c = (int)(splitmix(a + G * (uint64_t)draw) % (uint64_t)n);
      fresh = true;
      for (int l = 0; l < m; ++l) fresh = fresh && idx[l] != c;
    }
    if (!fresh) {                                       // (never in practice: the smallest unused index)
      for (c = 0;; ++c) {
        bool used = false;
        for (int l = 0; l < m; ++l) used = used || idx[l] == c;
        if (!used) break;
      }
    }
    idx[m] = c;
  }
  for (int m = 1; m < K; ++m) {                         // insertion sort
    const int c = idx[m];
    int l = m;
    while (l > 0 && idx[l - 1] > c) { idx[l] = idx[l - 1]; --l; }
    idx[l] = c;
  }
}

// K = 3 written out, the three indices in registers: the same draws and the same fallbacks ("the smallest unused index"), except
// that the third index takes one more draw where the second used up all SAMPLE_MAX_DRAWS (n >= 4: probability <= 4^-255).  This
// text, not the loop above at K = 3, is what keeps k_abs_refine's instructions and time where they were.
template <>
__device__ __forceinline__ void sample_distinct<3>(uint64_t seed, int64_t h, int n, int idx[3]) {
  const uint64_t G = 0x9E3779B97F4A7C15ull;
  const uint64_t a = splitmix(seed + G * (uint64_t)(h + 1));
  int draw = 0;
  auto next = [&]() { ++draw; return (int)(splitmix(a + G * (uint64_t)draw) % (uint64_t)n); };
  const int c0 = next();
  int c1 = next();
  while (c1 == c0 && draw < SAMPLE_MAX_DRAWS) c1 = next();
  if (c1 == c0) c1 = c0 == 0 ? 1 : 0;
  int c2 = next();
  while ((c2 == c0 || c2 == c1) && draw < SAMPLE_MAX_DRAWS) c2 = next();
  if (c2 == c0 || c2 == c1) c2 = (c0 != 0 && c1 != 0) ? 0 : (c0 != 1 && c1 != 1) ? 1 : 2;
  const int lo = min(c0, min(c1, c2)), hi = max(c0, max(c1, c2));
  idx[0] = lo; idx[1] = c0 + c1 + c2 - lo - hi; idx[2] = hi;
}

// ---- small vectors, rotations, cameras -------------------------------------------------------------------------------------------
__device__ __forceinline__ void cross3(const double* a, const double* b, double c[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// unit quaternion (w first) of a (nearly orthogonal) rotation matrix, by the largest of the four pivots
__device__ __forceinline__ void rotation_to_quat(const double* R, double q[4]) {
  const double tr = R[0] + R[4] + R[8];
  if (tr > 0.0) {
    const double s = 2.0 * sqrt(tr + 1.0);
    q[0] = 0.25 * s; q[1] = (R[7] - R[5]) / s; q[2] = (R[2] - R[6]) / s; q[3] = (R[3] - R[1]) / s;
  } else if (R[0] > R[4] && R[0] > R[8]) {
    const double s = 2.0 * sqrt(1.0 + R[0] - R[4] - R[8]);
    q[0] = (R[7] - R[5]) / s; q[1] = 0.25 * s; q[2] = (R[1] + R[3]) / s; q[3] = (R[2] + R[6]) / s;
  } else if (R[4] > R[8]) {
    const double s = 2.0 * sqrt(1.0 + R[4] - R[0] - R[8]);
    q[0] = (R[2] - R[6]) / s; q[1] = (R[1] + R[3]) / s; q[2] = 0.25 * s; q[3] = (R[5] + R[7]) / s;
  } else {
    const double s = 2.0 * sqrt(1.0 + R[8] - R[0] - R[4]);
    q[0] = (R[3] - R[1]) / s; q[1] = (R[2] + R[6]) / s; q[2] = (R[5] + R[7]) / s; q[3] = 0.25 * s;
  }
  const double inv = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
  for (int j = 0; j < 4; ++j) q[j] *= inv;
}

// the quaternion half of x (+) d as the bundle adjustment moves a pose: QuaternionManifold::Plus [upstream Ceres manifold.cc] on
// q0 with the tangent d[0 .. 2]; q1 re-normalised
__device__ __forceinline__ void quat_plus(const double* q0, const double* d, double q1[4]) {
  const double nd = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
#pragma unroll
  for (int j = 0; j < 4; ++j) q1[j] = q0[j];
  if (nd != 0.0) {
    const double sn = sin(nd) / nd;
    const double qd[4] = {cos(nd), sn * d[0], sn * d[1], sn * d[2]};
    q1[0] = qd[0] * q0[0] - qd[1] * q0[1] - qd[2] * q0[2] - qd[3] * q0[3];
    q1[1] = qd[0] * q0[1] + qd[1] * q0[0] + qd[2] * q0[3] - qd[3] * q0[2];
    q1[2] = qd[0] * q0[2] - qd[1] * q0[3] + qd[2] * q0[0] + qd[3] * q0[1];
    q1[3] = qd[0] * q0[3] + qd[1] * q0[2] - qd[2] * q0[1] + qd[3] * q0[0];
  }
  const double inv = 1.0 / sqrt(q1[0] * q1[0] + q1[1] * q1[1] + q1[2] * q1[2] + q1[3] * q1[3]);
#pragma unroll
  for (int j = 0; j < 4; ++j) q1[j] *= inv;
}

// the focal length an error threshold in pixels is divided by: f, or the mean of fx and fy
__device__ __forceinline__ double mean_focal(int model, const double* k) {
  switch (model) {
    case PXR_SIMPLE_PINHOLE: case PXR_SIMPLE_RADIAL: case PXR_RADIAL: case PXR_SIMPLE_RADIAL_FISHEYE: case PXR_RADIAL_FISHEYE:
      return k[0];
    default:
      return 0.5 * (k[0] + k[1]);
  }
}

// ---- hypotheses: the key, its selection across a workgroup, the stop rule ----------------------------------------------------------
struct HypKey {                // larger count, then smaller sum, then smaller sample, then smaller root
  int cnt; double sum; int h; int root;
  __device__ __forceinline__ bool beats(const HypKey& o) const {
    return cnt > o.cnt || (cnt == o.cnt && (sum < o.sum || (sum == o.sum && (h < o.h || (h == o.h && root < o.root)))));
  }
};

// the best key of a wavefront on every lane of it: compared, never accumulated, across the lanes
__device__ __forceinline__ void wave_best(HypKey& mine) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    HypKey other;
    other.cnt = __shfl_xor(mine.cnt, off, 64); other.sum = __shfl_xor(mine.sum, off, 64);
    other.h = __shfl_xor(mine.h, off, 64); other.root = __shfl_xor(mine.root, off, 64);
    if (other.beats(mine)) mine = other;
  }
}

// trials the stop rule asks for at `cnt` inliers; p_all_inliers = the probability that a minimal sample is all inliers at that
// count, formed by the caller (its association is part of the estimator's arithmetic)
__device__ __forceinline__ double trials_needed(double confidence, int min_trials, int max_trials, int cnt, double p_all_inliers) {
  double need = (double)max_trials;
  if (cnt > 0) {
    const double x = log(1.0 - confidence) / log(1.0 - p_all_inliers);      // all inliers: -inf below, x = +0
    if (x < need) need = x;
  }
  if (need < (double)min_trials) need = (double)min_trials;
  if (need > (double)max_trials) need = (double)max_trials;
  return need;
}

// The end of a pass of WAVES rounds (round pass * WAVES + w on wavefront w, `mine` = that round's wave_best): lane 0 of every
// wavefront parks its key in LDS, then every lane merges the rounds of the pass into `best` in round order, with the stop rule
// (need(cnt): trials_needed at cnt) at every round boundary.  Both barriers are met by the whole workgroup; true: stop.
template <int WAVES, class Need>
__device__ __forceinline__ bool merge_rounds(double* sh_ksum, int (*sh_kint)[3], const HypKey& mine, int pass, int round_size,
                                             int max_trials, HypKey& best, int& done, Need need) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { sh_ksum[wave] = mine.sum; sh_kint[wave][0] = mine.cnt; sh_kint[wave][1] = mine.h; sh_kint[wave][2] = mine.root; }
  __syncthreads();
  bool stop = false;
  for (int w = 0; w < WAVES && !stop; ++w) {            // the rounds in order; the stop rule at every round boundary
    if ((int64_t)(pass * WAVES + w) * round_size >= max_trials) { stop = true; break; }
    const HypKey key = {sh_kint[w][0], sh_ksum[w], sh_kint[w][1], sh_kint[w][2]};
    if (key.beats(best)) best = key;
    done = (pass * WAVES + w + 1) * round_size;
    stop = (double)done >= need(best.cnt);
  }
  __syncthreads();
  return stop;
}

// ---- the refinement's pieces -------------------------------------------------------------------------------------------------------
// sums over the workgroup in a fixed order: lane t's addends to sh_part[t] (THREADS x CHUNK doubles), column c summed over
// t = 0 .. THREADS - 1 by lane c into sh_tot (N doubles); every lane ends with the N sums
template <int THREADS, int CHUNK, int N>
__device__ __forceinline__ void block_sum(double (&v)[N], double* sh_part, double* sh_tot) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int c0 = 0; c0 < N; c0 += CHUNK) {
#pragma unroll
    for (int c = 0; c < CHUNK; ++c) if (c0 + c < N) sh_part[tid * CHUNK + c] = v[c0 + c];
    __syncthreads();
    if (tid < CHUNK && c0 + tid < N) {
      double s = 0.0;
      for (int t = 0; t < THREADS; ++t) s += sh_part[t * CHUNK + tid];
      sh_tot[c0 + tid] = s;
    }
    __syncthreads();
  }
#pragma unroll
  for (int c = 0; c < N; ++c) v[c] = sh_tot[c];
}

// (H + lambda diag(H)) d = -g by Cholesky; acc = the upper triangle of H by rows (D (D + 1) / 2), g (D), the cost.
// false: not positive definite
template <int D>
__device__ __forceinline__ bool solve_damped(const double (&acc)[D * (D + 1) / 2 + D + 1], double lambda, double d[D]) {
  constexpr int G0 = D * (D + 1) / 2;
  double L[D][D];
  {
    int c = 0;
#pragma unroll
    for (int m = 0; m < D; ++m)
#pragma unroll
      for (int l = m; l < D; ++l) { L[l][m] = acc[c]; ++c; }
  }
#pragma unroll
  for (int m = 0; m < D; ++m) L[m][m] += lambda * L[m][m];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    double s = L[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
    ok = ok && s > 0.0;
    const double piv = sqrt(s);
    L[j][j] = piv;
#pragma unroll
    for (int i = j + 1; i < D; ++i) {
      double v = L[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
      L[i][j] = v / piv;
    }
  }
  double y[D];
#pragma unroll
  for (int i = 0; i < D; ++i) {
    double v = -acc[G0 + i];
#pragma unroll
    for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
    y[i] = v / L[i][i];
  }
#pragma unroll
  for (int i = D - 1; i >= 0; --i) {
    double v = y[i];
#pragma unroll
    for (int k = i + 1; k < D; ++k) v -= L[k][i] * d[k];
    d[i] = v / L[i][i];
    ok = ok && isfinite(d[i]);
  }
  return ok;
}

// Levenberg-Marquardt over D parameters on a state of NS doubles, refined in place: sums(x, acc) forms the normal equations at
// x (acc as solve_damped takes it), plus(x, d, x1) moves it.  lambda from 1e-4, x 0.1 (not below 1e-12) on a kept step, x 10 on
// a refused or unsolvable one, until lambda > 1e12 (sections 19, 21 and 22).  Every lane holds the same sums, so every lane takes
// the same decisions and ends with the same state.
constexpr double LM_STEP_TOL = 1e-12;                  // a refinement stops at a step of this norm
constexpr double LM_COST_SLACK = 1e-12;                // a step is kept unless the cost grows by more than this fraction
template <int D, int NS, class Sums, class Plus>
__device__ __forceinline__ void lm_refine(int max_iterations, double (&x)[NS], Sums sums, Plus plus) {
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
    if (acc[NA - 1] <= cost + LM_COST_SLACK * cost) {
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
    if (sqrt(s) <= LM_STEP_TOL) break;
  }
}

// ---- records -------------------------------------------------------------------------------------------------------------------------
// The usable records (REC doubles each) of every item moved to the front of the item's slice, order kept (position j <- the j-th
// usable one; a move only ever goes towards the front, so the slice is compacted in place); pos[o0 + j] = where the j-th came from.
// One lane per item, 256 lanes per workgroup.
template <int REC>
__global__ __launch_bounds__(256) void k_compact_records(int64_t n_items, const int64_t* __restrict__ offsets, double* __restrict__ rec,
                                                         const uint8_t* __restrict__ valid, int32_t* __restrict__ pos,
                                                         int32_t* __restrict__ n_valid) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n_items) return;
  const int64_t o0 = offsets[t];
  const int64_t n = offsets[t + 1] - o0;
  int32_t nv = 0;
  for (int64_t j = 0; j < n; ++j) {
    if (!valid[o0 + j]) continue;
    if (nv != j) {
#pragma unroll
      for (int m = 0; m < REC; ++m) rec[(size_t)(o0 + nv) * REC + m] = rec[(size_t)(o0 + j) * REC + m];
    }
    pos[o0 + nv] = (int32_t)j;
    ++nv;
  }
  n_valid[t] = nv;
}

}  // namespace pxr
