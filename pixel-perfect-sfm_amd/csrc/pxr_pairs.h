// pxr_pairs.h -- what the three robust estimators over image pairs share beyond pxr_robust.h and pxr_batch.h (essential matrix:
// pxr_twoview.hip, homography: pxr_homography.hip, fundamental matrix: pxr_fundamental.hip): the record of a match and how a
// workgroup opens its pair, the local optimisation of the homography and fundamental-matrix winners, and the host side of a call
// up to the estimator's own kernels: the checks, the processing order, the workspace, and the two kernels that turn matches into
// per-pair records.  What differs per estimator -- the minimal solver, the error function, the normal equations, the
// parametrisation -- stays in its file.  Header only: an estimator's translation unit is complete with it.
//
//   k_pair_records        one lane per match: its pair (binary search of the offsets), undistort both sides -> record (x1, y1, x2, y2)
//   k_compact_records<4>  (pxr_robust.h) one lane per pair: the usable records of a pair moved to the front of its slice (in
//                         order), positions kept
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <optional>
#include <vector>

#include "pxr_batch.h"
#include "pxr_device.h"
#include "pxr_internal.h"
#include "pxr_robust.h"
#include "pxr_undistort.h"

namespace pxr {

constexpr int PAIR_THREADS = 256;                      // lanes of every workgroup of the three estimators
constexpr int PAIR_WAVES = PAIR_THREADS / 64;
constexpr int PAIR_REC = 4;                            // doubles per record: x1, y1, x2, y2 (normalised image points)
constexpr int PAIR_LDS = PXR_TWOVIEW_LDS_MATCHES;      // records of a pair staged in LDS (32 B each); the rest is read from global memory (L2)

// ---- device: a workgroup and its pair ----------------------------------------------------------------------------------------------
struct PairRecords {           // what every lane of the workgroup knows about its pair
  const double* sh; const double* g; int n; int64_t o0;
  double thr, thr2;
  __device__ __forceinline__ const double* rec(int j) const { return j < PAIR_LDS ? sh + j * PAIR_REC : g + (size_t)j * PAIR_REC; }
};

// the threshold in the normalised plane: max_error over the mean focal length of both cameras, or over that of camera 2 (where
// the error lives in image 2 alone)
enum class PairThreshold { BothCameras, Camera2 };

// what every lane of a workgroup needs of its pair (a: the estimator's TvArgs / HgArgs / FmArgs); false: fewer than min_n usable
// matches.  own(): what the estimator derives from P.n for itself, ahead of the barrier.
template <PairThreshold POLICY, class Args, class Own>
__device__ __forceinline__ bool open_pair(const Args& a, int pi, int min_n, double* sh_rec, PairRecords& P, Own own) {
  P.o0 = a.offsets[pi];
  P.n = a.n_valid[pi];
  if (P.n < min_n) return false;
  P.g = a.rec + (size_t)P.o0 * PAIR_REC;
  P.sh = sh_rec;
  for (int x = threadIdx.x; x < min(P.n, PAIR_LDS) * PAIR_REC; x += PAIR_THREADS) sh_rec[x] = P.g[x];
  if constexpr (POLICY == PairThreshold::BothCameras) {
    const int cam1 = a.pair_camera[2 * (size_t)pi], cam2 = a.pair_camera[2 * (size_t)pi + 1];
    const double f1 = mean_focal(a.cam_model[cam1], a.cam_params + (size_t)cam1 * PXR_KPAD);
    const double f2 = mean_focal(a.cam_model[cam2], a.cam_params + (size_t)cam2 * PXR_KPAD);
    P.thr = 0.5 * (a.o.max_error / f1 + a.o.max_error / f2);
  } else {
    const int cam2 = a.pair_camera[2 * (size_t)pi + 1];
    P.thr = a.o.max_error / mean_focal(a.cam_model[cam2], a.cam_params + (size_t)cam2 * PXR_KPAD);
  }
  P.thr2 = P.thr * P.thr;
  own();
  __syncthreads();
  return true;
}
template <PairThreshold POLICY, class Args>
__device__ __forceinline__ bool open_pair(const Args& a, int pi, int min_n, double* sh_rec, PairRecords& P) {
  return open_pair<POLICY>(a, pi, min_n, sh_rec, P, [] {});
}

// The local optimisation of a winner M (3 x 3, row-major, Frobenius norm 1; every lane holds the same): its inliers under
// err2(M, record) <= thr2 into `cur`; then up to lo_rounds times: refine(M, cur, M1) refines a copy on them (false: no
// parametrisation, M stays), M1 is scaled back to norm 1 and all n are classified under it into `nxt`; fewer inliers: M stays,
// else M1 takes its place and the masks swap; the rounds end when the set stands still.  Returns the inlier count of the M that
// stays, `cur` its classification.  CHUNK: block_sum's, over sh_part / sh_tot.
template <int CHUNK, class Err2, class Refine>
__device__ __forceinline__ int local_optimisation(const PairRecords& P, int lo_rounds, double (&M)[9], uint8_t*& cur, uint8_t*& nxt,
                                                  Err2 err2, Refine refine, double* sh_part, double* sh_tot) {
  const int tid = threadIdx.x, n = P.n;
  const double thr2 = P.thr2;
  double first[1] = {0.0};
  for (int j = tid; j < n; j += PAIR_THREADS) {
    const bool in = err2(M, P.rec(j)) <= thr2;
    cur[P.o0 + j] = in ? 1 : 0;                          // (a lane reads back only what it wrote: j = tid mod 256)
    first[0] += in ? 1.0 : 0.0;
  }
  block_sum<PAIR_THREADS, CHUNK>(first, sh_part, sh_tot);
  int cur_cnt = (int)first[0];
  for (int lo = 0; lo < lo_rounds; ++lo) {
    double M1[9];
    if (!refine(M, cur, M1)) break;                      // (uniform: every lane holds the same M)
    double s = 0.0;
#pragma unroll
    for (int m = 0; m < 9; ++m) s += M1[m] * M1[m];
    const double nrm = sqrt(s);
#pragma unroll
    for (int m = 0; m < 9; ++m) M1[m] = M1[m] / nrm;
    double cc[2] = {0.0, 0.0};                            // inliers of the refined model; how many memberships changed
    for (int j = tid; j < n; j += PAIR_THREADS) {
      const bool in = err2(M1, P.rec(j)) <= thr2;
      nxt[P.o0 + j] = in ? 1 : 0;
      cc[0] += in ? 1.0 : 0.0;
      cc[1] += (in != (cur[P.o0 + j] != 0)) ? 1.0 : 0.0;
    }
    block_sum<PAIR_THREADS, CHUNK>(cc, sh_part, sh_tot);
    if (!(cc[0] >= (double)cur_cnt)) break;               // fewer inliers: the model before it stays
#pragma unroll
    for (int m = 0; m < 9; ++m) M[m] = M1[m];
    uint8_t* sw = cur; cur = nxt; nxt = sw;
    cur_cnt = (int)cc[0];
    if (cc[1] == 0.0) break;
  }
  return cur_cnt;
}

// ---- the records kernel ------------------------------------------------------------------------------------------------------------
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_pair_records(int64_t n_matches, int32_t n_pairs, const int64_t* __restrict__ offsets,
                                                          const int32_t* __restrict__ pair_camera, const int32_t* __restrict__ cam_model,
                                                          const double* __restrict__ cam_params, const double* __restrict__ xy1,
                                                          const double* __restrict__ xy2, double* __restrict__ rec,
                                                          uint8_t* __restrict__ valid, uint8_t* __restrict__ inlier, double* __restrict__ err) {
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
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
  double* r = rec + (size_t)i * PAIR_REC;
  r[0] = uv[0]; r[1] = uv[1]; r[2] = uv[2]; r[3] = uv[3];
  valid[i] = ok ? 1 : 0;
  inlier[i] = 0;                                       // what a match keeps unless its pair gets a model
  err[i] = quiet_nan();
}

// ---- host: a call up to the estimator's own kernels ---------------------------------------------------------------------------------
struct PairCall {              // the arguments the three entry points have in common
  const char* fn;              // the entry point, as the messages name it
  pxr_ctx* ctx;
  int32_t n_pairs; const int64_t* d_pair_offsets; int64_t n_matches; const double* d_xy1; const double* d_xy2;
  const int32_t* d_pair_camera; int32_t n_cameras; const int32_t* d_cam_model; const double* d_cam_params;
  const pxr_pair_options* o;
  int32_t* d_status; int32_t* d_n_inliers; int32_t* d_n_trials; uint8_t* d_inlier; double* d_err;
  double* h_ms;                // the *_timed entry point's four stage times, or NULL
};

struct PairBatch {             // what open_pair_batch leaves for the estimator's kernels: arrays of the context's workspace
  int32_t* order; double* rec; int32_t* pos; int32_t* n_valid; uint8_t* mask_a; uint8_t* mask_b;
  int32_t* winner;             // [n_pairs][winner_ints]
  double* winner_model;        // [n_pairs][9]
  int32_t max_trials;          // o.max_num_trials rounded up to a multiple of o.round_size
  std::optional<StageTimer<5>> timer;                   // records | compact | hypotheses | refine; marks 0 .. 2 are set
};

// Everything of a call before its hypothesis kernel: the argument and option checks (own_outputs: whether the per-pair outputs
// that only this estimator has are all given; own_error: NULL, or what is wrong with the arguments that only it has, reported
// after the array checks), the host copy of offsets and cameras with its checks and the processing order, the workspace, the
// records and their compaction.  n_pairs == 0 returns PXR_OK with nothing launched and `b` untouched: the driver returns too.
// The stream is synchronised by batch_order and once more when the order is uploaded; nothing after that waits for it.
inline int open_pair_batch(const PairCall& c, bool own_outputs, const char* own_error, int winner_ints, PairBatch& b) {
  const char* fn = c.fn;
  const pxr_pair_options* o = c.o;
  PXR_REQUIRE(c.ctx && o, "%s: NULL argument", fn);
  PXR_REQUIRE(c.n_pairs >= 0 && c.n_matches >= 0 && c.n_cameras >= 0, "%s: negative size", fn);
  PXR_REQUIRE(c.n_matches < ((int64_t)1 << 31), "%s: more than 2^31 matches", fn);
  PXR_REQUIRE(c.n_pairs == 0 || (c.d_pair_offsets && c.d_pair_camera && own_outputs && c.d_status && c.d_n_inliers && c.d_n_trials &&
                                 c.d_cam_model && c.d_cam_params), "%s: NULL pair / camera array", fn);
  PXR_REQUIRE(c.n_matches == 0 || (c.d_xy1 && c.d_xy2 && c.d_inlier && c.d_err), "%s: NULL match array", fn);
  PXR_REQUIRE(!own_error, "%s: %s", fn, own_error);
  PXR_REQUIRE(o->max_error > 0.0 && o->confidence > 0.0 && o->confidence < 1.0 && o->min_inlier_ratio >= 0.0 && o->min_inlier_ratio <= 1.0 &&
                  o->min_num_inliers >= 0 && o->min_num_trials >= 0 && o->max_num_trials >= 1 && o->max_num_trials <= (1 << 20) &&
                  o->round_size >= 1 && o->round_size <= (1 << 20) && o->refine_max_iterations >= 0 && o->lo_rounds >= 0,
              "%s: option out of range", fn);
  if (c.h_ms) c.h_ms[0] = c.h_ms[1] = c.h_ms[2] = c.h_ms[3] = 0.0;
  if (c.n_pairs == 0) {
    PXR_REQUIRE(c.n_matches == 0, "%s: pair_offsets ends at 0, not at n_matches = %lld", fn, (long long)c.n_matches);
    return PXR_OK;
  }
  pxr_ctx* ctx = c.ctx;
  PXR_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int64_t T = c.n_pairs, N = c.n_matches;

  // offsets and cameras are validated on a host copy, which also gives the processing order: pairs by descending match count
  std::vector<int64_t> off;
  std::vector<int32_t> order, pcam((size_t)T * 2);
  PXR_HIP(hipMemcpyAsync(pcam.data(), c.d_pair_camera, sizeof(int32_t) * (size_t)T * 2, hipMemcpyDeviceToHost, st));
  const auto cameras_in_range = [&](int64_t t) {
    for (int side = 0; side < 2; ++side)
      PXR_REQUIRE(pcam[2 * t + side] >= 0 && pcam[2 * t + side] < c.n_cameras, "%s: pair %lld names a camera outside [0, n_cameras = %d)", fn,
                  (long long)t, (int)c.n_cameras);
    return (int)PXR_OK;
  };
  if (int rc = batch_order(ctx, {fn, "pair_offsets", "pair", "n_matches"}, false, c.d_pair_offsets, T, N, off, order, cameras_in_range)) return rc;

  uint8_t* valid;
  Workspace ws;
  ws.take(b.rec, (size_t)N * PAIR_REC); ws.take(valid, (size_t)N); ws.take(b.pos, (size_t)N);
  ws.take(b.mask_a, (size_t)N); ws.take(b.mask_b, (size_t)N); ws.take(b.n_valid, (size_t)T); ws.take(b.order, (size_t)T);
  ws.take(b.winner, (size_t)T * winner_ints); ws.take(b.winner_model, (size_t)T * 9);
  if (int rc = ws.commit(ctx)) return rc;
  b.max_trials = (int32_t)(((int64_t)o->max_num_trials + o->round_size - 1) / o->round_size * o->round_size);

  StageTimer<5>& timer = b.timer.emplace(st, c.h_ms);
  if (int rc = timer.create(fn)) return rc;

  int rc = hip_check(hipMemcpyAsync(b.order, order.data(), sizeof(int32_t) * (size_t)T, hipMemcpyHostToDevice, st), "hipMemcpyAsync");
  if (rc == PXR_OK) rc = hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");      // (`order` goes out of scope)
  if (rc != PXR_OK) return rc;
  timer.mark(0);
  if (N > 0)
    hipLaunchKernelGGL(k_pair_records<PAIR_THREADS>, blocks_for(N, PAIR_THREADS), dim3(PAIR_THREADS), 0, st, N, c.n_pairs, c.d_pair_offsets,
                       c.d_pair_camera, c.d_cam_model, c.d_cam_params, c.d_xy1, c.d_xy2, b.rec, valid, c.d_inlier, c.d_err);
  timer.mark(1);
  hipLaunchKernelGGL(k_compact_records<PAIR_REC>, blocks_for(T, PAIR_THREADS), dim3(PAIR_THREADS), 0, st, T, c.d_pair_offsets, b.rec, valid, b.pos,
                     b.n_valid);
  timer.mark(2);
  return PXR_OK;
}

// after the refine kernel's launch: mark 4, the launch error (`what` names the kernel), the stage times
inline int close_pair_batch(PairBatch& b, const char* what) {
  b.timer->mark(4);
  const int rc = hip_check(hipGetLastError(), what);
  const int from[4] = {0, 1, 2, 3};
  return rc == PXR_OK ? b.timer->read(from, 4) : rc;
}

inline void pair_default_options(pxr_pair_options* o) {
  if (!o) return;
  o->max_error = 4.0; o->min_inlier_ratio = 0.25; o->confidence = 0.999;
  o->seed = 0; o->min_num_inliers = 15; o->min_num_trials = 64; o->max_num_trials = 10000; o->round_size = 64;
  o->refine_max_iterations = 100; o->lo_rounds = 4;
}

// the fields TvArgs, HgArgs and FmArgs have in common (their layouts stay their own: the kernels load them by offset)
template <class Args>
inline void fill_pair_args(Args& a, const PairCall& c, const PairBatch& b) {
  a.offsets = c.d_pair_offsets; a.pair_camera = c.d_pair_camera; a.cam_model = c.d_cam_model; a.cam_params = c.d_cam_params;
  a.order = b.order; a.rec = b.rec; a.pos = b.pos; a.n_valid = b.n_valid; a.winner = b.winner; a.mask_a = b.mask_a; a.mask_b = b.mask_b;
  a.o = *c.o;
  a.max_trials = b.max_trials;
  a.status = c.d_status; a.n_inliers = c.d_n_inliers; a.n_trials = c.d_n_trials; a.inlier = c.d_inlier; a.err = c.d_err;
}

}  // namespace pxr
