// pxr_triangulate.hip -- track triangulation on gfx950: known poses + keypoints + tracks -> 3D points and their inliers.
//
// Replaces pycolmap.triangulate_points as hloc.triangulation.main calls it from the reference's triangulation mode
// (pixsfm/refine_hloc.py:112-114) for the geometry it does: undistort every observation ([upstream COLMAP 3.8]
// <Model>::ImageToWorld), estimate one point per track robustly, filter by angular and reprojection error, keep the tracks
// with enough parallax.  The estimator is NOT COLMAP's (random two-view samples + image-space DLT): pairs are enumerated in
// a fixed order and solved in ray space, so the result is a function of the input alone.
//
//   k_tri_check     obs_image / image_camera in range (nothing is trusted into the other kernels)
//   k_tri_rays      one lane per observation: undistort, rotate into the world frame -> unit bearing d, camera centre c, valid
//   k_compact_records<6>  (pxr_robust.h) one lane per track: the valid rays of a track moved to the front of its slice (in order),
//                   their positions kept
//   k_tri_tracks    the estimator: a track per group of 16 lanes (one DPP row), four tracks per wavefront; hypotheses strided
//                   over the lanes, each lane scoring its own against all rays of the track
//
// With S a set of rays, solve(S) = argmin_X sum_S |(I - d d^t)(X - c)|^2 = A^-1 b, A = sum (I - d d^t), b = sum (I - d d^t) c,
// by the adjugate of the symmetric 3 x 3.  score(X): cos_i = d_i . (X - c_i) / |X - c_i|, inlier_i = cos_i >= cos(max_angle_error).
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

constexpr int TRI_THREADS = 256;     // the per-observation kernels
constexpr int TRI_GROUP = 16;        // lanes per track
constexpr int TRI_TPW = 64 / TRI_GROUP;
constexpr int TRI_RAY = 6;           // doubles per ray: d (3), c (3)
constexpr int TRI_LDS_RAYS = 32;     // a track of up to this many valid rays is staged in LDS; longer ones read global memory (L2)

// ---- validation --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TRI_THREADS) void k_tri_check(int64_t n_obs, const int32_t* __restrict__ obs_image, int32_t n_images,
                                                           const int32_t* __restrict__ image_camera, int32_t n_cameras,
                                                           int* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * TRI_THREADS + threadIdx.x;
  int bad = 0;
  if (i < n_obs) { const int32_t im = obs_image[i]; if (im < 0 || im >= n_images) bad |= 1; }
  if (i < n_images) { const int32_t c = image_camera[i]; if (c < 0 || c >= n_cameras) bad |= 2; }
  if (bad) atomicOr(flag, bad);
}

// ---- batched undistortion (pxr_image_to_world) ---------------------------------------------------------------------------------
__global__ __launch_bounds__(TRI_THREADS) void k_image_to_world(int64_t n, const int32_t* __restrict__ cam_index, int32_t n_cameras,
                                                                const int32_t* __restrict__ cam_model,
                                                                const double* __restrict__ cam_params,
                                                                const double* __restrict__ xy, double* __restrict__ uv,
                                                                uint8_t* __restrict__ ok) {
  const int64_t i = (int64_t)blockIdx.x * TRI_THREADS + threadIdx.x;
  if (i >= n) return;
  const int32_t cam = cam_index ? cam_index[i] : 0;
  double u = quiet_nan(), v = quiet_nan();
  bool good = false;
  if (cam >= 0 && cam < n_cameras) {
    double k[PXR_KPAD];
#pragma unroll
    for (int j = 0; j < PXR_KPAD; ++j) k[j] = cam_params[(size_t)cam * PXR_KPAD + j];
    const double2 p = reinterpret_cast<const double2*>(xy)[i];
    good = image_to_world(cam_model[cam], k, p.x, p.y, u, v);
  }
  reinterpret_cast<double2*>(uv)[i] = make_double2(u, v);
  if (ok) ok[i] = good ? 1 : 0;
}

// ---- kernel A: rays ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TRI_THREADS) void k_tri_rays(const pxr_tri_view v, double* __restrict__ rays, uint8_t* __restrict__ valid,
                                                          uint8_t* __restrict__ obs_inlier, double* __restrict__ obs_err) {
  const int64_t i = (int64_t)blockIdx.x * TRI_THREADS + threadIdx.x;
  if (i >= v.n_obs) return;
  const int img = v.d_obs_image[i], cam = v.d_image_camera[img];
  double k[PXR_KPAD], R[9], t[3];
#pragma unroll
  for (int j = 0; j < PXR_KPAD; ++j) k[j] = v.d_cam_params[(size_t)cam * PXR_KPAD + j];
  quat_to_rotation(v.d_qvec + 4 * (size_t)img, R);
#pragma unroll
  for (int j = 0; j < 3; ++j) t[j] = v.d_tvec[3 * (size_t)img + j];
  const double2 p = reinterpret_cast<const double2*>(v.d_obs_xy)[i];
  double un, vn;
  bool ok = image_to_world(v.d_cam_model[cam], k, p.x, p.y, un, vn);
  // d = R^t (u, v, 1) / |.|, c = -R^t t
  const double inv = 1.0 / sqrt(un * un + vn * vn + 1.0);
  double* r = rays + (size_t)i * TRI_RAY;
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    r[m] = (R[m] * un + R[3 + m] * vn + R[6 + m]) * inv;
    r[3 + m] = -(R[m] * t[0] + R[3 + m] * t[1] + R[6 + m] * t[2]);
    ok = ok && isfinite(r[m]) && isfinite(r[3 + m]);
  }
  valid[i] = ok ? 1 : 0;
  obs_inlier[i] = 0;            // what an observation keeps unless its track gets a point
  obs_err[i] = quiet_nan();
}

// ---- kernel B: the estimator -----------------------------------------------------------------------------------------------------
struct TriArgs {
  pxr_tri_view v;
  const int32_t* order;        // [n_tracks] tracks by descending length
  const double* rays;          // [n_obs][TRI_RAY], compacted per track
  const int32_t* pos;          // [n_obs]
  const int32_t* n_valid;      // [n_tracks]
  double cos_min_tri, cos_max_err, max_reproj;
  int32_t min_len, max_hyp;
  double* xyz; int32_t* status; int32_t* n_inliers; uint8_t* obs_inlier; double* obs_err;
};

struct Sym3 {                  // A (6: 00 01 02 11 12 22) and b (3) of solve()
  double a[6], b[3];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int j = 0; j < 6; ++j) a[j] = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) b[j] = 0.0;
  }
  __device__ __forceinline__ void add(const double* d, const double* c) {     // += (I - d d^t), (I - d d^t) c
    a[0] += 1.0 - d[0] * d[0]; a[1] += -(d[0] * d[1]); a[2] += -(d[0] * d[2]);
    a[3] += 1.0 - d[1] * d[1]; a[4] += -(d[1] * d[2]); a[5] += 1.0 - d[2] * d[2];
    const double dc = d[0] * c[0] + d[1] * c[1] + d[2] * c[2];
#pragma unroll
    for (int j = 0; j < 3; ++j) b[j] += c[j] - d[j] * dc;
  }
  __device__ __forceinline__ void row16() {
#pragma unroll
    for (int j = 0; j < 6; ++j) a[j] = row16_sum(a[j]);
#pragma unroll
    for (int j = 0; j < 3; ++j) b[j] = row16_sum(b[j]);
  }
  __device__ __forceinline__ void solve(double X[3]) const {                  // adjugate; a singular A leaves a non-finite X
    const double c00 = a[3] * a[5] - a[4] * a[4], c01 = a[2] * a[4] - a[1] * a[5], c02 = a[1] * a[4] - a[2] * a[3];
    const double c11 = a[0] * a[5] - a[2] * a[2], c12 = a[1] * a[2] - a[0] * a[4], c22 = a[0] * a[3] - a[1] * a[1];
    const double det = a[0] * c00 + a[1] * c01 + a[2] * c02;
    X[0] = (c00 * b[0] + c01 * b[1] + c02 * b[2]) / det;
    X[1] = (c01 * b[0] + c11 * b[1] + c12 * b[2]) / det;
    X[2] = (c02 * b[0] + c12 * b[1] + c22 * b[2]) / det;
  }
};

// cos of the angle between ray (d, c) and X - c (NaN when X sits on the centre: never an inlier)
__device__ __forceinline__ double ray_cos(const double* r, const double* X) {
  const double w0 = X[0] - r[3], w1 = X[1] - r[4], w2 = X[2] - r[5];
  return (r[0] * w0 + r[1] * w1 + r[2] * w2) / sqrt(w0 * w0 + w1 * w1 + w2 * w2);
}

// pair number p of the n (n - 1) / 2 unordered pairs (a < b) in lexicographic order
__device__ __forceinline__ void tri_pair(int64_t p, int64_t n, int& a_out, int& b_out) {
  const double m = (double)(2 * n - 1);
  int64_t a = (int64_t)floor((m - sqrt(m * m - 8.0 * (double)p)) * 0.5);
  a = max((int64_t)0, min(a, n - 2));
  auto start = [&](int64_t r) { return r * (2 * n - r - 1) / 2; };
  while (a + 1 <= n - 2 && start(a + 1) <= p) ++a;
  while (a > 0 && start(a) > p) --a;
  a_out = (int)a;
  b_out = (int)(a + 1 + (p - start(a)));
}

// pair number of hypothesis h: h itself while all P pairs fit, else floor(h P / max_hyp) (split so that no product overflows)
__device__ __forceinline__ int64_t tri_hypothesis_pair(int64_t h, int64_t P, int64_t max_hyp) {
  return P <= max_hyp ? h : h * (P / max_hyp) + h * (P % max_hyp) / max_hyp;
}

__device__ __forceinline__ bool group_any(bool pred, int group) {
  return ((__ballot(pred) >> (TRI_GROUP * group)) & 0xffffull) != 0;
}

// the pixel error of track-local valid ray j against X
__device__ __forceinline__ double tri_reproj(const TriArgs& a, int64_t o0, int j, const double* X) {
  const int64_t i = o0 + a.pos[o0 + j];
  const int img = a.v.d_obs_image[i], cam = a.v.d_image_camera[img];
  double k[PXR_KPAD];
#pragma unroll
  for (int m = 0; m < PXR_KPAD; ++m) k[m] = a.v.d_cam_params[(size_t)cam * PXR_KPAD + m];
  double x, y;
  if (!world_to_pixel(a.v.d_cam_model[cam], k, a.v.d_qvec + 4 * (size_t)img, a.v.d_tvec + 3 * (size_t)img, X, x, y)) return quiet_nan();
  const double ex = x - a.v.d_obs_xy[2 * i], ey = y - a.v.d_obs_xy[2 * i + 1];
  return sqrt(ex * ex + ey * ey);
}

// One track on the 16 lanes of a group.  Every branch that encloses a cross-lane operation (row16_sum, __shfl, __ballot) is
// uniform over the group; the hypothesis loop, where the lanes run different trip counts, has none.
template <bool LDS>
__device__ __forceinline__ void tri_track(const TriArgs& a, int64_t t, int64_t o0, int nv, const double* __restrict__ rays, int l, int group) {
  // rays: this track's compacted rays (LDS or global memory)
  const int64_t P = (int64_t)nv * (nv - 1) / 2;
  const int64_t H = min(P, (int64_t)a.max_hyp);
  // 1. hypotheses, strided over the lanes
  int best_cnt = -1, best_h = 0x7fffffff;
  double best_sum = 0.0;
  for (int64_t h = l; h < H; h += TRI_GROUP) {
    const int64_t p = tri_hypothesis_pair(h, P, a.max_hyp);
    int ia, ib;
    tri_pair(p, nv, ia, ib);
    const double* ra = rays + ia * TRI_RAY;
    const double* rb = rays + ib * TRI_RAY;
    if (ra[0] * rb[0] + ra[1] * rb[1] + ra[2] * rb[2] > a.cos_min_tri) continue;      // parallax too small
    Sym3 s; s.clear(); s.add(ra, ra + 3); s.add(rb, rb + 3);
    double X[3];
    s.solve(X);
    int cnt = 0, own = 0;
    double sum = 0.0;
    for (int j = 0; j < nv; ++j) {
      const double c = ray_cos(rays + j * TRI_RAY, X);
      if (c >= a.cos_max_err) { ++cnt; sum += 1.0 - c; own += (j == ia || j == ib); }
    }
    if (own != 2) continue;
    if (cnt > best_cnt || (cnt == best_cnt && sum < best_sum)) { best_cnt = cnt; best_sum = sum; best_h = (int)h; }   // (h ascends: ties keep the first)
  }
  // 2. selection: max over (count, -sum, -h), compared -- no floating-point accumulation across lanes
#pragma unroll
  for (int off = TRI_GROUP / 2; off > 0; off >>= 1) {
    const int oc = __shfl_xor(best_cnt, off, TRI_GROUP), oh = __shfl_xor(best_h, off, TRI_GROUP);
    const double os = __shfl_xor(best_sum, off, TRI_GROUP);
    if (oc > best_cnt || (oc == best_cnt && (os < best_sum || (os == best_sum && oh < best_h)))) { best_cnt = oc; best_sum = os; best_h = oh; }
  }
  if (best_cnt < 0) {
    if (l == 0) { a.status[t] = 2; a.n_inliers[t] = 0; }
    return;
  }
  double X[3];
  {
    const int64_t p = tri_hypothesis_pair(best_h, P, a.max_hyp);
    int ia, ib;
    tri_pair(p, nv, ia, ib);
    Sym3 s; s.clear(); s.add(rays + ia * TRI_RAY, rays + ia * TRI_RAY + 3); s.add(rays + ib * TRI_RAY, rays + ib * TRI_RAY + 3);
    s.solve(X);                                                                       // (the winner's own arithmetic, on every lane)
  }
  // 3. local optimisation: X' = solve(inliers of X), kept when it has at least as many inliers
  {
    Sym3 s; s.clear();
    for (int j = l; j < nv; j += TRI_GROUP) {
      const double* r = rays + j * TRI_RAY;
      if (ray_cos(r, X) >= a.cos_max_err) s.add(r, r + 3);
    }
    s.row16();
    double X1[3];
    s.solve(X1);
    double cnt1 = 0.0;
    for (int j = l; j < nv; j += TRI_GROUP) cnt1 += ray_cos(rays + j * TRI_RAY, X1) >= a.cos_max_err ? 1.0 : 0.0;
    cnt1 = row16_sum(cnt1);
    if (cnt1 >= (double)best_cnt) { X[0] = X1[0]; X[1] = X1[1]; X[2] = X1[2]; }
  }
  // 4. reprojection filter; the final flags of a lane's rays (j = l mod 16) wait in obs_inlier, which that lane alone reads back
  double n_ang = 0.0, n_fin = 0.0;
  {
    Sym3 s; s.clear();
    for (int j = l; j < nv; j += TRI_GROUP) {
      const double* r = rays + j * TRI_RAY;
      bool fin = false;
      if (ray_cos(r, X) >= a.cos_max_err) {
        n_ang += 1.0;
        fin = tri_reproj(a, o0, j, X) <= a.max_reproj;
        if (fin) { n_fin += 1.0; s.add(r, r + 3); }
      }
      a.obs_inlier[o0 + a.pos[o0 + j]] = fin ? 1 : 0;
    }
    n_ang = row16_sum(n_ang); n_fin = row16_sum(n_fin);
    if (n_fin < n_ang && n_fin >= 2.0) { s.row16(); s.solve(X); }
  }
  // 5. acceptance: enough members, and a pair of them that sees X under at least min_tri_angle
  bool accept = n_fin >= (double)max(2, a.min_len) && isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]);
  if (accept) {
    bool wide = false;
    for (int ci = 0; ci < nv && !wide; ci += TRI_GROUP) {
      const int i = ci + l;
      double ei[3] = {0.0, 0.0, 0.0};
      bool fi = false;
      if (i < nv && a.obs_inlier[o0 + a.pos[o0 + i]]) {
        const double* r = rays + i * TRI_RAY;
        const double w0 = X[0] - r[3], w1 = X[1] - r[4], w2 = X[2] - r[5], nrm = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
        ei[0] = w0 / nrm; ei[1] = w1 / nrm; ei[2] = w2 / nrm; fi = true;
      }
      for (int cj = ci; cj < nv && !wide; cj += TRI_GROUP) {
        const int j = cj + l;
        double ej[3] = {0.0, 0.0, 0.0};
        int fj = 0;
        if (j < nv && a.obs_inlier[o0 + a.pos[o0 + j]]) {
          const double* r = rays + j * TRI_RAY;
          const double w0 = X[0] - r[3], w1 = X[1] - r[4], w2 = X[2] - r[5], nrm = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
          ej[0] = w0 / nrm; ej[1] = w1 / nrm; ej[2] = w2 / nrm; fj = 1;
        }
        bool found = false;
        for (int rot = (ci == cj ? 1 : 0); rot < TRI_GROUP; ++rot) {                  // every lane meets every lane of the other chunk
          const int src = (l + rot) & (TRI_GROUP - 1);
          const double x0 = __shfl(ej[0], src, TRI_GROUP), x1 = __shfl(ej[1], src, TRI_GROUP), x2 = __shfl(ej[2], src, TRI_GROUP);
          const int f = __shfl(fj, src, TRI_GROUP);
          if (fi && f && ei[0] * x0 + ei[1] * x1 + ei[2] * x2 <= a.cos_min_tri) found = true;
        }
        wide = group_any(found, group);
      }
    }
    accept = wide;
  }
  if (!accept) {
    for (int j = l; j < nv; j += TRI_GROUP) a.obs_inlier[o0 + a.pos[o0 + j]] = 0;
    if (l == 0) { a.status[t] = 3; a.n_inliers[t] = 0; }
    return;
  }
  for (int j = l; j < nv; j += TRI_GROUP) a.obs_err[o0 + a.pos[o0 + j]] = tri_reproj(a, o0, j, X);
  if (l == 0) {
    a.xyz[3 * t] = X[0]; a.xyz[3 * t + 1] = X[1]; a.xyz[3 * t + 2] = X[2];
    a.status[t] = 0; a.n_inliers[t] = (int32_t)n_fin;
  }
}

__global__ __launch_bounds__(64) void k_tri_tracks(const TriArgs a) {
  __shared__ double sh_rays[TRI_TPW][TRI_LDS_RAYS * TRI_RAY];
  const int l = threadIdx.x & (TRI_GROUP - 1), group = threadIdx.x / TRI_GROUP;
  const int64_t slot = (int64_t)blockIdx.x * TRI_TPW + group;
  if (slot >= a.v.n_tracks) return;
  const int64_t t = a.order[slot];
  const int64_t o0 = a.v.d_track_offsets[t];
  const int nv = a.n_valid[t];
  if (nv < 2) {
    if (l == 0) { a.status[t] = 1; a.n_inliers[t] = 0; }
    return;
  }
  const double* g = a.rays + (size_t)o0 * TRI_RAY;
  if (nv <= TRI_LDS_RAYS) {
    for (int x = l; x < nv * TRI_RAY; x += TRI_GROUP) sh_rays[group][x] = g[x];
    __threadfence_block();                      // LDS words of the other lanes of this group
    __builtin_amdgcn_wave_barrier();
    tri_track<true>(a, t, o0, nv, sh_rays[group], l, group);
  } else {
    tri_track<false>(a, t, o0, nv, g, l, group);
  }
}

static int triangulate(pxr_ctx* ctx, const pxr_tri_view* v, const pxr_tri_options* o, double* d_xyz, int32_t* d_status,
                       int32_t* d_n_inliers, uint8_t* d_obs_inlier, double* d_obs_err, double* h_ms) {
  const char* fn = "pxr_triangulate_tracks";
  PXR_REQUIRE(ctx && v && o, "%s: NULL argument", fn);
  PXR_REQUIRE(v->n_tracks >= 0 && v->n_obs >= 0 && v->n_images >= 0 && v->n_cameras >= 0, "%s: negative size", fn);
  PXR_REQUIRE(v->n_obs < ((int64_t)1 << 31) && v->n_tracks < ((int64_t)1 << 31), "%s: more than 2^31 observations or tracks", fn);
  PXR_REQUIRE(v->n_tracks == 0 || (v->d_track_offsets && d_xyz && d_status && d_n_inliers), "%s: NULL track array", fn);
  PXR_REQUIRE(v->n_obs == 0 || (v->d_obs_image && v->d_obs_xy && d_obs_inlier && d_obs_err && v->d_image_camera && v->d_qvec &&
                                v->d_tvec && v->d_cam_model && v->d_cam_params), "%s: NULL observation / image / camera array", fn);
  PXR_REQUIRE(o->min_tri_angle >= 0.0 && o->min_tri_angle < 180.0 && o->max_angle_error >= 0.0 && o->max_angle_error < 90.0 &&
                  o->max_reproj_error >= 0.0 && o->max_hypotheses >= 1 && o->max_hypotheses <= (1 << 20), "%s: option out of range", fn);
  if (h_ms) h_ms[0] = h_ms[1] = h_ms[2] = h_ms[3] = 0.0;
  if (v->n_tracks == 0) return PXR_OK;
  PXR_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int64_t T = v->n_tracks, N = v->n_obs;

  // the offsets are validated on a host copy, which also gives the processing order: tracks by descending length (a stable
  // counting sort), so that the groups of a wavefront run tracks of like length and the longest start first
  std::vector<int64_t> off;
  std::vector<int32_t> order;
  if (int rc = batch_order(ctx, {fn, "track_offsets", "track", "n_obs"}, true, v->d_track_offsets, T, N, off, order, [](int64_t) { return (int)PXR_OK; }))
    return rc;

  int* flag; double* rays; uint8_t* valid; int32_t *pos, *n_valid, *d_order;
  Workspace ws;
  ws.take(flag, 4); ws.take(rays, (size_t)N * TRI_RAY); ws.take(valid, (size_t)N); ws.take(pos, (size_t)N);
  ws.take(n_valid, (size_t)T); ws.take(d_order, (size_t)T);
  if (int rc = ws.commit(ctx)) return rc;

  StageTimer<6> timer(st, h_ms);                         // check | (the flag's read-back) | rays | compact | tracks
  if (int rc = timer.create(fn)) return rc;

  int h_flag = 0;
  int rc = hip_check(hipMemsetAsync(flag, 0, 16, st), "hipMemsetAsync");
  if (rc == PXR_OK) {
    timer.mark(0);
    const int64_t n_check = std::max<int64_t>(N, v->n_images);
    if (n_check > 0)
      hipLaunchKernelGGL(k_tri_check, blocks_for(n_check, TRI_THREADS), dim3(TRI_THREADS), 0, st, N, v->d_obs_image, v->n_images,
                         v->d_image_camera, v->n_cameras, flag);
    timer.mark(1);
    rc = hip_check(hipMemcpyAsync(&h_flag, flag, 4, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
  }
  if (rc == PXR_OK) rc = hip_check(hipMemcpyAsync(d_order, order.data(), sizeof(int32_t) * (size_t)T, hipMemcpyHostToDevice, st), "hipMemcpyAsync");
  if (rc == PXR_OK) rc = hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");      // (also: `order` may go out of scope)
  if (rc != PXR_OK) return rc;
  if (h_flag) {
    if (h_flag & 1) return set_error(PXR_EINVAL, "%s: an observation names an image outside [0, n_images = %d)", fn, (int)v->n_images);
    return set_error(PXR_EINVAL, "%s: an image names a camera outside [0, n_cameras = %d)", fn, (int)v->n_cameras);
  }

  timer.mark(2);
  if (N > 0) hipLaunchKernelGGL(k_tri_rays, blocks_for(N, TRI_THREADS), dim3(TRI_THREADS), 0, st, *v, rays, valid, d_obs_inlier, d_obs_err);
  timer.mark(3);
  hipLaunchKernelGGL(k_compact_records<TRI_RAY>, blocks_for(T, TRI_THREADS), dim3(TRI_THREADS), 0, st, T, v->d_track_offsets, rays, valid, pos, n_valid);
  timer.mark(4);
  TriArgs a;
  a.v = *v; a.order = d_order; a.rays = rays; a.pos = pos; a.n_valid = n_valid;
  const double rad = 3.14159265358979323846 / 180.0;
  a.cos_min_tri = std::cos(o->min_tri_angle * rad); a.cos_max_err = std::cos(o->max_angle_error * rad);
  a.max_reproj = o->max_reproj_error; a.min_len = o->min_track_len; a.max_hyp = o->max_hypotheses;
  a.xyz = d_xyz; a.status = d_status; a.n_inliers = d_n_inliers; a.obs_inlier = d_obs_inlier; a.obs_err = d_obs_err;
  hipLaunchKernelGGL(k_tri_tracks, blocks_for(T, TRI_TPW), dim3(64), 0, st, a);
  timer.mark(5);
  rc = hip_check(hipGetLastError(), "k_tri_tracks launch");
  const int from[4] = {0, 2, 3, 4};
  return rc == PXR_OK ? timer.read(from, 4) : rc;
}

}  // namespace pxr

extern "C" int pxr_image_to_world(pxr_ctx* ctx, int64_t n, const int32_t* d_cam_index, int32_t n_cameras, const int32_t* d_cam_model,
                                  const double* d_cam_params, const double* d_xy, double* d_uv, uint8_t* d_ok) {
  PXR_REQUIRE(ctx && n >= 0 && n_cameras >= 0, "pxr_image_to_world: NULL context or negative size");
  if (n == 0) return PXR_OK;
  PXR_REQUIRE(d_cam_model && d_cam_params && d_xy && d_uv, "pxr_image_to_world: NULL argument");
  PXR_REQUIRE(n_cameras >= 1, "pxr_image_to_world: no cameras");
  PXR_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(pxr::k_image_to_world, dim3((unsigned)((n + pxr::TRI_THREADS - 1) / pxr::TRI_THREADS)), dim3(pxr::TRI_THREADS), 0,
                     ctx->stream, n, d_cam_index, n_cameras, d_cam_model, d_cam_params, d_xy, d_uv, d_ok);
  return pxr::hip_check(hipGetLastError(), "k_image_to_world launch");
}

extern "C" int pxr_triangulate_tracks(pxr_ctx* ctx, const pxr_tri_view* view, const pxr_tri_options* options, double* d_xyz,
                                      int32_t* d_status, int32_t* d_n_inliers, uint8_t* d_obs_inlier, double* d_obs_err) {
  return pxr::triangulate(ctx, view, options, d_xyz, d_status, d_n_inliers, d_obs_inlier, d_obs_err, nullptr);
}

extern "C" int pxr_triangulate_tracks_timed(pxr_ctx* ctx, const pxr_tri_view* view, const pxr_tri_options* options, double* d_xyz,
                                            int32_t* d_status, int32_t* d_n_inliers, uint8_t* d_obs_inlier, double* d_obs_err,
                                            double* h_kernel_ms) {
  PXR_REQUIRE(h_kernel_ms, "pxr_triangulate_tracks_timed: NULL h_kernel_ms");
  return pxr::triangulate(ctx, view, options, d_xyz, d_status, d_n_inliers, d_obs_inlier, d_obs_err, h_kernel_ms);
}
