// pxr_global.hip -- global mapping on gfx950: rotation averaging over the view graph, then global positioning of all camera
// centres and points at once (the specification is the comment of include/pixsfm_hip.h).
//
// Rotation averaging (pxr_rotation_averaging).  Host: validation, the root, Prim's spanning tree and the rotations along it, the
// image -> pairs adjacency (CSR, ascending pair index).  Device, per iteration:
//   k_ra_residual   one lane per pair: e_p = Log(R_j^t R_p R_i), its angle and the weight rho_p of the iteration
//   k_ra_assemble   one lane per image row, OWNER COMPUTES: the row of the grounded graph Laplacian (upper triangle) and one
//                   coordinate of the right-hand side, summed over the image's pairs in ascending pair index -- no atomics
//   chol_factor_solve   (pxr_chol.hip) three times, one per coordinate: (n - 1)^2 matrix, the same for all three
//   k_ra_update     one workgroup: R_k <- R_k Exp(w_k), max |w_k|
// Rotations are unit quaternions (w first, R(a b) = R(a) R(b)) from the first to the last kernel.
//
// Global positioning (pxr_global_positioning).  Host: validation, the tracks by descending length, the fixed-point scale.
// Device: k_gp_rays once, then per round
//   k_gp_tracks     a track per 16 lanes: A_k = sum w (I - d d^t), its determinant, A_k^-1 by the adjugate
//   k_gp_contract   a track per 16 lanes, the ordered pairs (a, b) of its observations strided over the lanes: the 3 x 3 blocks
//                   of the reduced system, added to S as 64-bit FIXED-POINT integers (atomicAdd on integers commutes: the same
//                   bits every run whatever the order)
//   k_gp_pairs      one lane per pair: mu w_p (I - b b^t) into the blocks (i, i), (j, j), (i, j), the same way
//   k_gp_gauge      one workgroup: g and h of the scale constraint, owner computes per image
//   k_gp_pack       fixed point -> [S | g] in the layout of chol_factor_solve, the root's rows and columns left out
//   chol_factor_solve   y = S^-1 g
//   k_gp_scale      one workgroup: c = h y / (g . y), the round's info word
//   k_gp_update     a track per 16 lanes: X_k = A_k^-1 sum w (I - d d^t) c_i, then the new weight of every observation
//   k_gp_pair_update  one lane per pair: the new weight of the pair
// Cross-lane operations are __shfl_xor and __syncthreads only, and there is no MFMA here: the file runs lane by lane on the CPU
// (tests/lane_emulation/global_on_host.cpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "pxr_batch.h"
#include "pxr_device.h"
#include "pxr_internal.h"
#include "pxr_undistort.h"

namespace pxr {

size_t chol_workspace_doubles(int n);
int chol_factor_solve(hipStream_t st, double* a, int n, int* d_info, double* linv_ws, double* x_out, bool zero_info);

constexpr int GM_THREADS = 256;      // the per-pair / per-observation / per-entry kernels, and the one-workgroup kernels
constexpr int GM_GROUP = 16;         // lanes per track
constexpr int GM_TPW = 64 / GM_GROUP;
constexpr double GM_DEG = 3.14159265358979323846 / 180.0;

// ---- quaternions (w, x, y, z), host and device ---------------------------------------------------------------------------------
__host__ __device__ inline void quat_mul(const double* a, const double* b, double* o) {      // R(o) = R(a) R(b)
  const double w = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  const double x = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  const double y = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  const double z = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
  o[0] = w; o[1] = x; o[2] = y; o[3] = z;
}
__host__ __device__ inline void quat_conj(const double* a, double* o) { o[0] = a[0]; o[1] = -a[1]; o[2] = -a[2]; o[3] = -a[3]; }
// unit length, w >= 0
__host__ __device__ inline void quat_canonical(double* q) {
  const double s = (q[0] < 0.0 ? -1.0 : 1.0) / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  q[0] *= s; q[1] *= s; q[2] *= s; q[3] *= s;
}
// the rotation vector of q: angle 2 atan2(|v|, |w|) about v (the series' first term where |v| <= 1e-12)
__host__ __device__ inline void quat_log(const double* q, double* e) {
  const double sg = q[0] < 0.0 ? -1.0 : 1.0;
  const double w = sg * q[0], x = sg * q[1], y = sg * q[2], z = sg * q[3];
  const double s = sqrt(x * x + y * y + z * z);
  const double k = s > 1e-12 ? 2.0 * atan2(s, w) / s : 2.0;
  e[0] = k * x; e[1] = k * y; e[2] = k * z;
}
__host__ __device__ inline void quat_exp(const double* om, double* q) {
  const double th = sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);
  double k = 0.5;
  q[0] = 1.0;
  if (th > 1e-12) { k = sin(0.5 * th) / th; q[0] = cos(0.5 * th); }
  q[1] = k * om[0]; q[2] = k * om[1]; q[3] = k * om[2];
}

// sum over the workgroup of GM_THREADS lanes, in a fixed order; every lane gets it
__device__ __forceinline__ double block_sum(double v, double* sh) {
  const int tid = threadIdx.x;
  __syncthreads();
  sh[tid] = v;
  __syncthreads();
  for (int s = GM_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) sh[tid] += sh[tid + s];
    __syncthreads();
  }
  return sh[0];
}
__device__ __forceinline__ double group_sum(double v) {         // over the 16 lanes of a track
#pragma unroll
  for (int m = GM_GROUP / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, GM_GROUP);
  return v;
}

// The pair list of both drivers on the host.  pair_image and the weights are downloaded and the stream synchronised (a download
// the driver queued before the call has arrived too); every pair is checked -- its images in range, no self pair, a finite
// non-negative weight -- and then by check_pair(p, i, j), the driver's own check of pair p = (i, j) (PXR_OK or its error); the
// images' adjacency (adj_off / adj_pair) lists each image's pairs in ascending pair index.
template <class CheckPair>
static int pair_list(pxr_ctx* ctx, const char* fn, int n, int P, const int32_t* d_pair_image, const double* d_pair_weight,
                     std::vector<int32_t>& pim, std::vector<double>& pw, std::vector<int32_t>& adj_off, std::vector<int32_t>& adj_pair,
                     CheckPair check_pair) {
  pim.resize((size_t)2 * P); pw.resize((size_t)P);
  if (P > 0) {
    PXR_HIP(hipMemcpyAsync(pim.data(), d_pair_image, sizeof(int32_t) * 2 * (size_t)P, hipMemcpyDeviceToHost, ctx->stream));
    PXR_HIP(hipMemcpyAsync(pw.data(), d_pair_weight, sizeof(double) * (size_t)P, hipMemcpyDeviceToHost, ctx->stream));
  }
  PXR_HIP(hipStreamSynchronize(ctx->stream));
  adj_off.assign((size_t)n + 1, 0);
  for (int p = 0; p < P; ++p) {
    const int i = pim[2 * p], j = pim[2 * p + 1];
    PXR_REQUIRE(i >= 0 && i < n && j >= 0 && j < n, "%s: pair %d names an image outside [0, n_images = %d)", fn, p, n);
    PXR_REQUIRE(i != j, "%s: pair %d joins image %d to itself", fn, p, i);
    PXR_REQUIRE(std::isfinite(pw[p]) && pw[p] >= 0.0, "%s: the weight of pair %d is negative or not finite", fn, p);
    if (int rc = check_pair(p, i, j)) return rc;
    ++adj_off[i + 1]; ++adj_off[j + 1];
  }
  for (int k = 0; k < n; ++k) adj_off[k + 1] += adj_off[k];
  adj_pair.resize((size_t)2 * P);
  std::vector<int32_t> fill(adj_off.begin(), adj_off.end() - 1);
  for (int p = 0; p < P; ++p) { adj_pair[fill[pim[2 * p]]++] = p; adj_pair[fill[pim[2 * p + 1]]++] = p; }
  return PXR_OK;
}

// ================================================================================================================================
// rotation averaging
// ================================================================================================================================
__global__ __launch_bounds__(GM_THREADS) void k_ra_residual(int32_t n_pairs, const int32_t* __restrict__ pair_image,
                                                            const double* __restrict__ pair_q, const double* __restrict__ q,
                                                            const double* __restrict__ weight, int l1, double min_angle, double sigma,
                                                            double* __restrict__ e, double* __restrict__ rho, double* __restrict__ angle) {
  const int p = blockIdx.x * GM_THREADS + threadIdx.x;
  if (p >= n_pairs) return;
  const int i = pair_image[2 * p], j = pair_image[2 * p + 1];
  double qi[4], qj[4], qp[4], t[4], r[4], v[3];
#pragma unroll
  for (int k = 0; k < 4; ++k) { qi[k] = q[4 * (size_t)i + k]; qj[k] = q[4 * (size_t)j + k]; qp[k] = pair_q[4 * (size_t)p + k]; }
  quat_conj(qj, qj);
  quat_mul(qj, qp, t);
  quat_mul(t, qi, r);                                             // R_j^t R_p R_i
  quat_log(r, v);
  const double th = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  const double ts = th / sigma;
  e[3 * (size_t)p] = v[0]; e[3 * (size_t)p + 1] = v[1]; e[3 * (size_t)p + 2] = v[2];
  rho[p] = l1 ? weight[p] / fmax(th, min_angle) : weight[p] / (1.0 + ts * ts);
  angle[p] = th;
}

// row of image k (k != root) of [L | b_coord]: aug is zero on entry
__global__ __launch_bounds__(GM_THREADS) void k_ra_assemble(int32_t n_images, int32_t root, int coord, const int32_t* __restrict__ adj_off,
                                                            const int32_t* __restrict__ adj_pair, const int32_t* __restrict__ pair_image,
                                                            const double* __restrict__ e, const double* __restrict__ rho,
                                                            double* __restrict__ aug) {
  const int k = blockIdx.x * GM_THREADS + threadIdx.x;
  if (k >= n_images || k == root) return;
  const int m = n_images - 1, ld = m + 1;
  const int row = k < root ? k : k - 1;
  double* a = aug + (size_t)row * ld;
  double diag = 0.0, rhs = 0.0;
  for (int x = adj_off[k]; x < adj_off[k + 1]; ++x) {
    const int p = adj_pair[x];
    const int i = pair_image[2 * p], j = pair_image[2 * p + 1];
    const double w = rho[p], ec = e[3 * (size_t)p + coord];
    const int other = (j == k) ? i : j;
    diag += w;
    rhs += (j == k) ? w * ec : -(w * ec);
    if (other != root) {
      const int col = other < root ? other : other - 1;
      if (col > row) a[col] -= w;                                 // this lane alone writes the row
    }
  }
  a[row] = diag;
  a[m] = rhs;
}

// q_k <- q_k Exp(w_k); stat[0] = max |w_k|
__global__ __launch_bounds__(GM_THREADS) void k_ra_update(int32_t n_images, int32_t root, const double* __restrict__ omega,
                                                          double* __restrict__ q, double* __restrict__ stat) {
  __shared__ double sh[GM_THREADS];
  const int tid = threadIdx.x, m = n_images - 1;
  double mx = 0.0;
  for (int k = tid; k < n_images; k += GM_THREADS) {
    if (k == root) continue;
    const int row = k < root ? k : k - 1;
    const double om[3] = {omega[row], omega[m + row], omega[2 * (size_t)m + row]};
    const double th = sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);
    mx = th > mx || th != th ? th : mx;                           // a NaN stays
    double dq[4], qk[4], o[4];
    quat_exp(om, dq);
#pragma unroll
    for (int c = 0; c < 4; ++c) qk[c] = q[4 * (size_t)k + c];
    quat_mul(qk, dq, o);
    quat_canonical(o);
#pragma unroll
    for (int c = 0; c < 4; ++c) q[4 * (size_t)k + c] = o[c];
  }
  sh[tid] = mx;
  __syncthreads();
  for (int s = GM_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) { const double o = sh[tid + s]; if (o > sh[tid] || o != o) sh[tid] = o; }
    __syncthreads();
  }
  if (tid == 0) stat[0] = sh[0];
}

static int rotation_averaging(pxr_ctx* ctx, int32_t n_images, int32_t n_pairs, const int32_t* d_pair_image, const double* d_pair_qvec,
                              const double* d_pair_weight, const pxr_rotavg_options* o, double* d_qvec, int32_t* h_root,
                              int32_t* h_iterations, double* d_pair_angle, double* h_ms) {
  const char* fn = "pxr_rotation_averaging";
  PXR_REQUIRE(ctx && o && d_qvec && h_root && h_iterations, "%s: NULL argument", fn);
  PXR_REQUIRE(n_images >= 1 && n_pairs >= 0, "%s: n_images = %d, n_pairs = %d", fn, (int)n_images, (int)n_pairs);
  PXR_REQUIRE(n_images - 1 <= PXR_MAX_IMAGES_DIRECT, "%s: n_images - 1 = %d exceeds PXR_MAX_IMAGES_DIRECT = %d (the dense solve)", fn,
              (int)n_images - 1, (int)PXR_MAX_IMAGES_DIRECT);
  PXR_REQUIRE(n_pairs == 0 || (d_pair_image && d_pair_qvec && d_pair_weight && d_pair_angle), "%s: NULL pair array", fn);
  PXR_REQUIRE(o->l1_iterations >= 0 && o->max_iterations >= 1 && o->min_angle > 0.0 && o->sigma > 0.0 && o->tolerance >= 0.0,
              "%s: option out of range", fn);
  PXR_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int n = n_images, P = n_pairs, m = n - 1;

  // ---- host: validation, root, spanning tree, adjacency ------------------------------------------------------------------------
  std::vector<int32_t> pim, adj_off, adj_pair;
  std::vector<double> pq((size_t)4 * P), pw, sum_w((size_t)n, 0.0);
  if (P > 0) PXR_HIP(hipMemcpyAsync(pq.data(), d_pair_qvec, sizeof(double) * 4 * (size_t)P, hipMemcpyDeviceToHost, st));
  const auto unit_qvec = [&](int p, int i, int j) {
    double* q = &pq[4 * (size_t)p];
    const double nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    PXR_REQUIRE(std::isfinite(nq) && nq > 0.0, "%s: the qvec of pair %d is zero or not finite", fn, p);
    for (int c = 0; c < 4; ++c) q[c] /= nq;
    sum_w[i] += pw[p]; sum_w[j] += pw[p];
    return (int)PXR_OK;
  };
  if (int rc = pair_list(ctx, fn, n, P, d_pair_image, d_pair_weight, pim, pw, adj_off, adj_pair, unit_qvec)) return rc;
  int root = 0;
  for (int k = 1; k < n; ++k) if (sum_w[k] > sum_w[root]) root = k;
  // Prim from the root over the pairs of positive weight: the heaviest pair that leaves the tree, the lower index of equals
  std::vector<double> q0((size_t)4 * n, 0.0);
  std::vector<char> in_tree((size_t)n, 0);
  in_tree[root] = 1; q0[4 * (size_t)root] = 1.0;
  for (int reached = 1; reached < n; ++reached) {
    int best = -1;
    for (int p = 0; p < P; ++p)
      if (in_tree[pim[2 * p]] != in_tree[pim[2 * p + 1]] && pw[p] > 0.0 && (best < 0 || pw[p] > pw[best])) best = p;
    PXR_REQUIRE(best >= 0, "%s: %d of %d images are not connected to the root (image %d) over pairs of positive weight", fn, n - reached, n, root);
    const int i = pim[2 * best], j = pim[2 * best + 1];
    const double* qp = &pq[4 * (size_t)best];
    if (in_tree[i]) {                                             // R_j = R_p R_i
      quat_mul(qp, &q0[4 * (size_t)i], &q0[4 * (size_t)j]);
      quat_canonical(&q0[4 * (size_t)j]);
      in_tree[j] = 1;
    } else {                                                      // R_i = R_p^t R_j
      double c[4];
      quat_conj(qp, c);
      quat_mul(c, &q0[4 * (size_t)j], &q0[4 * (size_t)i]);
      quat_canonical(&q0[4 * (size_t)i]);
      in_tree[i] = 1;
    }
  }

  // ---- device ---------------------------------------------------------------------------------------------------------------------
  const size_t n_aug = (size_t)(m + 1) * (m + 1);
  double *stat, *d_pq, *e, *rho, *ang, *aug, *linv, *omega; int* info; int32_t *d_off, *d_adj;
  Workspace ws;
  ws.take(stat, 2); ws.take(info, 4); ws.take(d_pq, (size_t)4 * P); ws.take(e, (size_t)3 * P);
  ws.take(rho, (size_t)P); ws.take(ang, (size_t)P); ws.take(d_off, (size_t)n + 1); ws.take(d_adj, (size_t)2 * P);
  ws.take(aug, n_aug); ws.take(linv, chol_workspace_doubles(std::max(m, 1))); ws.take(omega, (size_t)3 * std::max(m, 1));
  if (int rc = ws.commit(ctx)) return rc;

  if (h_ms) h_ms[0] = h_ms[1] = h_ms[2] = 0.0;
  StageTimer<4> timer(st, h_ms);                                  // residuals | assembly | solves (+ update)
  if (int rc = timer.create(fn)) return rc;
  PXR_HIP(hipMemcpyAsync(d_qvec, q0.data(), sizeof(double) * 4 * (size_t)n, hipMemcpyHostToDevice, st));
  PXR_HIP(hipMemcpyAsync(d_off, adj_off.data(), sizeof(int32_t) * ((size_t)n + 1), hipMemcpyHostToDevice, st));
  if (P > 0) {
    PXR_HIP(hipMemcpyAsync(d_pq, pq.data(), sizeof(double) * 4 * (size_t)P, hipMemcpyHostToDevice, st));
    PXR_HIP(hipMemcpyAsync(d_adj, adj_pair.data(), sizeof(int32_t) * 2 * (size_t)P, hipMemcpyHostToDevice, st));
  }
  *h_root = root;
  *h_iterations = 0;
  const double sigma = o->sigma * GM_DEG;
  for (int it = 0; m > 0 && it < o->max_iterations; ++it) {
    timer.mark(0);
    hipLaunchKernelGGL(k_ra_residual, blocks_for(P, GM_THREADS), dim3(GM_THREADS), 0, st, P, d_pair_image, d_pq, d_qvec, d_pair_weight,
                       it < o->l1_iterations ? 1 : 0, o->min_angle, sigma, e, rho, ang);
    timer.mark(1);
    // the three coordinates share the matrix; the factorisation overwrites it, so it is assembled three times.  The assembly
    // is timed with the solves it alternates with
    for (int coord = 0; coord < 3; ++coord) {
      PXR_HIP(hipMemsetAsync(aug, 0, sizeof(double) * n_aug, st));
      hipLaunchKernelGGL(k_ra_assemble, blocks_for(n, GM_THREADS), dim3(GM_THREADS), 0, st, n, root, coord, d_off, d_adj, d_pair_image, e, rho, aug);
      if (coord == 0) timer.mark(2);
      if (int rc = chol_factor_solve(st, aug, m, info, linv, omega + (size_t)coord * m, coord == 0)) return rc;
    }
    hipLaunchKernelGGL(k_ra_update, dim3(1), dim3(GM_THREADS), 0, st, n, root, omega, d_qvec, stat);
    timer.mark(3);
    int h_info = 0;
    double h_max = 0.0;
    PXR_HIP(hipMemcpyAsync(&h_info, info, sizeof(int), hipMemcpyDeviceToHost, st));
    PXR_HIP(hipMemcpyAsync(&h_max, stat, sizeof(double), hipMemcpyDeviceToHost, st));
    PXR_HIP(hipStreamSynchronize(st));
    if (int rc = timer.add()) return rc;
    if (h_info != 0 || !std::isfinite(h_max))
      return set_error(PXR_ENUMERIC, "%s: the Laplacian of iteration %d is not positive definite (pivot %d)", fn, it, h_info);
    *h_iterations = it + 1;
    if (it >= o->l1_iterations && h_max < o->tolerance) break;
  }
  if (P > 0)
    hipLaunchKernelGGL(k_ra_residual, blocks_for(P, GM_THREADS), dim3(GM_THREADS), 0, st, P, d_pair_image, d_pq, d_qvec, d_pair_weight, 0,
                       o->min_angle, sigma, e, rho, d_pair_angle);
  if (int rc = hip_check(hipGetLastError(), "k_ra_residual launch")) return rc;
  return hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
}

// ================================================================================================================================
// global positioning
// ================================================================================================================================
// a symmetric 3 x 3 is six doubles: 00 01 02 11 12 22.  P = I - d d^t times w, added to s
__device__ __forceinline__ void add_projector(double* s, const double* d, double w) {
  s[0] += w * (1.0 - d[0] * d[0]); s[1] += w * (-(d[0] * d[1])); s[2] += w * (-(d[0] * d[2]));
  s[3] += w * (1.0 - d[1] * d[1]); s[4] += w * (-(d[1] * d[2])); s[5] += w * (1.0 - d[2] * d[2]);
}
__device__ __forceinline__ void sym_mul(const double* s, const double* v, double* o) {
  o[0] = s[0] * v[0] + s[1] * v[1] + s[2] * v[2];
  o[1] = s[1] * v[0] + s[3] * v[1] + s[4] * v[2];
  o[2] = s[2] * v[0] + s[4] * v[1] + s[5] * v[2];
}
// (I - d d^t) v
__device__ __forceinline__ void project(const double* d, const double* v, double* o) {
  const double dv = d[0] * v[0] + d[1] * v[1] + d[2] * v[2];
  o[0] = v[0] - d[0] * dv; o[1] = v[1] - d[1] * dv; o[2] = v[2] - d[2] * dv;
}

__global__ __launch_bounds__(GM_THREADS) void k_gp_rays(const pxr_tri_view v, double* __restrict__ rays, uint8_t* __restrict__ ok_out,
                                                        double* __restrict__ w) {
  const int64_t i = (int64_t)blockIdx.x * GM_THREADS + threadIdx.x;
  if (i >= v.n_obs) return;
  const int img = v.d_obs_image[i], cam = v.d_image_camera[img];
  double k[PXR_KPAD], R[9];
#pragma unroll
  for (int j = 0; j < PXR_KPAD; ++j) k[j] = v.d_cam_params[(size_t)cam * PXR_KPAD + j];
  quat_to_rotation(v.d_qvec + 4 * (size_t)img, R);
  const double2 p = reinterpret_cast<const double2*>(v.d_obs_xy)[i];
  double un, vn, d[3];
  bool ok = image_to_world(v.d_cam_model[cam], k, p.x, p.y, un, vn);
  const double inv = 1.0 / sqrt(un * un + vn * vn + 1.0);
#pragma unroll
  for (int m = 0; m < 3; ++m) {                                   // d = R^t (u, v, 1) / |.|
    d[m] = (R[m] * un + R[3 + m] * vn + R[6 + m]) * inv;
    ok = ok && isfinite(d[m]);
  }
#pragma unroll
  for (int m = 0; m < 3; ++m) rays[3 * (size_t)i + m] = ok ? d[m] : 0.0;
  ok_out[i] = ok ? 1 : 0;
  w[i] = ok ? 1.0 : 0.0;
}

struct GpArgs {
  int64_t n_tracks;
  const int64_t* track_offsets;
  const int32_t* order;        // [n_tracks] tracks by descending length
  const int32_t* obs_image;
  const double* rays;          // [n_obs][3]
  const uint8_t* ok;           // [n_obs]
  double* w;                   // [n_obs] the observations' weights
  double* ainv;                // [n_tracks][6]
  uint8_t* valid;              // [n_tracks]
  int32_t n_images, root;
  unsigned long long* S;       // [3 n_images][3 n_images] fixed point (rows and columns of the root stay zero)
  double scale;                // 2^k of the fixed point
  double min_det, sigma_obs;
  const double* centre;        // [n_images][3]
  int cheirality, final_round;
  double* xyz; int32_t* status;
};

__global__ __launch_bounds__(64) void k_gp_tracks(const GpArgs a) {
  const int l = threadIdx.x & (GM_GROUP - 1);
  const int64_t t = (int64_t)blockIdx.x * GM_TPW + (threadIdx.x / GM_GROUP);
  if (t >= a.n_tracks) return;
  const int64_t o0 = a.track_offsets[t], o1 = a.track_offsets[t + 1];
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t o = o0 + l; o < o1; o += GM_GROUP) {
    const double w = a.w[o];
    if (w > 0.0) add_projector(s, a.rays + 3 * (size_t)o, w);
  }
#pragma unroll
  for (int j = 0; j < 6; ++j) s[j] = group_sum(s[j]);
  if (l != 0) return;
  const double c00 = s[3] * s[5] - s[4] * s[4], c01 = s[2] * s[4] - s[1] * s[5], c02 = s[1] * s[4] - s[2] * s[3];
  const double c11 = s[0] * s[5] - s[2] * s[2], c12 = s[1] * s[2] - s[0] * s[4], c22 = s[0] * s[3] - s[1] * s[1];
  const double det = s[0] * c00 + s[1] * c01 + s[2] * c02;
  const bool good = det > a.min_det;                             // (false for a NaN)
  const double r = good ? 1.0 / det : 0.0;
  double* out = a.ainv + 6 * (size_t)t;
  out[0] = c00 * r; out[1] = c01 * r; out[2] = c02 * r; out[3] = c11 * r; out[4] = c12 * r; out[5] = c22 * r;
  a.valid[t] = good ? 1 : 0;
}

// Fixed point.  Every addend of S is, in exact arithmetic, at most 1 in magnitude: w <= 1, |I - d d^t| = 1, and with
// B_a = w_a P_a <= A_k (positive-semidefinite order)  |u^t B_a A^-1 B_b v|^2 <= (u^t B_a A^-1 B_a u)(v^t B_b A^-1 B_b v) <= 1 for unit
// u, v (Cauchy-Schwarz, B A^-1 B <= B <= I); rounding in a badly conditioned A^-1 is covered by clamping the addend to [-2, 2].
// An entry of block row i receives at most  M_i = sum over the observations a of image i of len(track(a))  +  pairs of image i
// addends (one per ordered pair (a, b); the diagonal term of a is folded into the pair (a, a); a pair adds once to each of its
// blocks), so with M = max_i M_i and 2 M 2^k <= 2^62 no sum leaves the 64-bit range: k = 61 - ceil(log2 M), at most 60 (the host).
__device__ __forceinline__ void fixed_add(unsigned long long* slot, double v, double scale) {
  v = fmin(fmax(v, -2.0), 2.0);
  atomicAdd(slot, (unsigned long long)__double2ll_rn(v * scale));
}

__global__ __launch_bounds__(64) void k_gp_contract(const GpArgs a) {
  const int l = threadIdx.x & (GM_GROUP - 1);
  const int64_t slot = (int64_t)blockIdx.x * GM_TPW + (threadIdx.x / GM_GROUP);
  if (slot >= a.n_tracks) return;
  const int64_t t = a.order[slot];
  if (!a.valid[t]) return;
  const int64_t o0 = a.track_offsets[t], L = a.track_offsets[t + 1] - o0;
  double ai[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) ai[j] = a.ainv[6 * (size_t)t + j];
  const size_t ld = 3 * (size_t)a.n_images;
  for (int64_t idx = l; idx < L * L; idx += GM_GROUP) {
    const int64_t ka = idx / L, kb = idx - ka * L;
    const double wa = a.w[o0 + ka], wb = a.w[o0 + kb];
    const int i = a.obs_image[o0 + ka], j = a.obs_image[o0 + kb];
    if (!(wa > 0.0) || !(wb > 0.0) || i > j || i == a.root || j == a.root) continue;
    const double* da = a.rays + 3 * (size_t)(o0 + ka);
    const double* db = a.rays + 3 * (size_t)(o0 + kb);
    // M = w_a w_b P_a A^-1 P_b, row by row: q_c = column c of A^-1 P_b = A^-1 e_c - (A^-1 d_b) d_b[c]
    double adb[3], M[3][3];
    sym_mul(ai, db, adb);
    const double acol[3][3] = {{ai[0], ai[1], ai[2]}, {ai[1], ai[3], ai[4]}, {ai[2], ai[4], ai[5]}};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double qc[3], pc[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) qc[r] = acol[c][r] - adb[r] * db[c];
      project(da, qc, pc);
#pragma unroll
      for (int r = 0; r < 3; ++r) M[r][c] = -(wa * wb * pc[r]);
    }
    if (ka == kb) {                                               // + w_a P_a: the observation's own term of S_ii
      double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      add_projector(s, da, wa);
      M[0][0] += s[0]; M[0][1] += s[1]; M[0][2] += s[2]; M[1][0] += s[1]; M[1][1] += s[3]; M[1][2] += s[4];
      M[2][0] += s[2]; M[2][1] += s[4]; M[2][2] += s[5];
    }
    unsigned long long* blk = a.S + (3 * (size_t)i) * ld + 3 * (size_t)j;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (i != j || r <= c) fixed_add(blk + r * ld + c, M[r][c], a.scale);
  }
}

struct GpPairArgs {
  int32_t n_pairs, n_images, root;
  const int32_t* pair_image; const double* pair_dir;
  const double* w0;            // [n_pairs] w_p / max w
  double* robust;              // [n_pairs] the pairs' robust factors
  const int32_t* adj_off; const int32_t* adj_pair;
  unsigned long long* S; double scale;
  double* g;                   // [3 n_images]
  double* stat;                // [0] h, [1] g . y
  const double* centre; double sigma_pair; int cheirality;
  double* weight_out;
};

__global__ __launch_bounds__(GM_THREADS) void k_gp_pairs(const GpPairArgs a) {
  const int p = blockIdx.x * GM_THREADS + threadIdx.x;
  if (p >= a.n_pairs) return;
  const double w = a.w0[p] * a.robust[p];
  if (!(w > 0.0)) return;
  const int i0 = a.pair_image[2 * p], j0 = a.pair_image[2 * p + 1];
  const int i = min(i0, j0), j = max(i0, j0);
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  add_projector(s, a.pair_dir + 3 * (size_t)p, w);
  const double full[3][3] = {{s[0], s[1], s[2]}, {s[1], s[3], s[4]}, {s[2], s[4], s[5]}};
  const size_t ld = 3 * (size_t)a.n_images;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (r <= c && i != a.root) fixed_add(a.S + (3 * (size_t)i + r) * ld + 3 * (size_t)i + c, full[r][c], a.scale);
      if (r <= c && j != a.root) fixed_add(a.S + (3 * (size_t)j + r) * ld + 3 * (size_t)j + c, full[r][c], a.scale);
      if (i != a.root && j != a.root) fixed_add(a.S + (3 * (size_t)i + r) * ld + 3 * (size_t)j + c, -full[r][c], a.scale);
    }
}

// g_j += w b, g_i -= w b per image over its pairs in ascending pair index; h = sum w
__global__ __launch_bounds__(GM_THREADS) void k_gp_gauge(const GpPairArgs a) {
  __shared__ double sh[GM_THREADS];
  const int tid = threadIdx.x;
  for (int k = tid; k < a.n_images; k += GM_THREADS) {
    double g[3] = {0.0, 0.0, 0.0};
    for (int x = a.adj_off[k]; x < a.adj_off[k + 1]; ++x) {
      const int p = a.adj_pair[x];
      const double w = a.w0[p] * a.robust[p];
      const double sw = a.pair_image[2 * p + 1] == k ? w : -w;
#pragma unroll
      for (int c = 0; c < 3; ++c) g[c] += sw * a.pair_dir[3 * (size_t)p + c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) a.g[3 * (size_t)k + c] = g[c];
  }
  double h = 0.0;
  for (int p = tid; p < a.n_pairs; p += GM_THREADS) h += a.w0[p] * a.robust[p];
  h = block_sum(h, sh);
  if (tid == 0) a.stat[0] = h;
}

// [S | g] without the root, m = 3 (n_images - 1): rows 0 .. m - 1, upper triangle; the last row and the lower triangle zero
__global__ __launch_bounds__(GM_THREADS) void k_gp_pack(int32_t n_images, int32_t root, const unsigned long long* __restrict__ S, double inv_scale,
                                                        const double* __restrict__ g, double* __restrict__ aug) {
  const int m = 3 * (n_images - 1), ld = m + 1;
  const int64_t t = (int64_t)blockIdx.x * GM_THREADS + threadIdx.x;
  if (t >= (int64_t)ld * ld) return;
  const int r = (int)(t / ld), c = (int)(t - (int64_t)r * ld);
  double v = 0.0;
  if (r < m) {
    const int fr = r + (r / 3 >= root ? 3 : 0);
    if (c == m) v = g[fr];
    else if (r <= c) v = (double)(long long)S[(size_t)fr * (3 * (size_t)n_images) + (c + (c / 3 >= root ? 3 : 0))] * inv_scale;
  }
  aug[t] = v;
}

// c = h y / (g . y); flag[0] = 1 where the factorisation met a non-positive pivot or g . y is not positive (centres untouched)
__global__ __launch_bounds__(GM_THREADS) void k_gp_scale(int32_t n_images, int32_t root, const double* __restrict__ g, const double* __restrict__ y,
                                                         const double* __restrict__ stat, const int* __restrict__ info, int* __restrict__ flag,
                                                         double* __restrict__ centre) {
  __shared__ double sh[GM_THREADS];
  const int tid = threadIdx.x, m = 3 * (n_images - 1);
  double s = 0.0;
  for (int r = tid; r < m; r += GM_THREADS) s += g[r + (r / 3 >= root ? 3 : 0)] * y[r];
  const double gy = block_sum(s, sh);
  const bool good = info[0] == 0 && gy > 0.0 && isfinite(gy);
  if (!good) { if (tid == 0) flag[0] = 1; return; }
  const double k = stat[0] / gy;
  for (int r = tid; r < m; r += GM_THREADS) centre[r + (r / 3 >= root ? 3 : 0)] = k * y[r];
  if (tid < 3) centre[3 * (size_t)root + tid] = 0.0;
}

// the robust weight of a ray d (or a baseline b) against v = target - origin; 0 where v is zero or not finite
__device__ __forceinline__ double robust_weight(const double* d, const double* v, double sigma, int cheirality) {
  double pv[3];
  project(d, v, pv);
  const double n2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
  if (!(n2 > 0.0) || !isfinite(n2)) return 0.0;
  if (cheirality && !(d[0] * v[0] + d[1] * v[1] + d[2] * v[2] > 0.0)) return 0.0;
  const double s = sqrt((pv[0] * pv[0] + pv[1] * pv[1] + pv[2] * pv[2]) / n2) / sigma;
  return 1.0 / (1.0 + s * s);
}

__global__ __launch_bounds__(64) void k_gp_update(const GpArgs a) {
  const int l = threadIdx.x & (GM_GROUP - 1);
  const int64_t t = (int64_t)blockIdx.x * GM_TPW + (threadIdx.x / GM_GROUP);
  if (t >= a.n_tracks) return;
  const int64_t o0 = a.track_offsets[t], o1 = a.track_offsets[t + 1];
  const bool valid = a.valid[t] != 0;
  double b[3] = {0.0, 0.0, 0.0}, X[3];
  for (int64_t o = o0 + l; valid && o < o1; o += GM_GROUP) {
    const double w = a.w[o];
    if (!(w > 0.0)) continue;
    double pc[3];
    project(a.rays + 3 * (size_t)o, a.centre + 3 * (size_t)a.obs_image[o], pc);
#pragma unroll
    for (int c = 0; c < 3; ++c) b[c] += w * pc[c];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) b[c] = group_sum(b[c]);
  sym_mul(a.ainv + 6 * (size_t)t, b, X);
  for (int64_t o = o0 + l; o < o1; o += GM_GROUP) {
    double w = 0.0;
    if (valid && a.ok[o]) {
      const double* c = a.centre + 3 * (size_t)a.obs_image[o];
      const double v[3] = {X[0] - c[0], X[1] - c[1], X[2] - c[2]};
      w = robust_weight(a.rays + 3 * (size_t)o, v, a.sigma_obs, a.cheirality);
    }
    a.w[o] = w;
  }
  if (a.final_round && l == 0) {
    a.status[t] = valid ? 0 : 1;
    if (valid) { a.xyz[3 * (size_t)t] = X[0]; a.xyz[3 * (size_t)t + 1] = X[1]; a.xyz[3 * (size_t)t + 2] = X[2]; }
  }
}

__global__ __launch_bounds__(GM_THREADS) void k_gp_pair_update(const GpPairArgs a) {
  const int p = blockIdx.x * GM_THREADS + threadIdx.x;
  if (p >= a.n_pairs) return;
  const double* ci = a.centre + 3 * (size_t)a.pair_image[2 * p];
  const double* cj = a.centre + 3 * (size_t)a.pair_image[2 * p + 1];
  const double v[3] = {cj[0] - ci[0], cj[1] - ci[1], cj[2] - ci[2]};
  const double r = robust_weight(a.pair_dir + 3 * (size_t)p, v, a.sigma_pair, a.cheirality);
  a.robust[p] = r;
  a.weight_out[p] = a.w0[p] * r;
}

static int global_positioning(pxr_ctx* ctx, const pxr_tri_view* v, int32_t n_pairs, const int32_t* d_pair_image, const double* d_pair_dir,
                              const double* d_pair_weight, int32_t root, const pxr_globalpos_options* o, double* d_centre, double* d_xyz,
                              int32_t* d_track_status, double* d_obs_weight, double* d_pair_weight_out, int32_t* h_status, int32_t* h_rounds,
                              double* h_ms) {
  const char* fn = "pxr_global_positioning";
  PXR_REQUIRE(ctx && v && o && h_status && h_rounds && d_centre, "%s: NULL argument", fn);
  PXR_REQUIRE(v->n_tracks >= 0 && v->n_obs >= 0 && v->n_images >= 1 && v->n_cameras >= 0 && n_pairs >= 0, "%s: negative size or no image", fn);
  PXR_REQUIRE(v->n_obs < ((int64_t)1 << 31) && v->n_tracks < ((int64_t)1 << 31), "%s: more than 2^31 observations or tracks", fn);
  PXR_REQUIRE(v->n_tracks == 0 || (v->d_track_offsets && d_xyz && d_track_status), "%s: NULL track array", fn);
  PXR_REQUIRE(v->n_obs == 0 || (v->d_obs_image && v->d_obs_xy && d_obs_weight && v->d_image_camera && v->d_qvec && v->d_cam_model &&
                                v->d_cam_params), "%s: NULL observation / image / camera array", fn);
  PXR_REQUIRE(v->n_obs == 0 || v->n_tracks > 0, "%s: observations without tracks", fn);
  PXR_REQUIRE(n_pairs == 0 || (d_pair_image && d_pair_dir && d_pair_weight && d_pair_weight_out), "%s: NULL pair array", fn);
  PXR_REQUIRE(root >= 0 && root < v->n_images, "%s: root = %d outside [0, n_images = %d)", fn, (int)root, (int)v->n_images);
  PXR_REQUIRE(v->n_images - 1 <= PXR_MAX_IMAGES_DIRECT, "%s: 3 (n_images - 1) = %d exceeds the dense solve's limit 3 PXR_MAX_IMAGES_DIRECT", fn,
              3 * ((int)v->n_images - 1));
  PXR_REQUIRE(o->iterations >= 1 && o->cheirality_from >= 0 && o->sigma_obs > 0.0 && o->sigma_pair > 0.0 && o->min_det >= 0.0,
              "%s: option out of range", fn);
  PXR_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int64_t T = v->n_tracks, N = v->n_obs;
  const int n = v->n_images, P = n_pairs, m = 3 * (n - 1);

  // ---- host: validation, the tracks' order, the adjacency, the fixed-point scale -------------------------------------------------
  std::vector<int64_t> off(1, 0);
  std::vector<int32_t> order, oim((size_t)N), icam((size_t)n);
  if (T > 0) {                                                    // (batch_order waits for the two downloads too)
    if (N > 0) PXR_HIP(hipMemcpyAsync(oim.data(), v->d_obs_image, sizeof(int32_t) * (size_t)N, hipMemcpyDeviceToHost, st));
    if (v->d_image_camera) PXR_HIP(hipMemcpyAsync(icam.data(), v->d_image_camera, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
    if (int rc = batch_order(ctx, {fn, "track_offsets", "track", "n_obs"}, false, v->d_track_offsets, T, N, off, order, [](int64_t) { return (int)PXR_OK; }))
      return rc;
  }
  std::vector<int64_t> addends((size_t)n, 0);                     // M_i of the fixed-point bound (k_gp_contract)
  for (int64_t t = 0; t < T; ++t)
    for (int64_t x = off[t]; x < off[t + 1]; ++x) {
      PXR_REQUIRE(oim[x] >= 0 && oim[x] < n, "%s: an observation names an image outside [0, n_images = %d)", fn, n);
      addends[oim[x]] += off[t + 1] - off[t];
    }
  if (N > 0)
    for (int k = 0; k < n; ++k)
      PXR_REQUIRE(icam[k] >= 0 && icam[k] < v->n_cameras, "%s: an image names a camera outside [0, n_cameras = %d)", fn, (int)v->n_cameras);
  std::vector<int32_t> pim, adj_off, adj_pair;
  std::vector<double> pdir((size_t)3 * P), pw;
  if (P > 0) PXR_HIP(hipMemcpyAsync(pdir.data(), d_pair_dir, sizeof(double) * 3 * (size_t)P, hipMemcpyDeviceToHost, st));
  double w_max = 0.0;
  const auto unit_direction = [&](int p, int i, int j) {
    const double* b = &pdir[3 * (size_t)p];
    const double nb = std::sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
    PXR_REQUIRE(std::isfinite(nb) && std::fabs(nb - 1.0) <= 1e-9, "%s: the direction of pair %d is not a finite unit vector", fn, p);
    w_max = std::max(w_max, pw[p]);
    ++addends[i]; ++addends[j];
    return (int)PXR_OK;
  };
  if (int rc = pair_list(ctx, fn, n, P, d_pair_image, d_pair_weight, pim, pw, adj_off, adj_pair, unit_direction)) return rc;
  for (int p = 0; p < P; ++p) pw[p] = w_max > 0.0 ? pw[p] / w_max : 0.0;
  int64_t M = 1;
  for (int k = 0; k < n; ++k) M = std::max(M, addends[k]);
  int bits = 0;
  while (((int64_t)1 << bits) < M) ++bits;                        // ceil(log2 M)
  const double scale = std::ldexp(1.0, std::min(61 - bits, 60));

  // ---- device ---------------------------------------------------------------------------------------------------------------------
  const size_t n_aug = (size_t)(m + 1) * (m + 1), n_S = 9 * (size_t)n * n;
  GpArgs a;
  double *stat, *rays, *w0, *robust, *g, *aug, *linv, *y; int *info, *flag; uint8_t* ok; int32_t *d_order, *d_off, *d_adj; unsigned long long* S;
  Workspace ws;
  ws.take(stat, 2); ws.take(info, 4); ws.take(flag, 4);
  ws.take(rays, (size_t)3 * N); ws.take(ok, (size_t)N); ws.take(d_order, (size_t)T);
  ws.take(a.ainv, (size_t)6 * T); ws.take(a.valid, (size_t)T);
  ws.take(w0, (size_t)P); ws.take(robust, (size_t)P); ws.take(d_off, (size_t)n + 1); ws.take(d_adj, (size_t)2 * P);
  ws.take(g, (size_t)3 * n); ws.take(S, n_S); ws.take(aug, n_aug);
  ws.take(linv, chol_workspace_doubles(std::max(m, 1))); ws.take(y, (size_t)std::max(m, 1));
  if (int rc = ws.commit(ctx)) return rc;

  if (h_ms) for (int k = 0; k < 5; ++k) h_ms[k] = 0.0;
  StageTimer<6> timer(st, h_ms);                                  // tracks | contraction (+ pairs) | gauge + pack | Cholesky | scale + updates
  if (int rc = timer.create(fn)) return rc;
  if (T > 0) PXR_HIP(hipMemcpyAsync(d_order, order.data(), sizeof(int32_t) * (size_t)T, hipMemcpyHostToDevice, st));
  PXR_HIP(hipMemcpyAsync(d_off, adj_off.data(), sizeof(int32_t) * ((size_t)n + 1), hipMemcpyHostToDevice, st));
  if (P > 0) {
    PXR_HIP(hipMemcpyAsync(d_adj, adj_pair.data(), sizeof(int32_t) * 2 * (size_t)P, hipMemcpyHostToDevice, st));
    PXR_HIP(hipMemcpyAsync(w0, pw.data(), sizeof(double) * (size_t)P, hipMemcpyHostToDevice, st));
    std::vector<double> ones((size_t)P, 1.0);
    PXR_HIP(hipMemcpyAsync(robust, ones.data(), sizeof(double) * (size_t)P, hipMemcpyHostToDevice, st));
    PXR_HIP(hipStreamSynchronize(st));                             // (`ones` goes out of scope)
  }
  PXR_HIP(hipMemsetAsync(flag, 0, 16, st));
  PXR_HIP(hipMemsetAsync(d_centre, 0, sizeof(double) * 3 * (size_t)n, st));

  a.n_tracks = T; a.track_offsets = v->d_track_offsets; a.order = d_order; a.obs_image = v->d_obs_image;
  a.rays = rays; a.ok = ok; a.w = d_obs_weight; a.n_images = n; a.root = root; a.S = S; a.scale = scale; a.min_det = o->min_det;
  a.sigma_obs = o->sigma_obs * GM_DEG; a.centre = d_centre; a.cheirality = 0; a.final_round = 0; a.xyz = d_xyz; a.status = d_track_status;
  GpPairArgs b;
  b.n_pairs = P; b.n_images = n; b.root = root; b.pair_image = d_pair_image; b.pair_dir = d_pair_dir; b.w0 = w0; b.robust = robust;
  b.adj_off = d_off; b.adj_pair = d_adj; b.S = S; b.scale = scale; b.g = g; b.stat = stat; b.centre = d_centre;
  b.sigma_pair = o->sigma_pair * GM_DEG; b.cheirality = 0; b.weight_out = d_pair_weight_out;

  if (N > 0) hipLaunchKernelGGL(k_gp_rays, blocks_for(N, GM_THREADS), dim3(GM_THREADS), 0, st, *v, rays, ok, d_obs_weight);
  *h_status = 0;
  *h_rounds = 0;
  for (int it = 0; it < o->iterations; ++it) {
    a.cheirality = b.cheirality = it >= o->cheirality_from ? 1 : 0;
    a.final_round = it == o->iterations - 1 ? 1 : 0;
    timer.mark(0);
    if (T > 0) hipLaunchKernelGGL(k_gp_tracks, blocks_for(T, GM_TPW), dim3(64), 0, st, a);
    timer.mark(1);
    if (m > 0) {
      PXR_HIP(hipMemsetAsync(S, 0, sizeof(unsigned long long) * n_S, st));
      if (T > 0) hipLaunchKernelGGL(k_gp_contract, blocks_for(T, GM_TPW), dim3(64), 0, st, a);
      if (P > 0) hipLaunchKernelGGL(k_gp_pairs, blocks_for(P, GM_THREADS), dim3(GM_THREADS), 0, st, b);
    }
    timer.mark(2);
    if (m > 0) {
      hipLaunchKernelGGL(k_gp_gauge, dim3(1), dim3(GM_THREADS), 0, st, b);
      hipLaunchKernelGGL(k_gp_pack, blocks_for((int64_t)n_aug, GM_THREADS), dim3(GM_THREADS), 0, st, n, root, S, 1.0 / scale, g, aug);
    }
    timer.mark(3);
    if (m > 0)
      if (int rc = chol_factor_solve(st, aug, m, info, linv, y, true)) return rc;
    timer.mark(4);
    int h_flag = 0;
    if (m > 0) {
      hipLaunchKernelGGL(k_gp_scale, dim3(1), dim3(GM_THREADS), 0, st, n, root, g, y, stat, info, flag, d_centre);
      // the round's info word: nothing of a degenerate round goes on (the centres are the previous round's)
      PXR_HIP(hipMemcpyAsync(&h_flag, flag, sizeof(int), hipMemcpyDeviceToHost, st));
      PXR_HIP(hipStreamSynchronize(st));
    }
    if (h_flag) { *h_status = 1; break; }
    if (T > 0) hipLaunchKernelGGL(k_gp_update, blocks_for(T, GM_TPW), dim3(64), 0, st, a);
    if (P > 0) hipLaunchKernelGGL(k_gp_pair_update, blocks_for(P, GM_THREADS), dim3(GM_THREADS), 0, st, b);
    timer.mark(5);
    *h_rounds = it + 1;
    if (h_ms) {
      PXR_HIP(hipStreamSynchronize(st));
      if (int rc = timer.add()) return rc;
    }
  }
  if (int rc = hip_check(hipGetLastError(), "k_gp launch")) return rc;
  return hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
}

}  // namespace pxr

extern "C" void pxr_rotavg_default_options(pxr_rotavg_options* o) {
  if (!o) return;
  o->l1_iterations = 20; o->max_iterations = 40; o->min_angle = 1e-3; o->sigma = 5.0; o->tolerance = 1e-10;
}

extern "C" int pxr_rotation_averaging(pxr_ctx* ctx, int32_t n_images, int32_t n_pairs, const int32_t* d_pair_image, const double* d_pair_qvec,
                                      const double* d_pair_weight, const pxr_rotavg_options* options, double* d_qvec, int32_t* h_root,
                                      int32_t* h_iterations, double* d_pair_angle) {
  return pxr::rotation_averaging(ctx, n_images, n_pairs, d_pair_image, d_pair_qvec, d_pair_weight, options, d_qvec, h_root, h_iterations,
                                 d_pair_angle, nullptr);
}

extern "C" int pxr_rotation_averaging_timed(pxr_ctx* ctx, int32_t n_images, int32_t n_pairs, const int32_t* d_pair_image,
                                            const double* d_pair_qvec, const double* d_pair_weight, const pxr_rotavg_options* options,
                                            double* d_qvec, int32_t* h_root, int32_t* h_iterations, double* d_pair_angle, double* h_kernel_ms) {
  PXR_REQUIRE(h_kernel_ms, "pxr_rotation_averaging_timed: NULL h_kernel_ms");
  return pxr::rotation_averaging(ctx, n_images, n_pairs, d_pair_image, d_pair_qvec, d_pair_weight, options, d_qvec, h_root, h_iterations,
                                 d_pair_angle, h_kernel_ms);
}

extern "C" void pxr_globalpos_default_options(pxr_globalpos_options* o) {
  if (!o) return;
  o->iterations = 8; o->cheirality_from = 2; o->sigma_obs = 1.0; o->sigma_pair = 3.0; o->min_det = 1e-12;
}

extern "C" int pxr_global_positioning(pxr_ctx* ctx, const pxr_tri_view* view, int32_t n_pairs, const int32_t* d_pair_image,
                                      const double* d_pair_dir, const double* d_pair_weight, int32_t root, const pxr_globalpos_options* options,
                                      double* d_centre, double* d_xyz, int32_t* d_track_status, double* d_obs_weight, double* d_pair_weight_out,
                                      int32_t* h_status, int32_t* h_rounds) {
  return pxr::global_positioning(ctx, view, n_pairs, d_pair_image, d_pair_dir, d_pair_weight, root, options, d_centre, d_xyz, d_track_status,
                                 d_obs_weight, d_pair_weight_out, h_status, h_rounds, nullptr);
}

extern "C" int pxr_global_positioning_timed(pxr_ctx* ctx, const pxr_tri_view* view, int32_t n_pairs, const int32_t* d_pair_image,
                                            const double* d_pair_dir, const double* d_pair_weight, int32_t root,
                                            const pxr_globalpos_options* options, double* d_centre, double* d_xyz, int32_t* d_track_status,
                                            double* d_obs_weight, double* d_pair_weight_out, int32_t* h_status, int32_t* h_rounds,
                                            double* h_kernel_ms) {
  PXR_REQUIRE(h_kernel_ms, "pxr_global_positioning_timed: NULL h_kernel_ms");
  return pxr::global_positioning(ctx, view, n_pairs, d_pair_image, d_pair_dir, d_pair_weight, root, options, d_centre, d_xyz, d_track_status,
                                 d_obs_weight, d_pair_weight_out, h_status, h_rounds, h_kernel_ms);
}
