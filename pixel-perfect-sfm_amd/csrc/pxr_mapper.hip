// pxr_mapper.hip -- the device step of incremental mapping on gfx950 between triangulation and registration: which images see
// which triangulated points, how well those points are spread over the image, and the 2D-3D pairs every image gets.
//
// Replaces, for a whole batch of candidate images at once, [upstream COLMAP 3.8] IncrementalMapper::FindNextImages (the ranking
// by VisibilityPyramid::Score) and the 2D-3D gathering at the head of IncrementalMapper::RegisterNextImage -- as remembered,
// parity unpinned.  Everything here is integer arithmetic and copies: the outputs are a function of the
// input alone, bit for bit.
//
//   k_map_check   one workgroup per image: the image-major transpose is what it claims to be (indices in range, ascending inside
//                 an image, every observation filed under its own image), obs_track / image_camera in range, camera sizes positive
//   k_map_count   one workgroup per image: visible observations counted, their pyramid cells marked as bit words in LDS
//                 (atomicOr), the score summed from the population counts of the words
//   k_exclusive_scan (pxr_scan.h)   corr_offsets = exclusive scan of n_visible
//   k_map_write   one workgroup per image: the visible observations written in ascending observation order -- a prefix sum over
//                 the lanes of a wavefront by shuffles, over the wavefronts through LDS, chunk after chunk
//
// Every branch that encloses __syncthreads or a shuffle is uniform over the workgroup.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "pxr_batch.h"
#include "pxr_internal.h"
#include "pxr_scan.h"

namespace pxr {

constexpr int MAP_THREADS = 256;
constexpr int MAP_WAVES = MAP_THREADS / 64;
constexpr int MAP_MAX_LEVELS = 6;
constexpr int MAP_WORDS = 172;       // level l = 1 .. 6 owns max(1, 4^l / 32) words: 1 + 1 + 2 + 8 + 32 + 128

struct MapArgs {
  pxr_tri_view v;
  const int64_t* obs_track;          // [n_obs]
  const int64_t* image_obs_offsets;  // [n_images + 1]
  const int64_t* image_obs;          // [n_obs]
  const double* xyz;                 // [n_tracks][3]
  const int32_t* status;             // [n_tracks]
  const uint8_t* image_mask;         // [n_images]
  const int32_t* cam_size;           // [n_cameras][2]
  const int32_t* order;              // [n_images] images by descending number of observations
  int32_t levels;
  int32_t* n_visible; int64_t* score; int64_t* corr_offsets; int64_t* corr_obs; double* corr_xy; double* corr_xyz;
};

// the first word of level l (1-based) and the words it owns
__device__ __forceinline__ int map_level_first(int l) { return l <= 2 ? l - 1 : l == 3 ? 2 : l == 4 ? 4 : l == 5 ? 12 : 44; }
__device__ __forceinline__ int map_level_words(int l) { return l <= 2 ? 1 : 1 << (2 * l - 5); }

__device__ __forceinline__ bool map_visible(const MapArgs& a, int64_t o) {
  const int64_t t = a.obs_track[o];
  if (a.status[t] != 0) return false;
  const double* X = a.xyz + 3 * t;
  const double* p = a.v.d_obs_xy + 2 * o;
  return isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]) && isfinite(p[0]) && isfinite(p[1]);
}

// clamp((int)floor(x 2^L / size), 0, 2^L - 1), clamped before the conversion (x is finite)
__device__ __forceinline__ int map_cell(double x, int levels, int size) {
  const double f = floor(x * (double)(1 << levels) / (double)size), top = (double)((1 << levels) - 1);
  return f < 0.0 ? 0 : f > top ? (1 << levels) - 1 : (int)f;
}

// ---- validation --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MAP_THREADS) void k_map_check(const MapArgs a, int* __restrict__ flag) {
  const int32_t img = blockIdx.x;
  int bad = 0;
  if (threadIdx.x == 0) { const int32_t c = a.v.d_image_camera[img]; if (c < 0 || c >= a.v.n_cameras) bad |= 2; }
  if (img == 0)
    for (int c = threadIdx.x; c < a.v.n_cameras; c += MAP_THREADS)
      if (a.cam_size[2 * c] <= 0 || a.cam_size[2 * c + 1] <= 0) bad |= 16;
  const int64_t k0 = a.image_obs_offsets[img], k1 = a.image_obs_offsets[img + 1];
  for (int64_t k = k0 + threadIdx.x; k < k1; k += MAP_THREADS) {
    const int64_t o = a.image_obs[k];
    if (o < 0 || o >= a.v.n_obs) { bad |= 4; continue; }
    if (a.v.d_obs_image[o] != img || (k > k0 && a.image_obs[k - 1] >= o)) bad |= 8;
    const int64_t t = a.obs_track[o];
    if (t < 0 || t >= a.v.n_tracks) bad |= 1;
  }
  if (bad) atomicOr(flag, bad);
}

// ---- pass 1: counts and occupancy ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MAP_THREADS) void k_map_count(const MapArgs a) {
  __shared__ int s_bits[MAP_WORDS];
  __shared__ long long s_part[MAP_WAVES];
  const int32_t img = a.order[blockIdx.x];
  if (!a.image_mask[img]) {
    if (threadIdx.x == 0) { a.n_visible[img] = 0; a.score[img] = 0; }
    return;
  }
  const int L = a.levels, words = map_level_first(L) + map_level_words(L);
  for (int w = threadIdx.x; w < words; w += MAP_THREADS) s_bits[w] = 0;
  __syncthreads();
  const int32_t cam = a.v.d_image_camera[img];
  const int W = a.cam_size[2 * cam], H = a.cam_size[2 * cam + 1];
  const int64_t k0 = a.image_obs_offsets[img], k1 = a.image_obs_offsets[img + 1];
  long long count = 0;
  for (int64_t k = k0 + threadIdx.x; k < k1; k += MAP_THREADS) {
    const int64_t o = a.image_obs[k];
    if (!map_visible(a, o)) continue;
    ++count;
    const int cx = map_cell(a.v.d_obs_xy[2 * o], L, W), cy = map_cell(a.v.d_obs_xy[2 * o + 1], L, H);
    for (int l = 1; l <= L; ++l) {
      const int bit = ((cy >> (L - l)) << l) | (cx >> (L - l));               // < 4^l
      atomicOr(&s_bits[map_level_first(l) + (bit >> 5)], (int)(1u << (bit & 31)));
    }
  }
  __syncthreads();
  long long score = 0;
  for (int l = 1; l <= L; ++l) {
    const int first = map_level_first(l), nw = map_level_words(l);
    for (int w = threadIdx.x; w < nw; w += MAP_THREADS) score += ((long long)1 << (2 * l)) * __builtin_popcount((unsigned)s_bits[first + w]);
  }
  count = block_int_sum<MAP_THREADS>(count, s_part);
  score = block_int_sum<MAP_THREADS>(score, s_part);
  if (threadIdx.x == 0) { a.n_visible[img] = (int32_t)count; a.score[img] = score; }
}

// ---- pass 2: the ordered write ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MAP_THREADS) void k_map_write(const MapArgs a) {
  __shared__ long long s_part[MAP_WAVES];
  const int32_t img = a.order[blockIdx.x];
  if (!a.image_mask[img] || a.n_visible[img] == 0) return;
  const int64_t k0 = a.image_obs_offsets[img], k1 = a.image_obs_offsets[img + 1];
  int64_t at = a.corr_offsets[img];
  for (int64_t kb = k0; kb < k1; kb += MAP_THREADS) {
    const int64_t k = kb + threadIdx.x;
    const int64_t o = k < k1 ? a.image_obs[k] : -1;
    const bool vis = o >= 0 && map_visible(a, o);
    long long total;
    const long long before = block_exclusive_scan<MAP_THREADS>((long long)(vis ? 1 : 0), s_part, total);
    if (vis) {
      const int64_t j = at + before;
      const int64_t t = a.obs_track[o];
      a.corr_obs[j] = o;
      a.corr_xy[2 * j] = a.v.d_obs_xy[2 * o]; a.corr_xy[2 * j + 1] = a.v.d_obs_xy[2 * o + 1];
      a.corr_xyz[3 * j] = a.xyz[3 * t]; a.corr_xyz[3 * j + 1] = a.xyz[3 * t + 1]; a.corr_xyz[3 * j + 2] = a.xyz[3 * t + 2];
    }
    at += total;
  }
}

static int mapper_visibility(pxr_ctx* ctx, const pxr_tri_view* v, const int64_t* d_obs_track, const int64_t* d_image_obs_offsets,
                             const int64_t* d_image_obs, const double* d_xyz, const int32_t* d_status, const uint8_t* d_image_mask,
                             const int32_t* d_cam_size, int32_t pyramid_levels, int32_t* d_n_visible, int64_t* d_score,
                             int64_t* d_corr_offsets, int64_t* d_corr_obs, double* d_corr_xy, double* d_corr_xyz, int64_t* h_n_corr,
                             double* h_ms) {
  const char* fn = "pxr_mapper_visibility";
  PXR_REQUIRE(ctx && v && h_n_corr, "%s: NULL argument", fn);
  PXR_REQUIRE(v->n_tracks >= 0 && v->n_obs >= 0 && v->n_images >= 0 && v->n_cameras >= 0, "%s: negative size", fn);
  PXR_REQUIRE(v->n_obs < ((int64_t)1 << 31) && v->n_tracks < ((int64_t)1 << 31), "%s: more than 2^31 observations or tracks", fn);
  PXR_REQUIRE(pyramid_levels >= 1 && pyramid_levels <= MAP_MAX_LEVELS, "%s: pyramid_levels = %d outside [1, %d]", fn, (int)pyramid_levels,
              MAP_MAX_LEVELS);
  PXR_REQUIRE(v->d_track_offsets && d_image_obs_offsets && d_corr_offsets, "%s: NULL offsets array", fn);
  PXR_REQUIRE(v->n_images == 0 || (v->d_image_camera && d_image_mask && d_cam_size && d_n_visible && d_score), "%s: NULL image / camera array", fn);
  PXR_REQUIRE(v->n_obs == 0 || (v->d_obs_image && v->d_obs_xy && d_obs_track && d_image_obs && d_corr_obs && d_corr_xy && d_corr_xyz),
              "%s: NULL observation array", fn);
  PXR_REQUIRE(v->n_tracks == 0 || (d_xyz && d_status), "%s: NULL track array", fn);
  if (h_ms) h_ms[0] = h_ms[1] = h_ms[2] = h_ms[3] = 0.0;
  PXR_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int64_t T = v->n_tracks, N = v->n_obs;
  const int32_t I = v->n_images;

  // both offsets arrays are validated on host copies; the images' one also gives the processing order (most observations first)
  std::vector<int64_t> off;
  std::vector<int32_t> order, track_order;
  auto none = [](int64_t) { return (int)PXR_OK; };
  if (int rc = batch_order(ctx, {fn, "track_offsets", "track", "n_obs"}, true, v->d_track_offsets, T, N, off, track_order, none)) return rc;
  if (int rc = batch_order(ctx, {fn, "image_obs_offsets", "image", "n_obs"}, false, d_image_obs_offsets, I, N, off, order, none)) return rc;
  if (I == 0) {
    PXR_HIP(hipMemsetAsync(d_corr_offsets, 0, sizeof(int64_t), st));
    *h_n_corr = 0;
    return hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
  }

  int* flag; int32_t* d_order;
  Workspace ws;
  ws.take(flag, 4); ws.take(d_order, (size_t)I);
  if (int rc = ws.commit(ctx)) return rc;

  MapArgs a;
  a.v = *v; a.obs_track = d_obs_track; a.image_obs_offsets = d_image_obs_offsets; a.image_obs = d_image_obs; a.xyz = d_xyz;
  a.status = d_status; a.image_mask = d_image_mask; a.cam_size = d_cam_size; a.order = d_order; a.levels = pyramid_levels;
  a.n_visible = d_n_visible; a.score = d_score; a.corr_offsets = d_corr_offsets; a.corr_obs = d_corr_obs; a.corr_xy = d_corr_xy;
  a.corr_xyz = d_corr_xyz;

  StageTimer<6> timer(st, h_ms);                         // check | (the flag's read-back) | count | scan | write
  if (int rc = timer.create(fn)) return rc;

  int h_flag = 0;
  int rc = hip_check(hipMemsetAsync(flag, 0, 16, st), "hipMemsetAsync");
  if (rc == PXR_OK) {
    timer.mark(0);
    hipLaunchKernelGGL(k_map_check, dim3((unsigned)I), dim3(MAP_THREADS), 0, st, a, flag);
    timer.mark(1);
    rc = hip_check(hipMemcpyAsync(&h_flag, flag, 4, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
  }
  if (rc == PXR_OK) rc = hip_check(hipMemcpyAsync(d_order, order.data(), sizeof(int32_t) * (size_t)I, hipMemcpyHostToDevice, st), "hipMemcpyAsync");
  if (rc == PXR_OK) rc = hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");      // (also: `order` may go out of scope)
  if (rc != PXR_OK) return rc;
  if (h_flag) {
    if (h_flag & 4) return set_error(PXR_EINVAL, "%s: image_obs names an observation outside [0, n_obs = %lld)", fn, (long long)N);
    if (h_flag & 8) return set_error(PXR_EINVAL, "%s: image_obs is not the image-major transpose of obs_image, ascending inside an image", fn);
    if (h_flag & 1) return set_error(PXR_EINVAL, "%s: an observation names a track outside [0, n_tracks = %lld)", fn, (long long)T);
    if (h_flag & 2) return set_error(PXR_EINVAL, "%s: an image names a camera outside [0, n_cameras = %d)", fn, (int)v->n_cameras);
    return set_error(PXR_EINVAL, "%s: a camera has a width or height that is not positive", fn);
  }

  timer.mark(2);
  hipLaunchKernelGGL(k_map_count, dim3((unsigned)I), dim3(MAP_THREADS), 0, st, a);
  timer.mark(3);
  hipLaunchKernelGGL((k_exclusive_scan<MAP_THREADS, int32_t, int64_t>), dim3(1), dim3(MAP_THREADS), 0, st, (int64_t)I, (const int32_t*)d_n_visible,
                     d_corr_offsets, 1);
  timer.mark(4);
  hipLaunchKernelGGL(k_map_write, dim3((unsigned)I), dim3(MAP_THREADS), 0, st, a);
  timer.mark(5);
  rc = hip_check(hipGetLastError(), "k_map_write launch");
  int64_t total = 0;
  if (rc == PXR_OK) rc = hip_check(hipMemcpyAsync(&total, d_corr_offsets + I, sizeof(int64_t), hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
  if (rc == PXR_OK) rc = hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
  if (rc != PXR_OK) return rc;
  *h_n_corr = total;
  const int from[4] = {0, 2, 3, 4};
  return timer.read(from, 4);
}

}  // namespace pxr

extern "C" int pxr_mapper_visibility(pxr_ctx* ctx, const pxr_tri_view* view, const int64_t* d_obs_track, const int64_t* d_image_obs_offsets,
                                     const int64_t* d_image_obs, const double* d_xyz, const int32_t* d_status,
                                     const uint8_t* d_image_mask, const int32_t* d_cam_size, int32_t pyramid_levels,
                                     int32_t* d_n_visible, int64_t* d_score, int64_t* d_corr_offsets, int64_t* d_corr_obs,
                                     double* d_corr_xy, double* d_corr_xyz, int64_t* h_n_corr) {
  return pxr::mapper_visibility(ctx, view, d_obs_track, d_image_obs_offsets, d_image_obs, d_xyz, d_status, d_image_mask, d_cam_size,
                                pyramid_levels, d_n_visible, d_score, d_corr_offsets, d_corr_obs, d_corr_xy, d_corr_xyz, h_n_corr, nullptr);
}

extern "C" int pxr_mapper_visibility_timed(pxr_ctx* ctx, const pxr_tri_view* view, const int64_t* d_obs_track,
                                           const int64_t* d_image_obs_offsets, const int64_t* d_image_obs, const double* d_xyz,
                                           const int32_t* d_status, const uint8_t* d_image_mask, const int32_t* d_cam_size,
                                           int32_t pyramid_levels, int32_t* d_n_visible, int64_t* d_score, int64_t* d_corr_offsets,
                                           int64_t* d_corr_obs, double* d_corr_xy, double* d_corr_xyz, int64_t* h_n_corr,
                                           double* h_kernel_ms) {
  PXR_REQUIRE(h_kernel_ms, "pxr_mapper_visibility_timed: NULL h_kernel_ms");
  return pxr::mapper_visibility(ctx, view, d_obs_track, d_image_obs_offsets, d_image_obs, d_xyz, d_status, d_image_mask, d_cam_size,
                                pyramid_levels, d_n_visible, d_score, d_corr_offsets, d_corr_obs, d_corr_xy, d_corr_xyz, h_n_corr,
                                h_kernel_ms);
}
