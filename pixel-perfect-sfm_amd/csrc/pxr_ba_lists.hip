// pxr_ba_lists.hip -- the structure of a BA solve on the device: block layout, observation lists per image and per point, the
// chunkings and the flattened index chains of the Schur / back-substitution kernels.  First stage of pxr_ba_solve /
// pxr_ba_solve_geometric (pxr_ba_solve.hip); the host-side rules are in pxr_ba_structure.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "pxr_ba_driver.h"
#include "pxr_scan.h"

namespace pxr {

// ---- set-up: flattened index chains of the Schur / back-substitution kernels ------------------------------------
// obs_cols[o] / part_obs[o]: column descriptor and observation id of slot o of the point-ordered list;
// so[o]: {observation, point, first partner slot, partner count (0 = constant point)} of slot o of the image-ordered list
__global__ __launch_bounds__(256) void k_build_descriptors(int64_t n_obs, const int32_t* __restrict__ obs_image,
                                                           const int32_t* __restrict__ obs_point,
                                                           const int32_t* __restrict__ image_camera,
                                                           const int64_t* __restrict__ pt_obs, const int64_t* __restrict__ img_obs,
                                                           const int64_t* __restrict__ pt_ptr, const int* __restrict__ pt_var,
                                                           const int* __restrict__ pose_off, const int* __restrict__ pose_dim,
                                                           const int* __restrict__ intr_off, const int* __restrict__ intr_dim,
                                                           int4* __restrict__ obs_cols, int* __restrict__ part_obs,
                                                           int4* __restrict__ so) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= n_obs) return;
  const int64_t j = pt_obs[o];
  const int im = obs_image[j], cm = image_camera[im];
  obs_cols[o] = make_int4(pose_off[im], pose_dim[im], intr_off[cm], intr_dim[cm]);
  part_obs[o] = (int)j;
  const int64_t i = img_obs[o];
  const int64_t pt = obs_point[i];
  so[o] = make_int4((int)i, (int)pt, (int)pt_ptr[pt], pt_var[pt] ? (int)(pt_ptr[pt + 1] - pt_ptr[pt]) : 0);
}

// ---- observation lists on the device (set-up) -------------------------------------------------------------------------
// counts per image / per point, index range check, and whether the observations are ordered by point (then the
// point-ordered list is the identity); flags[0] = out-of-range index seen, flags[1] = a point index decreases
// (the image counts are histogrammed in LDS per chunk of COUNT_CHUNK observations: a million global atomics on the ~13 cache
//  lines of 200 image counters took 0.5 ms of every solve, profiles/r6_lm_setup.txt)
constexpr int COUNT_CHUNK = 4096;
__global__ __launch_bounds__(256) void k_count_indices(int64_t n_obs, const int32_t* __restrict__ obs_image,
                                                       const int32_t* __restrict__ obs_point, int n_img, int64_t n_pts,
                                                       unsigned long long* __restrict__ img_cnt, unsigned long long* __restrict__ pt_cnt,
                                                       int* __restrict__ flags) {
  extern __shared__ unsigned int sh_img[];                 // n_img counters (n_img <= SORT_MAX_IMAGES)
  for (int k = threadIdx.x; k < n_img; k += 256) sh_img[k] = 0u;
  __syncthreads();
  const int64_t i0 = (int64_t)blockIdx.x * COUNT_CHUNK, i1 = min(n_obs, i0 + COUNT_CHUNK);
  for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
    const int im = obs_image[i], pt = obs_point[i];
    if (im < 0 || im >= n_img || pt < 0 || pt >= n_pts) { atomicOr(&flags[0], 1); continue; }
    atomicAdd(&sh_img[im], 1u);
    atomicAdd(&pt_cnt[pt + 1], 1ull);
    if (i > 0 && obs_point[i - 1] > pt) atomicOr(&flags[1], 1);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < n_img; k += 256)
    if (sh_img[k]) atomicAdd(&img_cnt[k + 1], (unsigned long long)sh_img[k]);
}
// the per-point side of the structure without a trip to the host (200k points: 1.6 MB each way through pageable memory were
// 0.5 ms of every solve): pt_ptr = prefix sums of the counts k_count_indices left in cnt[p + 1] (cnt[0] = 0), pt_var[p] = the point
// is not constant and has an observation, *n_var = how many.  Two launches: the sums of chunks of PT_SCAN_CHUNK points, then
// every workgroup adds up the chunks before its own and scans its chunk.
constexpr int PT_SCAN_CHUNK = 2048;
__global__ __launch_bounds__(256) void k_pt_scan_partials(int64_t n_pts, const unsigned long long* __restrict__ cnt, unsigned long long* __restrict__ part) {
  __shared__ unsigned long long s_part[256 / 64];
  const int64_t p0 = (int64_t)blockIdx.x * PT_SCAN_CHUNK;
  unsigned long long s = 0;
  for (int j = threadIdx.x; j < PT_SCAN_CHUNK; j += 256) if (p0 + j < n_pts) s += cnt[p0 + j + 1];
  s = block_int_sum<256>(s, s_part);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void k_pt_scan_apply(int64_t n_pts, const unsigned long long* __restrict__ cnt, const unsigned long long* __restrict__ part,
                                                       const uint8_t* __restrict__ pt_const, int64_t* __restrict__ pt_ptr, int* __restrict__ pt_var,
                                                       unsigned long long* __restrict__ n_var) {
  __shared__ unsigned long long s_part[256 / 64];
  constexpr int PER = PT_SCAN_CHUNK / 256;
  const int t = threadIdx.x;
  unsigned long long base = 0;
  for (int g = t; g < (int)blockIdx.x; g += 256) base += part[g];
  base = block_int_sum<256>(base, s_part);
  const int64_t p0 = (int64_t)blockIdx.x * PT_SCAN_CHUNK + (int64_t)t * PER;
  unsigned long long c[PER], mine = 0;
  int nv = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    c[j] = p0 + j < n_pts ? cnt[p0 + j + 1] : 0ull;
    mine += c[j];
  }
  unsigned long long chunk_total;
  unsigned long long run = base + block_exclusive_scan<256>(mine, s_part, chunk_total);
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    if (p0 + j >= n_pts) break;
    run += c[j];
    pt_ptr[p0 + j + 1] = (int64_t)run;
    const int v = (!pt_const[p0 + j] && c[j] > 0) ? 1 : 0;
    pt_var[p0 + j] = v; nv += v;
  }
  if (blockIdx.x == 0 && t == 0) pt_ptr[0] = 0;
  const unsigned long long tot = block_int_sum<256>((unsigned long long)nv, s_part);
  if (t == 0 && tot) atomicAdd(n_var, tot);
}
__global__ void k_iota(int64_t n, int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = i;
}
// STABLE counting sort of the observation ids by image (the order the host fill produces: ascending observation id inside
// an image -- the summation order of k_img and of the Schur contraction, which must not depend on the run):
//   k_sort_hist     a workgroup counts the images of its contiguous chunk of SORT_CHUNK observations,
//   k_sort_offsets  per image, an exclusive scan of those counts over the chunks on top of the image's first slot,
//   k_sort_scatter  the workgroup walks its chunk in order, 256 observations a round: slot = running offset of the image +
//                   number of EARLIER observations of the round with the same image.
constexpr int SORT_CHUNK = 4096, SORT_MAX_IMAGES = 8192;
__global__ __launch_bounds__(256) void k_sort_hist(int64_t n_obs, const int32_t* __restrict__ obs_image, int n_img,
                                                   int* __restrict__ hist) {
  extern __shared__ int sh_cnt[];
  for (int k = threadIdx.x; k < n_img; k += blockDim.x) sh_cnt[k] = 0;
  __syncthreads();
  const int64_t b0 = (int64_t)blockIdx.x * SORT_CHUNK, b1 = min(n_obs, b0 + SORT_CHUNK);
  for (int64_t i = b0 + threadIdx.x; i < b1; i += blockDim.x) atomicAdd(&sh_cnt[obs_image[i]], 1);
  __syncthreads();
  for (int k = threadIdx.x; k < n_img; k += blockDim.x) hist[(size_t)blockIdx.x * n_img + k] = sh_cnt[k];
}
__global__ void k_sort_offsets(int n_img, int n_chunks, const int64_t* __restrict__ img_ptr, int* __restrict__ hist) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_img) return;
  int run = (int)img_ptr[k];
  for (int b = 0; b < n_chunks; ++b) {
    const int c = hist[(size_t)b * n_img + k];
    hist[(size_t)b * n_img + k] = run;
    run += c;
  }
}
__global__ __launch_bounds__(256) void k_sort_scatter(int64_t n_obs, const int32_t* __restrict__ obs_image, int n_img,
                                                      const int* __restrict__ hist, int64_t* __restrict__ img_obs) {
  extern __shared__ int sh_off[];          // [n_img] running offsets, then [256] the keys of the round
  int* keys = sh_off + n_img;
  for (int k = threadIdx.x; k < n_img; k += blockDim.x) sh_off[k] = hist[(size_t)blockIdx.x * n_img + k];
  const int64_t b0 = (int64_t)blockIdx.x * SORT_CHUNK, b1 = min(n_obs, b0 + SORT_CHUNK);
  for (int64_t r0 = b0; r0 < b1; r0 += 256) {
    const int64_t i = r0 + threadIdx.x;
    const int key = i < b1 ? obs_image[i] : -1;
    __syncthreads();                       // offsets initialised / updated by the previous round
    keys[threadIdx.x] = key;
    __syncthreads();
    int before = 0, after = 0;
    if (key >= 0) {
      for (int t = 0; t < 256; ++t) {
        const int same = keys[t] == key;
        before += same & (t < (int)threadIdx.x);
        after += same & (t > (int)threadIdx.x);
      }
      img_obs[sh_off[key] + before] = i;
    }
    __syncthreads();                       // every slot of the round is computed from the old offsets
    if (key >= 0 && after == 0) sh_off[key] += before + 1;
  }
}

// Fast path (observations ordered by point -- what every caller of this library produces -- and at most SORT_MAX_IMAGES images):
// the 2 x n_obs index arrays never leave the device; only the per-image COUNTS come to the host, the lists are built by a stable
// counting sort on the device.  Otherwise (and with PXR_BA_SETUP_HOST=1, for the equivalence test) the lists are built on the
// host from a copy of the index arrays (host_lists, pxr_ba_structure.h).
int build_structure(pxr_ctx* ctx, const pxr_ba_view* view, const uint8_t* h_pose_const, const uint8_t* h_tvec_const_mask,
                    const uint16_t* h_cam_const_mask, const uint8_t* h_point_const, const SolveKnobs& knobs, const SetupClock& clock,
                    SolveStructure* out) {
  SolveStructure& s = *out;
  hipStream_t st = ctx->stream;
  const int64_t n_obs = view->n_obs, n_pts = view->n_points;
  const int n_img = view->n_images, n_cam = view->n_cameras;
  StructError err;
  std::vector<int32_t> obs_image, obs_point;               // the general host path only
  s.image_camera.resize(n_img); s.cam_model.resize(n_cam);
  s.img_ptr.assign(n_img + 1, 0);
  s.device_lists = n_img <= SORT_MAX_IMAGES && !knobs.setup_host;
  PXR_HIP(hipMemcpyAsync(s.image_camera.data(), view->d_image_camera, 4 * n_img, hipMemcpyDeviceToHost, st));
  PXR_HIP(hipMemcpyAsync(s.cam_model.data(), view->d_cam_model, 4 * n_cam, hipMemcpyDeviceToHost, st));
  clock.mark("camera tables read");
  // ---- counts per image / per point, the range check, whether the input is ordered by point
  if (s.device_lists) {
    int h_flags[2] = {0, 0};
    RC(s.d_cnt.alloc((size_t)n_img + 1 + (size_t)n_pts + 1 + 1)); RC(s.d_flags.alloc(2));     // ... + the number of variable points
    clock.mark("counter buffers");
    PXR_HIP(hipMemsetAsync(s.d_cnt.p, 0, sizeof(unsigned long long) * s.d_cnt.n, st));
    PXR_HIP(hipMemsetAsync(s.d_flags.p, 0, sizeof(int) * 2, st));
    hipLaunchKernelGGL(k_count_indices, dim3((unsigned)((n_obs + COUNT_CHUNK - 1) / COUNT_CHUNK)), dim3(256), sizeof(unsigned int) * n_img, st, n_obs, view->d_obs_image,
                       view->d_obs_point, n_img, n_pts, s.d_cnt.p, s.d_cnt.p + n_img + 1, s.d_flags.p);
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "counter width");
    PXR_HIP(hipMemcpyAsync(s.img_ptr.data(), s.d_cnt.p, sizeof(int64_t) * (n_img + 1), hipMemcpyDeviceToHost, st));
    PXR_HIP(hipMemcpyAsync(h_flags, s.d_flags.p, sizeof(int) * 2, hipMemcpyDeviceToHost, st));
    PXR_HIP(hipStreamSynchronize(st));
    PXR_REQUIRE(h_flags[0] == 0, "pxr_ba_solve: an observation references an image / point out of range");
    if (h_flags[1]) s.device_lists = false;                 // not ordered by point: the general host path
  }
  if (!s.device_lists) {
    obs_image.resize(n_obs); obs_point.resize(n_obs);
    PXR_HIP(hipMemcpyAsync(obs_image.data(), view->d_obs_image, 4 * n_obs, hipMemcpyDeviceToHost, st));
    PXR_HIP(hipMemcpyAsync(obs_point.data(), view->d_obs_point, 4 * n_obs, hipMemcpyDeviceToHost, st));
  }
  PXR_HIP(hipStreamSynchronize(st));
  clock.mark(s.device_lists ? "counts on the host" : "index arrays on the host");
  // ---- host: block layout, lists (general path) or prefix sums (fast path), chunks
  if (block_layout(n_img, n_cam, h_pose_const, h_tvec_const_mask, h_cam_const_mask, s.cam_model.data(), &s.layout, &err)) return struct_error(err);
  const BlockLayout& l = s.layout;
  HostLists& hl = s.host;
  if (!s.device_lists) {
    if (host_lists(n_obs, obs_image.data(), obs_point.data(), n_img, n_pts, h_point_const, l.n_c, &hl, &err)) return struct_error(err);
    s.img_ptr = hl.img_ptr; s.n_pvar = hl.n_pvar;
  } else {
    for (int i = 0; i < n_img; ++i) s.img_ptr[i + 1] += s.img_ptr[i];
  }
  clock.mark(s.device_lists ? "host prefix sums" : "host CSR (counts, fill)");
  s.chunks = chunk_images(s.img_ptr, 512);                  // observations per k_img workgroup (4 LDS batches)
  // Schur contraction: larger chunks (fewer LDS flushes), and per-observation column descriptors so the inner loop does not
  // chase obs -> image -> camera -> offsets
  s.schur_chunks = chunk_images(s.img_ptr, 1024);
  PXR_REQUIRE(n_obs < ((int64_t)1 << 31), "pxr_ba_solve: more than 2^31 observations per rank");
  clock.mark("host structure (CSR, chunks)");
  // ---- device
  RC(s.d_pose_off.upload(l.pose_off, st)); RC(s.d_pose_dim.upload(l.pose_dim, st)); RC(s.d_tmask.upload(l.tmask, st));
  RC(s.d_intr_off.upload(l.intr_off, st)); RC(s.d_intr_dim.upload(l.intr_dim, st)); RC(s.d_cmask.upload(l.cmask, st));
  RC(s.d_chunks.upload(s.chunks, st));
  if (s.device_lists) {
    // offsets, variable flags and their number from the counts that never left the device (k_pt_scan_*)
    unsigned long long h_n_pvar = 0;
    const int n_parts = (int)((n_pts + PT_SCAN_CHUNK - 1) / PT_SCAN_CHUNK);
    unsigned long long* const d_pt_cnt = s.d_cnt.p + n_img + 1;
    RC(s.d_pt_var.alloc(n_pts)); RC(s.d_pt_ptr.alloc((size_t)n_pts + 1)); RC(s.d_pt_const.alloc(n_pts)); RC(s.d_pt_part.alloc(n_parts));
    PXR_HIP(hipMemcpyAsync(s.d_pt_const.p, h_point_const, (size_t)n_pts, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_pt_scan_partials, dim3(n_parts), dim3(256), 0, st, n_pts, (const unsigned long long*)d_pt_cnt, s.d_pt_part.p);
    hipLaunchKernelGGL(k_pt_scan_apply, dim3(n_parts), dim3(256), 0, st, n_pts, (const unsigned long long*)d_pt_cnt, (const unsigned long long*)s.d_pt_part.p,
                       (const uint8_t*)s.d_pt_const.p, s.d_pt_ptr.p, s.d_pt_var.p, d_pt_cnt + n_pts + 1);
    PXR_HIP(hipMemcpyAsync(&h_n_pvar, d_pt_cnt + n_pts + 1, sizeof(h_n_pvar), hipMemcpyDeviceToHost, st));
    RC(s.d_img_obs.alloc(n_obs)); RC(s.d_pt_obs.alloc(n_obs));
    hipLaunchKernelGGL(k_iota, blocks_for(n_obs, 256), dim3(256), 0, st, n_obs, s.d_pt_obs.p);     // ordered by point already
    DevBuf<int64_t> d_img_ptr;
    DevBuf<int> d_hist;
    const int n_chunks = (int)((n_obs + SORT_CHUNK - 1) / SORT_CHUNK);
    RC(d_img_ptr.upload(s.img_ptr, st)); RC(d_hist.alloc((size_t)n_chunks * n_img));
    hipLaunchKernelGGL(k_sort_hist, dim3(n_chunks), dim3(256), sizeof(int) * n_img, st, n_obs, view->d_obs_image, n_img, d_hist.p);
    hipLaunchKernelGGL(k_sort_offsets, dim3((n_img + 255) / 256), dim3(256), 0, st, n_img, n_chunks, d_img_ptr.p, d_hist.p);
    hipLaunchKernelGGL(k_sort_scatter, dim3(n_chunks), dim3(256), sizeof(int) * (n_img + 256), st, n_obs, view->d_obs_image, n_img,
                       d_hist.p, s.d_img_obs.p);
    LAUNCH_CHECK("observation-list kernels");
    clock.mark("list kernels launched");
    PXR_HIP(hipStreamSynchronize(st));      // d_img_ptr / d_hist go out of scope
    clock.mark("list kernels done");
    s.n_pvar = (int64_t)h_n_pvar;
    if (require_variable_block(l.n_c, s.n_pvar, &err)) return struct_error(err);
  } else {
    RC(s.d_pt_var.upload(hl.pt_var, st)); RC(s.d_pt_ptr.upload(hl.pt_ptr, st));
    RC(s.d_img_obs.upload(hl.img_obs, st)); RC(s.d_pt_obs.upload(hl.pt_obs, st));
  }
  RC(s.d_schur_chunks.upload(s.schur_chunks, st));
  RC(s.d_obs_cols.alloc(n_obs)); RC(s.d_so.alloc(n_obs)); RC(s.d_part_obs.alloc(n_obs));
  hipLaunchKernelGGL(k_build_descriptors, blocks_for(n_obs, 256), dim3(256), 0, st, n_obs, view->d_obs_image, view->d_obs_point,
                     view->d_image_camera, s.d_pt_obs.p, s.d_img_obs.p, s.d_pt_ptr.p, s.d_pt_var.p, s.d_pose_off.p, s.d_pose_dim.p,
                     s.d_intr_off.p, s.d_intr_dim.p, s.d_obs_cols.p, s.d_part_obs.p, s.d_so.p);
  LAUNCH_CHECK("k_build_descriptors");
  clock.mark("index uploads");
  return PXR_OK;
}

}  // namespace pxr
