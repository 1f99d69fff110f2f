// pxr_localize.hip -- the glue of batched map localization on gfx950: which map images see the same points
// (covisibility counts and each image's best partners), the covisibility clusters of every query's retrieved images, and the 2D-3D
// pairs of every (query, cluster) gathered from the matcher's device output in the order pxr_absolute_pose takes them.
//
// Replaces hloc.pairs_from_covisibility, hloc.localize_sfm.do_covisibility_clustering and the gathering of
// hloc.localize_sfm.pose_from_cluster as pixsfm/localize.py:main uses them -- as remembered, parity unpinned.  Everything here is
// integer arithmetic and copies: the outputs are a function of the input alone, bit for bit.
//
//   k_covis_check     a thread per observation: its image index is in range
//   k_covis_count     a track per 16 lanes, the L^2 ordered pairs of its observations strided over them with a running (a, b);
//                     global int32 atomicAdd (integer addition commutes: the same bits every run)
//   k_covis_topk      one workgroup per row: the best partner that is worse than the previous one, num_matched times
//   k_cluster_check   a thread per retrieved entry: its image index is in range
//   k_cluster         one wavefront per query, lane r = entry r: a 64-bit adjacency mask per lane, its transitive closure by
//                     shuffles, component = lowest set bit, size = population count, number = rank among the components
//   k_loc_walk        a lane per (problem, query keypoint): <false> counts the pairs the keypoint emits, checks the indices it
//                     reads and sums the counts of its workgroup (block_int_sum); <true> places the lane -- the workgroup's start
//                     plus block_exclusive_scan of the counts -- repeats the walk and writes
//   k_exclusive_scan (pxr_scan.h)   where every workgroup writes (one element per 256 lanes: a single-workgroup scan over the
//                     lanes themselves measured 6.5 ms at 2M lanes, three times the two walks together)
//   k_loc_offsets     corr_offsets of the problems out of the lanes' starts
//
// Every branch that encloses __syncthreads, a shuffle or a ballot is uniform over the lanes that exchange there.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "pxr_batch.h"
#include "pxr_internal.h"
#include "pxr_scan.h"

namespace pxr {

constexpr int LOC_THREADS = 256;
constexpr int LOC_WAVES = LOC_THREADS / 64;
constexpr int LOC_MAX_LIST = PXR_MAX_LOC_ENTRIES;   // retrieved images of a query, entries of a problem: one wavefront, one 64-bit mask
constexpr int LOC_INDEX_BITS = 13;        // PXR_MAX_COVIS_IMAGES = 2^13: (count, -index) packs into one 64-bit key
static_assert(PXR_MAX_COVIS_IMAGES == 1 << LOC_INDEX_BITS, "the top-k key packs the image index into LOC_INDEX_BITS bits");

// ---- covisibility counts -------------------------------------------------------------------------------------------------------
struct CovisArgs {
  int32_t n_images;
  int64_t n_tracks;
  const int64_t* track_offsets;   // [n_tracks + 1]
  int64_t n_obs;
  const int32_t* obs_image;       // [n_obs]
  const uint8_t* track_mask;      // [n_tracks] or NULL
  const int32_t* order;           // [n_tracks] tracks by descending length: the 16-lane groups of a wavefront get tracks alike
  int32_t* count;                 // [n_images][n_images]
};

__global__ __launch_bounds__(LOC_THREADS) void k_covis_check(const CovisArgs a, int* __restrict__ flag) {
  const int64_t o = (int64_t)blockIdx.x * LOC_THREADS + threadIdx.x;
  if (o >= a.n_obs) return;
  const int32_t i = a.obs_image[o];
  if (i < 0 || i >= a.n_images) atomicOr(flag, 1);
}

__global__ __launch_bounds__(LOC_THREADS) void k_covis_count(const CovisArgs a) {
  const int64_t g = ((int64_t)blockIdx.x * LOC_THREADS + threadIdx.x) >> 4;
  const int sub = threadIdx.x & 15;
  if (g >= a.n_tracks) return;
  const int64_t t = a.order[g];
  if (a.track_mask && !a.track_mask[t]) return;
  const int64_t o0 = a.track_offsets[t], L = a.track_offsets[t + 1] - o0;
  if (L < 2) return;
  // item n = a L + b of the L^2 ordered pairs, n = sub, sub + 16, ...: (a, b) advances by (16 / L, 16 % L) with one carry
  const int64_t da = 16 / L, db = 16 % L;
  int64_t pa = sub / L, pb = sub % L, held = -1;
  int32_t ia = 0;
  while (pa < L) {
    if (pa != held) { ia = a.obs_image[o0 + pa]; held = pa; }
    const int32_t ib = a.obs_image[o0 + pb];
    if (ia != ib) atomicAdd(&a.count[(int64_t)ia * a.n_images + ib], 1);
    pa += da; pb += db;
    if (pb >= L) { pb -= L; ++pa; }
  }
}

// the largest v of the workgroup, on every thread; s_part has LOC_WAVES slots
__device__ __forceinline__ unsigned long long loc_block_max(unsigned long long v, unsigned long long* s_part) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const unsigned long long w = __shfl_xor(v, off, 64); v = w > v ? w : v; }
  __syncthreads();                              // (the previous use of s_part is over)
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned long long m = 0;
#pragma unroll
  for (int w = 0; w < LOC_WAVES; ++w) m = s_part[w] > m ? s_part[w] : m;
  return m;
}

// Row i: partner j with count c > 0 has the key (c << 13) | (8191 - j), distinct over j, so "the next best" is the largest key
// below the previous one: (count descending, index ascending).  `best` is uniform over the workgroup, and so is every branch on it.
__global__ __launch_bounds__(LOC_THREADS) void k_covis_topk(int32_t n_images, const int32_t* __restrict__ count, int32_t K,
                                                            int32_t* __restrict__ topk_index, int32_t* __restrict__ topk_count,
                                                            int32_t* __restrict__ n_topk) {
  __shared__ unsigned long long s_part[LOC_WAVES];
  const int32_t i = blockIdx.x;
  const int32_t* row = count + (int64_t)i * n_images;
  const unsigned long long low = ((unsigned long long)1 << LOC_INDEX_BITS) - 1;
  unsigned long long prev = ~(unsigned long long)0;
  int32_t n = 0;
  for (; n < K; ++n) {
    unsigned long long best = 0;
    for (int32_t j = threadIdx.x; j < n_images; j += LOC_THREADS) {
      const int32_t c = row[j];
      if (c <= 0) continue;
      const unsigned long long key = ((unsigned long long)c << LOC_INDEX_BITS) | (low - (unsigned long long)j);
      if (key < prev && key > best) best = key;
    }
    best = loc_block_max(best, s_part);
    if (best == 0) break;
    if (threadIdx.x == 0) {
      topk_index[(int64_t)i * K + n] = (int32_t)(low - (best & low));
      topk_count[(int64_t)i * K + n] = (int32_t)(best >> LOC_INDEX_BITS);
    }
    prev = best;
  }
  for (int32_t r = n + threadIdx.x; r < K; r += LOC_THREADS) { topk_index[(int64_t)i * K + r] = -1; topk_count[(int64_t)i * K + r] = 0; }
  if (threadIdx.x == 0) n_topk[i] = n;
}

static int covisibility(pxr_ctx* ctx, int32_t n_images, int64_t n_tracks, const int64_t* d_track_offsets, int64_t n_obs,
                        const int32_t* d_obs_image, const uint8_t* d_track_mask, int32_t num_matched, int32_t* d_count,
                        int32_t* d_topk_index, int32_t* d_topk_count, int32_t* d_n_topk, double* h_ms) {
  const char* fn = "pxr_covisibility";
  PXR_REQUIRE(ctx, "%s: NULL context", fn);
  PXR_REQUIRE(n_images >= 0 && n_tracks >= 0 && n_obs >= 0, "%s: negative size", fn);
  PXR_REQUIRE(n_images <= PXR_MAX_COVIS_IMAGES, "%s: %d images, more than PXR_MAX_COVIS_IMAGES = %d (the count matrix is dense)", fn,
              (int)n_images, (int)PXR_MAX_COVIS_IMAGES);
  PXR_REQUIRE(n_obs < ((int64_t)1 << 31) && n_tracks < ((int64_t)1 << 31), "%s: 2^31 observations or tracks, or more", fn);
  const bool topk = d_topk_index || d_topk_count || d_n_topk;
  PXR_REQUIRE(!topk || (d_topk_index && d_topk_count && d_n_topk), "%s: the three top-k outputs come together or not at all", fn);
  PXR_REQUIRE(!topk || (num_matched >= 1 && num_matched <= PXR_MAX_COVIS_MATCHED), "%s: num_matched = %d outside [1, %d]", fn,
              (int)num_matched, (int)PXR_MAX_COVIS_MATCHED);
  PXR_REQUIRE(d_track_offsets, "%s: NULL track_offsets", fn);
  PXR_REQUIRE(n_obs == 0 || d_obs_image, "%s: NULL obs_image", fn);
  PXR_REQUIRE(n_images == 0 || d_count, "%s: NULL count", fn);
  if (h_ms) h_ms[0] = h_ms[1] = h_ms[2] = 0.0;
  PXR_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;

  std::vector<int64_t> off;
  std::vector<int32_t> order;
  auto none = [](int64_t) { return (int)PXR_OK; };
  if (int rc = batch_order(ctx, {fn, "track_offsets", "track", "n_obs"}, false, d_track_offsets, n_tracks, n_obs, off, order, none)) return rc;
  PXR_REQUIRE(n_images > 0 || n_obs == 0, "%s: observations without images", fn);
  if (n_images == 0) return PXR_OK;

  int* flag; int32_t* d_order;
  Workspace ws;
  ws.take(flag, 4); ws.take(d_order, (size_t)n_tracks);
  if (int rc = ws.commit(ctx)) return rc;
  CovisArgs a;
  a.n_images = n_images; a.n_tracks = n_tracks; a.track_offsets = d_track_offsets; a.n_obs = n_obs; a.obs_image = d_obs_image;
  a.track_mask = d_track_mask; a.order = d_order; a.count = d_count;

  StageTimer<5> timer(st, h_ms);                         // check | (the flag's read-back) | count | topk
  if (int rc = timer.create(fn)) return rc;
  int h_flag = 0;
  int rc = hip_check(hipMemsetAsync(flag, 0, 16, st), "hipMemsetAsync");
  if (rc == PXR_OK) {
    timer.mark(0);
    if (n_obs > 0) hipLaunchKernelGGL(k_covis_check, blocks_for(n_obs, LOC_THREADS), dim3(LOC_THREADS), 0, st, a, flag);
    timer.mark(1);
    rc = hip_check(hipMemcpyAsync(&h_flag, flag, 4, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
  }
  if (rc == PXR_OK && n_tracks > 0)
    rc = hip_check(hipMemcpyAsync(d_order, order.data(), sizeof(int32_t) * (size_t)n_tracks, hipMemcpyHostToDevice, st), "hipMemcpyAsync");
  if (rc == PXR_OK) rc = hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");      // (also: `order` may go out of scope)
  if (rc != PXR_OK) return rc;
  if (h_flag) return set_error(PXR_EINVAL, "%s: an observation names an image outside [0, n_images = %d)", fn, (int)n_images);

  rc = hip_check(hipMemsetAsync(d_count, 0, sizeof(int32_t) * (size_t)n_images * (size_t)n_images, st), "hipMemsetAsync");
  if (rc != PXR_OK) return rc;
  timer.mark(2);
  if (n_tracks > 0) hipLaunchKernelGGL(k_covis_count, blocks_for(n_tracks * 16, LOC_THREADS), dim3(LOC_THREADS), 0, st, a);
  timer.mark(3);
  if (topk)
    hipLaunchKernelGGL(k_covis_topk, dim3((unsigned)n_images), dim3(LOC_THREADS), 0, st, n_images, (const int32_t*)d_count, num_matched,
                       d_topk_index, d_topk_count, d_n_topk);
  timer.mark(4);
  rc = hip_check(hipGetLastError(), "k_covis_topk launch");
  if (rc == PXR_OK) rc = hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
  if (rc != PXR_OK) return rc;
  const int from[3] = {0, 2, 3};
  return timer.read(from, 3);
}

// ---- covisibility clusters -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LOC_THREADS) void k_cluster_check(int32_t n_images, int64_t n_ret, const int32_t* __restrict__ ret,
                                                               int* __restrict__ flag) {
  const int64_t r = (int64_t)blockIdx.x * LOC_THREADS + threadIdx.x;
  if (r >= n_ret) return;
  if (ret[r] < 0 || ret[r] >= n_images) atomicOr(flag, 1);
}

// One wavefront: n <= 64 is uniform, the loops over s < n and the ballots are executed by all 64 lanes (a lane without an entry
// carries an empty mask and is nobody's neighbour).
__global__ __launch_bounds__(64) void k_cluster(int32_t n_images, const int32_t* __restrict__ count, const int64_t* __restrict__ ret_offsets,
                                                const int32_t* __restrict__ ret, int32_t* __restrict__ cluster,
                                                int32_t* __restrict__ n_clusters) {
  const int64_t q = blockIdx.x, r0 = ret_offsets[q];
  const int n = (int)(ret_offsets[q + 1] - r0), lane = threadIdx.x;
  if (n == 0) {
    if (lane == 0) n_clusters[q] = 0;
    return;
  }
  const bool live = lane < n;
  unsigned long long mask = 0;
  if (live) {
    const int32_t mine = ret[r0 + lane];
    const int32_t* row = count + (int64_t)mine * n_images;
    for (int s = 0; s < n; ++s) {
      const int32_t other = ret[r0 + s];
      if (other == mine || row[other] > 0) mask |= (unsigned long long)1 << s;
    }
  }
  // closure: a lane takes over the masks of everyone it reaches, until no lane of the wavefront learns anything
  for (;;) {
    unsigned long long next = mask;
    for (int s = 0; s < n; ++s) {
      const unsigned long long theirs = __shfl(mask, s, 64);
      if ((mask >> s) & 1) next |= theirs;
    }
    const int changed = next != mask;
    mask = next;
    if (!__ballot(changed)) break;
  }
  const int id = live ? __builtin_ctzll(mask) : 64, size = __builtin_popcountll(mask);
  const unsigned long long leaders = __ballot(live && id == lane);
  int rank = 0;                                              // components that come before this lane's: larger, or as large and found earlier
  for (int s = 0; s < n; ++s) {
    const int theirs = __shfl(size, s, 64);
    if (((leaders >> s) & 1) && (theirs > size || (theirs == size && s < id))) ++rank;
  }
  if (live) cluster[r0 + lane] = rank;
  if (lane == 0) n_clusters[q] = __builtin_popcountll(leaders);
}

static int covisibility_clusters(pxr_ctx* ctx, int32_t n_images, const int32_t* d_count, int32_t n_queries, const int64_t* d_ret_offsets,
                                 int64_t n_ret, const int32_t* d_ret, int32_t* d_cluster, int32_t* d_n_clusters, double* h_ms) {
  const char* fn = "pxr_covisibility_clusters";
  PXR_REQUIRE(ctx, "%s: NULL context", fn);
  PXR_REQUIRE(n_images >= 0 && n_queries >= 0 && n_ret >= 0, "%s: negative size", fn);
  PXR_REQUIRE(n_images <= PXR_MAX_COVIS_IMAGES, "%s: %d images, more than PXR_MAX_COVIS_IMAGES = %d", fn, (int)n_images,
              (int)PXR_MAX_COVIS_IMAGES);
  PXR_REQUIRE(d_ret_offsets, "%s: NULL ret_offsets", fn);
  PXR_REQUIRE(n_queries == 0 || d_n_clusters, "%s: NULL n_clusters", fn);
  PXR_REQUIRE(n_ret == 0 || (d_ret && d_cluster && d_count), "%s: NULL retrieval array", fn);
  if (h_ms) h_ms[0] = h_ms[1] = 0.0;
  PXR_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;

  std::vector<int64_t> off;
  std::vector<int32_t> order;
  auto short_enough = [&](int64_t q) {
    PXR_REQUIRE(off[q + 1] - off[q] <= LOC_MAX_LIST, "%s: query %lld has %lld retrieved images, more than %d", fn, (long long)q,
                (long long)(off[q + 1] - off[q]), LOC_MAX_LIST);
    return (int)PXR_OK;
  };
  if (int rc = batch_order(ctx, {fn, "ret_offsets", "query", "n_ret"}, false, d_ret_offsets, n_queries, n_ret, off, order, short_enough)) return rc;
  if (n_queries == 0) return PXR_OK;

  int* flag;
  Workspace ws;
  ws.take(flag, 4);
  if (int rc = ws.commit(ctx)) return rc;
  StageTimer<4> timer(st, h_ms);                         // check | (the flag's read-back) | clusters
  if (int rc = timer.create(fn)) return rc;
  int h_flag = 0;
  int rc = hip_check(hipMemsetAsync(flag, 0, 16, st), "hipMemsetAsync");
  if (rc == PXR_OK) {
    timer.mark(0);
    if (n_ret > 0) hipLaunchKernelGGL(k_cluster_check, blocks_for(n_ret, LOC_THREADS), dim3(LOC_THREADS), 0, st, n_images, n_ret, d_ret, flag);
    timer.mark(1);
    rc = hip_check(hipMemcpyAsync(&h_flag, flag, 4, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
  }
  if (rc == PXR_OK) rc = hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
  if (rc != PXR_OK) return rc;
  if (h_flag) return set_error(PXR_EINVAL, "%s: a retrieved image index is outside [0, n_images = %d)", fn, (int)n_images);

  timer.mark(2);
  hipLaunchKernelGGL(k_cluster, dim3((unsigned)n_queries), dim3(64), 0, st, n_images, d_count, d_ret_offsets, d_ret, d_cluster, d_n_clusters);
  timer.mark(3);
  rc = hip_check(hipGetLastError(), "k_cluster launch");
  if (rc == PXR_OK) rc = hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
  if (rc != PXR_OK) return rc;
  const int from[2] = {0, 2};
  return timer.read(from, 2);
}

// ---- 2D-3D pairs ---------------------------------------------------------------------------------------------------------------
struct LocArgs {
  int32_t n_problems;
  const int64_t* problem_offsets;   // [n_problems + 1]
  const int32_t* problem_pair;      // [n_entries]
  const int32_t* pairs;             // [n_pairs][2]
  const int64_t* pair_offsets;      // [n_pairs + 1]
  const int32_t* matches0;          // [n_rows]
  const int64_t* image_offsets;     // [n_set_images + 1]
  const double* kp_xy;              // [n_total][2]
  const int64_t* kp_point;          // [n_total]
  int64_t n_points;
  const double* xyz;                // [n_points][3]
  const int64_t* lane_first;        // [n_problems + 1] workspace: problem p owns lanes [lane_first[p], lane_first[p + 1]), one per query keypoint
  int64_t n_lanes;
  int32_t* lane_count;              // [n_lanes] workspace: the pairs every lane emits
  long long* block_count;           // [n_blocks] workspace: their sums over the workgroups of k_loc_walk
  long long* block_start;           // [n_blocks + 1] workspace: the exclusive scan of block_count, and the total
  int64_t* lane_start;              // [n_lanes] workspace: where every lane writes (filled by the write pass)
  int64_t* corr_offsets; int32_t* corr_kp; int64_t* corr_point; double* corr_xy; double* corr_xyz;
};

// the point that entry e gives query keypoint k, -1 for none; *bad collects 1: a match beyond the database image's keypoints,
// 2: a point beyond n_points (such an entry gives no point, so nothing is read out of range)
__device__ __forceinline__ int64_t loc_point(const LocArgs& a, int64_t e, int64_t k, int* bad) {
  const int32_t pr = a.problem_pair[e];
  const int32_t m = a.matches0[a.pair_offsets[pr] + k];
  if (m < 0) return -1;
  const int32_t db = a.pairs[2 * pr + 1];
  const int64_t base = a.image_offsets[db];
  if (m >= a.image_offsets[db + 1] - base) { *bad |= 1; return -1; }
  const int64_t pid = a.kp_point[base + m];
  if (pid >= a.n_points) { *bad |= 2; return -1; }
  return pid < 0 ? -1 : pid;
}

// The walk of one query keypoint over the entries of its problem, in order: a point is emitted where it is finite and no earlier
// entry gave it (the earlier entries are read again: no per-lane table).  *n: the pairs emitted, written from row `at` on.
template <bool WRITE>
__device__ __forceinline__ void loc_walk_lane(const LocArgs& a, int64_t lane, int64_t at, int* n_out, int* bad_out) {
  int32_t lo = 0, hi = a.n_problems;                      // the last p with lane_first[p] <= lane (problems without lanes are skipped)
  while (hi - lo > 1) {
    const int32_t mid = lo + (hi - lo) / 2;
    if (a.lane_first[mid] <= lane) lo = mid; else hi = mid;
  }
  const int32_t p = lo;
  const int64_t k = lane - a.lane_first[p], e0 = a.problem_offsets[p], e1 = a.problem_offsets[p + 1];
  const int32_t query = a.pairs[2 * a.problem_pair[e0]];
  const int64_t kp = a.image_offsets[query] + k;
  const double x = a.kp_xy[2 * kp], y = a.kp_xy[2 * kp + 1];
  int bad = 0, n = 0;
  if (isfinite(x) && isfinite(y))
    for (int64_t e = e0; e < e1; ++e) {
      const int64_t pid = loc_point(a, e, k, &bad);
      if (pid < 0) continue;
      const double X = a.xyz[3 * pid], Y = a.xyz[3 * pid + 1], Z = a.xyz[3 * pid + 2];
      if (!(isfinite(X) && isfinite(Y) && isfinite(Z))) continue;
      bool seen = false;
      for (int64_t f = e0; f < e && !seen; ++f) seen = loc_point(a, f, k, &bad) == pid;
      if (seen) continue;
      if (WRITE) {
        const int64_t j = at + n;
        a.corr_kp[j] = (int32_t)k; a.corr_point[j] = pid;
        a.corr_xy[2 * j] = x; a.corr_xy[2 * j + 1] = y;
        a.corr_xyz[3 * j] = X; a.corr_xyz[3 * j + 1] = Y; a.corr_xyz[3 * j + 2] = Z;
      }
      ++n;
    }
  *n_out = n; *bad_out = bad;
}

// Where a lane writes: the workgroup's start (the scan of the workgroups' totals) plus the prefix of the counts inside the
// workgroup.  Every thread of the workgroup reaches the block sum / block scan; a thread past the last lane brings a count of 0.
template <bool WRITE>
__global__ __launch_bounds__(LOC_THREADS) void k_loc_walk(const LocArgs a, int* __restrict__ flag) {
  __shared__ long long s_part[LOC_WAVES];
  const int64_t lane = (int64_t)blockIdx.x * LOC_THREADS + threadIdx.x;
  const bool live = lane < a.n_lanes;
  int bad = 0, n = 0;
  int64_t at = 0;
  if (WRITE) {
    long long total;
    at = a.block_start[blockIdx.x] + block_exclusive_scan<LOC_THREADS>((long long)(live ? a.lane_count[lane] : 0), s_part, total);
    if (live) a.lane_start[lane] = at;
  }
  if (live) loc_walk_lane<WRITE>(a, lane, at, &n, &bad);
  if (!WRITE) {
    if (live) a.lane_count[lane] = n;
    const long long sum = block_int_sum<LOC_THREADS>((long long)n, s_part);
    if (threadIdx.x == 0) a.block_count[blockIdx.x] = sum;
    if (bad) atomicOr(flag, bad);
  }
}

__global__ __launch_bounds__(LOC_THREADS) void k_loc_offsets(const LocArgs a) {
  const int64_t p = (int64_t)blockIdx.x * LOC_THREADS + threadIdx.x;
  if (p > a.n_problems) return;
  const int64_t first = a.lane_first[p];
  a.corr_offsets[p] = first < a.n_lanes ? a.lane_start[first] : a.block_start[(a.n_lanes + LOC_THREADS - 1) / LOC_THREADS];
}

static int localization_pairs(pxr_ctx* ctx, int32_t n_problems, const int64_t* d_problem_offsets, int64_t n_entries,
                              const int32_t* d_problem_pair, int32_t n_pairs, const int32_t* d_pairs, const int64_t* d_pair_offsets,
                              int64_t n_rows, const int32_t* d_matches0, int32_t n_set_images, const int64_t* d_image_offsets,
                              int64_t n_total, const double* d_kp_xy, const int64_t* d_kp_point, int64_t n_points, const double* d_xyz,
                              int64_t* d_corr_offsets, int32_t* d_corr_kp, int64_t* d_corr_point, double* d_corr_xy, double* d_corr_xyz,
                              int64_t* h_n_corr, double* h_ms) {
  const char* fn = "pxr_localization_pairs";
  PXR_REQUIRE(ctx && h_n_corr, "%s: NULL argument", fn);
  PXR_REQUIRE(n_problems >= 0 && n_entries >= 0 && n_pairs >= 0 && n_rows >= 0 && n_set_images >= 0 && n_total >= 0 && n_points >= 0,
              "%s: negative size", fn);
  PXR_REQUIRE(d_problem_offsets && d_pair_offsets && d_image_offsets && d_corr_offsets, "%s: NULL offsets array", fn);
  PXR_REQUIRE(n_entries == 0 || d_problem_pair, "%s: NULL problem_pair", fn);
  PXR_REQUIRE(n_pairs == 0 || d_pairs, "%s: NULL pairs", fn);
  PXR_REQUIRE(n_rows == 0 || (d_matches0 && d_corr_kp && d_corr_point && d_corr_xy && d_corr_xyz), "%s: NULL match or output array", fn);
  PXR_REQUIRE(n_total == 0 || (d_kp_xy && d_kp_point), "%s: NULL keypoint array", fn);
  PXR_REQUIRE(n_points == 0 || d_xyz, "%s: NULL xyz", fn);
  if (h_ms) h_ms[0] = h_ms[1] = h_ms[2] = 0.0;
  PXR_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int32_t P = n_problems;

  // the lists are small (one entry per retrieved image): they are validated on host copies, which also give every problem's lanes
  std::vector<int64_t> img_off, pair_off, prob_off;
  std::vector<int32_t> order, pairs((size_t)n_pairs * 2), entries((size_t)n_entries);
  auto none = [](int64_t) { return (int)PXR_OK; };
  if (int rc = batch_order(ctx, {fn, "image_offsets", "image", "n_total"}, false, d_image_offsets, n_set_images, n_total, img_off, order, none)) return rc;
  if (n_pairs > 0) PXR_HIP(hipMemcpyAsync(pairs.data(), d_pairs, sizeof(int32_t) * 2 * (size_t)n_pairs, hipMemcpyDeviceToHost, st));
  if (n_entries > 0) PXR_HIP(hipMemcpyAsync(entries.data(), d_problem_pair, sizeof(int32_t) * (size_t)n_entries, hipMemcpyDeviceToHost, st));
  auto pair_rows = [&](int64_t p) {
    const int32_t q = pairs[2 * (size_t)p], db = pairs[2 * (size_t)p + 1];
    PXR_REQUIRE(q >= 0 && q < n_set_images && db >= 0 && db < n_set_images, "%s: pair %lld names an image outside [0, n_set_images = %d)", fn,
                (long long)p, (int)n_set_images);
    PXR_REQUIRE(pair_off[p + 1] - pair_off[p] == img_off[q + 1] - img_off[q], "%s: pair %lld owns %lld rows of matches0, its first image has %lld keypoints",
                fn, (long long)p, (long long)(pair_off[p + 1] - pair_off[p]), (long long)(img_off[q + 1] - img_off[q]));
    return (int)PXR_OK;
  };
  if (int rc = batch_order(ctx, {fn, "pair_offsets", "pair", "n_rows"}, false, d_pair_offsets, n_pairs, n_rows, pair_off, order, pair_rows)) return rc;
  std::vector<int64_t> lane_first((size_t)P + 1, 0);
  auto one_query = [&](int64_t p) {
    const int64_t e0 = prob_off[p], e1 = prob_off[p + 1];
    PXR_REQUIRE(e1 - e0 <= LOC_MAX_LIST, "%s: problem %lld has %lld entries, more than %d", fn, (long long)p, (long long)(e1 - e0), LOC_MAX_LIST);
    PXR_REQUIRE(e1 <= n_entries, "%s: problem_offsets passes n_entries = %lld at problem %lld", fn, (long long)n_entries, (long long)p);
    int64_t lanes = 0;
    for (int64_t e = e0; e < e1; ++e) {
      const int32_t pr = entries[(size_t)e];
      PXR_REQUIRE(pr >= 0 && pr < n_pairs, "%s: entry %lld names a pair outside [0, n_pairs = %d)", fn, (long long)e, (int)n_pairs);
      PXR_REQUIRE(pairs[2 * (size_t)pr] == pairs[2 * (size_t)entries[(size_t)e0]], "%s: the entries of problem %lld do not share their first image", fn,
                  (long long)p);
      lanes = pair_off[pr + 1] - pair_off[pr];
    }
    lane_first[(size_t)p + 1] = lane_first[(size_t)p] + lanes;
    return (int)PXR_OK;
  };
  if (int rc = batch_order(ctx, {fn, "problem_offsets", "problem", "n_entries"}, false, d_problem_offsets, P, n_entries, prob_off, order, one_query)) return rc;
  const int64_t n_lanes = lane_first[(size_t)P];
  PXR_REQUIRE(n_lanes < ((int64_t)1 << 31) * LOC_THREADS, "%s: too many (problem, keypoint) lanes", fn);

  if (n_lanes == 0) {
    PXR_HIP(hipMemsetAsync(d_corr_offsets, 0, sizeof(int64_t) * ((size_t)P + 1), st));
    *h_n_corr = 0;
    return hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
  }

  const int64_t n_blocks = (n_lanes + LOC_THREADS - 1) / LOC_THREADS;
  int* flag; int64_t* d_lane_first; int32_t* d_lane_count; int64_t* d_lane_start; long long* d_block_count; long long* d_block_start;
  Workspace ws;
  ws.take(flag, 4); ws.take(d_lane_first, (size_t)P + 1); ws.take(d_lane_count, (size_t)n_lanes); ws.take(d_lane_start, (size_t)n_lanes);
  ws.take(d_block_count, (size_t)n_blocks); ws.take(d_block_start, (size_t)n_blocks + 1);
  if (int rc = ws.commit(ctx)) return rc;
  LocArgs a;
  a.n_problems = P; a.problem_offsets = d_problem_offsets; a.problem_pair = d_problem_pair; a.pairs = d_pairs; a.pair_offsets = d_pair_offsets;
  a.matches0 = d_matches0; a.image_offsets = d_image_offsets; a.kp_xy = d_kp_xy; a.kp_point = d_kp_point; a.n_points = n_points; a.xyz = d_xyz;
  a.lane_first = d_lane_first; a.n_lanes = n_lanes; a.lane_count = d_lane_count; a.lane_start = d_lane_start;
  a.block_count = d_block_count; a.block_start = d_block_start;
  a.corr_offsets = d_corr_offsets; a.corr_kp = d_corr_kp; a.corr_point = d_corr_point; a.corr_xy = d_corr_xy; a.corr_xyz = d_corr_xyz;

  StageTimer<5> timer(st, h_ms);                         // count | (the flag's read-back) | scan | write
  if (int rc = timer.create(fn)) return rc;
  int h_flag = 0;
  int rc = hip_check(hipMemsetAsync(flag, 0, 16, st), "hipMemsetAsync");
  if (rc == PXR_OK) rc = hip_check(hipMemcpyAsync(d_lane_first, lane_first.data(), sizeof(int64_t) * ((size_t)P + 1), hipMemcpyHostToDevice, st), "hipMemcpyAsync");
  if (rc == PXR_OK) {
    timer.mark(0);
    hipLaunchKernelGGL(k_loc_walk<false>, blocks_for(n_lanes, LOC_THREADS), dim3(LOC_THREADS), 0, st, a, flag);
    timer.mark(1);
    rc = hip_check(hipMemcpyAsync(&h_flag, flag, 4, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
  }
  if (rc == PXR_OK) rc = hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");      // (also: `lane_first` may go out of scope)
  if (rc != PXR_OK) return rc;
  if (h_flag & 1) return set_error(PXR_EINVAL, "%s: matches0 names a keypoint beyond those of the pair's second image", fn);
  if (h_flag) return set_error(PXR_EINVAL, "%s: kp_point names a point outside [0, n_points = %lld)", fn, (long long)n_points);

  timer.mark(2);
  hipLaunchKernelGGL((k_exclusive_scan<LOC_THREADS, long long, long long>), dim3(1), dim3(LOC_THREADS), 0, st, n_blocks,
                     (const long long*)d_block_count, d_block_start, 1);
  timer.mark(3);
  hipLaunchKernelGGL(k_loc_walk<true>, blocks_for(n_lanes, LOC_THREADS), dim3(LOC_THREADS), 0, st, a, flag);
  hipLaunchKernelGGL(k_loc_offsets, blocks_for((int64_t)P + 1, LOC_THREADS), dim3(LOC_THREADS), 0, st, a);
  timer.mark(4);
  rc = hip_check(hipGetLastError(), "k_loc_walk launch");
  long long total = 0;
  if (rc == PXR_OK) rc = hip_check(hipMemcpyAsync(&total, d_block_start + n_blocks, sizeof(long long), hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
  if (rc == PXR_OK) rc = hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
  if (rc != PXR_OK) return rc;
  *h_n_corr = total;
  const int from[3] = {0, 2, 3};
  return timer.read(from, 3);
}

}  // namespace pxr

extern "C" int pxr_covisibility(pxr_ctx* ctx, int32_t n_images, int64_t n_tracks, const int64_t* d_track_offsets, int64_t n_obs,
                                const int32_t* d_obs_image, const uint8_t* d_track_mask, int32_t num_matched, int32_t* d_count,
                                int32_t* d_topk_index, int32_t* d_topk_count, int32_t* d_n_topk) {
  return pxr::covisibility(ctx, n_images, n_tracks, d_track_offsets, n_obs, d_obs_image, d_track_mask, num_matched, d_count, d_topk_index,
                           d_topk_count, d_n_topk, nullptr);
}

extern "C" int pxr_covisibility_timed(pxr_ctx* ctx, int32_t n_images, int64_t n_tracks, const int64_t* d_track_offsets, int64_t n_obs,
                                      const int32_t* d_obs_image, const uint8_t* d_track_mask, int32_t num_matched, int32_t* d_count,
                                      int32_t* d_topk_index, int32_t* d_topk_count, int32_t* d_n_topk, double* h_kernel_ms) {
  PXR_REQUIRE(h_kernel_ms, "pxr_covisibility_timed: NULL h_kernel_ms");
  return pxr::covisibility(ctx, n_images, n_tracks, d_track_offsets, n_obs, d_obs_image, d_track_mask, num_matched, d_count, d_topk_index,
                           d_topk_count, d_n_topk, h_kernel_ms);
}

extern "C" int pxr_covisibility_clusters(pxr_ctx* ctx, int32_t n_images, const int32_t* d_count, int32_t n_queries,
                                         const int64_t* d_ret_offsets, int64_t n_ret, const int32_t* d_ret, int32_t* d_cluster,
                                         int32_t* d_n_clusters) {
  return pxr::covisibility_clusters(ctx, n_images, d_count, n_queries, d_ret_offsets, n_ret, d_ret, d_cluster, d_n_clusters, nullptr);
}

extern "C" int pxr_covisibility_clusters_timed(pxr_ctx* ctx, int32_t n_images, const int32_t* d_count, int32_t n_queries,
                                               const int64_t* d_ret_offsets, int64_t n_ret, const int32_t* d_ret, int32_t* d_cluster,
                                               int32_t* d_n_clusters, double* h_kernel_ms) {
  PXR_REQUIRE(h_kernel_ms, "pxr_covisibility_clusters_timed: NULL h_kernel_ms");
  return pxr::covisibility_clusters(ctx, n_images, d_count, n_queries, d_ret_offsets, n_ret, d_ret, d_cluster, d_n_clusters, h_kernel_ms);
}

extern "C" int pxr_localization_pairs(pxr_ctx* ctx, int32_t n_problems, const int64_t* d_problem_offsets, int64_t n_entries,
                                      const int32_t* d_problem_pair, int32_t n_pairs, const int32_t* d_pairs, const int64_t* d_pair_offsets,
                                      int64_t n_rows, const int32_t* d_matches0, int32_t n_set_images, const int64_t* d_image_offsets,
                                      int64_t n_total, const double* d_kp_xy, const int64_t* d_kp_point, int64_t n_points,
                                      const double* d_xyz, int64_t* d_corr_offsets, int32_t* d_corr_kp, int64_t* d_corr_point,
                                      double* d_corr_xy, double* d_corr_xyz, int64_t* h_n_corr) {
  return pxr::localization_pairs(ctx, n_problems, d_problem_offsets, n_entries, d_problem_pair, n_pairs, d_pairs, d_pair_offsets, n_rows,
                                 d_matches0, n_set_images, d_image_offsets, n_total, d_kp_xy, d_kp_point, n_points, d_xyz, d_corr_offsets,
                                 d_corr_kp, d_corr_point, d_corr_xy, d_corr_xyz, h_n_corr, nullptr);
}

extern "C" int pxr_localization_pairs_timed(pxr_ctx* ctx, int32_t n_problems, const int64_t* d_problem_offsets, int64_t n_entries,
                                            const int32_t* d_problem_pair, int32_t n_pairs, const int32_t* d_pairs,
                                            const int64_t* d_pair_offsets, int64_t n_rows, const int32_t* d_matches0, int32_t n_set_images,
                                            const int64_t* d_image_offsets, int64_t n_total, const double* d_kp_xy, const int64_t* d_kp_point,
                                            int64_t n_points, const double* d_xyz, int64_t* d_corr_offsets, int32_t* d_corr_kp,
                                            int64_t* d_corr_point, double* d_corr_xy, double* d_corr_xyz, int64_t* h_n_corr,
                                            double* h_kernel_ms) {
  PXR_REQUIRE(h_kernel_ms, "pxr_localization_pairs_timed: NULL h_kernel_ms");
  return pxr::localization_pairs(ctx, n_problems, d_problem_offsets, n_entries, d_problem_pair, n_pairs, d_pairs, d_pair_offsets, n_rows,
                                 d_matches0, n_set_images, d_image_offsets, n_total, d_kp_xy, d_kp_point, n_points, d_xyz, d_corr_offsets,
                                 d_corr_kp, d_corr_point, d_corr_xy, d_corr_xyz, h_n_corr, h_kernel_ms);
}
