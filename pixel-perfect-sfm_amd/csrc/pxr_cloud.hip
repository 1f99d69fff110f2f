// pxr_cloud.hip -- reconstruction evaluation on point clouds: the nearest reference point within max_dist of every query point
// (pxr_cloud_nearest) and the voxel-averaged fractions of points within each tolerance (pxr_cloud_voxel_fractions); the
// specification is in include/pixsfm_hip.h and DESIGN.md section 28.  Both results are functions of their input arrays alone:
// the minimum with an index tie-break and the integer sums do not depend on the order the tables below are filled or walked in.
//
// pxr_cloud_nearest: a uniform grid over the reference cloud, kept as a HASHED table of buckets (a power of two >= 2 n_ref of
// them: a 50 m scene at a 5 cm cell is 10^9 cells, a dense grid is out of the question).
//   k_cloud_count    one lane per reference point: its cell, the cell's bucket, one integer atomic on the bucket's count.
//   k_scan_reduce, k_exclusive_scan (pxr_scan.h), k_scan_apply   the exclusive prefix sums of the counts, in place (chunks of
//                    SCAN_CHUNK buckets, one workgroup over the chunks' totals, the chunks again).
//   k_cloud_fill     one lane per reference point: a slot from the bucket's cursor (integer atomic), the point and its index copied
//                    there -- a bucket's points are contiguous for the query.  The cursors end as the buckets' ends: one array
//                    serves count, offset and end.
//   k_cloud_query    one lane per query point: the buckets of the 27 cells around its own, every point in them tested with the
//                    exact d2 of the specification.  Two cells in one bucket cost tests, not correctness (what is tested is d2, not
//                    the cell); a bucket met twice changes nothing.
//
// COVERAGE (why 27 cells are enough, rounding included).  Write u = 2^-53, m = max_dist, m2 = fl(m m).  For a candidate pair
// d2 <= m2, and d2 is a rounded sum of non-negative rounded terms, so fl(dx dx) <= d2 <= m2 for dx = fl(qx - rx) (rounding is
// monotone and fl(a + b) >= a for b >= 0); the same for y and z.
//   (1) m2 finite.  Either dx dx is in the normal range, and dx^2 (1 - u) <= m^2 (1 + u), |dx| <= m (1 + 2u); or it is not, and
//       |dx| < 2^-510.  A finite dx has |qx - rx| <= |dx| / (1 - u) (a difference that lands among the subnormals is exact).  So
//       |qx - rx| <= M (1 + 4u) with M = max(m, 2^-400).
//   (2) The cell side is h = fl(M (1 + 2^-20)) >= M (1 + 2^-20)(1 - u), so |qx - rx| / h <= 1 - 2^-21.
//   (3) The cell coordinate is c(x) = clamp(floor(fl(x / h)), -2^30, 2^30): monotone in x.  For rx <= qx with |c(rx)| < 2^30:
//       fl(qx / h) - fl(rx / h) <= (qx - rx) / h + u (|qx / h| + |rx / h|) + 2^-1074 <= 1 - 2^-21 + u (2^31 + 2) < 1, hence
//       c(qx) <= c(rx) + 1.  Where a coordinate is clamped, every point beyond the clamp shares the last cell, and the same
//       inequality holds for a pair that straddles it.  So |c(qx) - c(rx)| <= 1 on every axis: r lies in one of the 27 cells.
//   (4) m2 not finite (max_dist above about 1.3e154): every valid pair is a candidate, h is taken as +inf, every x / h is 0, all
//       points share cell 0 and the query is the brute-force search.
// The margin 2^-20 widens a cell by a millionth: it costs nothing and leaves the argument far from any rounding.
//
// pxr_cloud_voxel_fractions: an open-addressing table (a power of two >= 2 n slots) keyed by the packed voxel.
//   k_voxel_insert   one lane per point: floor(x / v) per axis in float64, the range check (a flag, read after the launch), the 63-bit
//                    key, a 64-bit compare-and-swap insert with linear probing, integer adds on the slot's counts.
//   k_voxel_reduce   every occupied slot: q_v[t] = llrint(((double)w / (double)n) 2^32), summed as 64-bit integers (a butterfly per
//                    wavefront, one integer atomic per wavefront and tolerance).
//   k_voxel_plain    voxel_size = 0, every valid point its own voxel: q is 2^32 or 0, no table.
#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>
#include <vector>

#include "pxr_batch.h"
#include "pxr_internal.h"
#include "pxr_scan.h"

namespace pxr {
namespace {

constexpr int CL_THREADS = 256;
constexpr int SCAN_PER_LANE = 16;
constexpr int SCAN_CHUNK = CL_THREADS * SCAN_PER_LANE;   // buckets of one scan workgroup
constexpr int32_t CELL_CLAMP = 1 << 30;
constexpr unsigned long long VOXEL_EMPTY = ~0ull;
constexpr int RES_NVOX = PXR_CLOUD_MAX_TOLERANCES, RES_BAD = PXR_CLOUD_MAX_TOLERANCES + 1, RES_WORDS = PXR_CLOUD_MAX_TOLERANCES + 2;

__device__ __forceinline__ bool finite3(double x, double y, double z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// (3) of the coverage argument; h > 0 or +inf
__device__ __forceinline__ int32_t cell_of(double x, double h) {
  const double c = floor(x / h);
  return (int32_t)fmin(fmax(c, -(double)CELL_CLAMP), (double)CELL_CLAMP);
}

__device__ __forceinline__ unsigned long long mix64(unsigned long long k) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
  return k;
}

__device__ __forceinline__ unsigned long long bucket_of(int32_t cx, int32_t cy, int32_t cz, unsigned long long mask) {
  const unsigned long long k = (unsigned long long)(uint32_t)cx * 0x9e3779b97f4a7c15ull + (unsigned long long)(uint32_t)cy * 0xc2b2ae3d27d4eb4full +
                               (unsigned long long)(uint32_t)cz * 0x165667b19e3779f9ull;
  return mix64(k) & mask;
}

struct GridArgs {
  const double* ref;          // [n_ref][3]
  int64_t n_ref;
  double h;                   // cell side
  unsigned long long mask;    // buckets - 1
  uint32_t* bucket;           // [buckets]: count, then offset, then end
  double* sorted_xyz;         // [n_ref][3] in bucket order (the valid points)
  int32_t* sorted_idx;        // [n_ref]
};

template <bool FILL>
__global__ __launch_bounds__(CL_THREADS) void k_cloud_grid(const GridArgs a) {
  const int64_t i = (int64_t)blockIdx.x * CL_THREADS + threadIdx.x;
  if (i >= a.n_ref) return;
  const double x = a.ref[3 * i], y = a.ref[3 * i + 1], z = a.ref[3 * i + 2];
  if (!finite3(x, y, z)) return;
  const unsigned long long b = bucket_of(cell_of(x, a.h), cell_of(y, a.h), cell_of(z, a.h), a.mask);
  const uint32_t slot = atomicAdd(&a.bucket[b], 1u);
  if (FILL) {                                            // slot < the number of valid points <= n_ref: the cursors start at the offsets
    a.sorted_xyz[3 * (int64_t)slot] = x; a.sorted_xyz[3 * (int64_t)slot + 1] = y; a.sorted_xyz[3 * (int64_t)slot + 2] = z;
    a.sorted_idx[slot] = (int32_t)i;
  }
}

// ---- exclusive prefix sums over the buckets, in place ------------------------------------------------------------------------------
// the chunks' totals; k_exclusive_scan in one workgroup turns them into the sums before each chunk; the chunks again
__global__ __launch_bounds__(CL_THREADS) void k_scan_reduce(const uint32_t* v, int64_t n, uint32_t* partial) {
  __shared__ uint32_t s_part[CL_THREADS / 64];
  const int64_t first = (int64_t)blockIdx.x * SCAN_CHUNK + (int64_t)threadIdx.x * SCAN_PER_LANE;
  uint32_t s = 0;
  for (int k = 0; k < SCAN_PER_LANE; ++k) if (first + k < n) s += v[first + k];
  const uint32_t total = block_int_sum<CL_THREADS>(s, s_part);
  if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

__global__ __launch_bounds__(CL_THREADS) void k_scan_apply(uint32_t* v, int64_t n, const uint32_t* partial) {
  __shared__ uint32_t s_part[CL_THREADS / 64];
  const int64_t first = (int64_t)blockIdx.x * SCAN_CHUNK + (int64_t)threadIdx.x * SCAN_PER_LANE;
  uint32_t c[SCAN_PER_LANE], s = 0;
#pragma unroll
  for (int k = 0; k < SCAN_PER_LANE; ++k) { c[k] = first + k < n ? v[first + k] : 0u; s += c[k]; }
  uint32_t total;
  uint32_t run = partial[blockIdx.x] + block_exclusive_scan<CL_THREADS>(s, s_part, total);
#pragma unroll
  for (int k = 0; k < SCAN_PER_LANE; ++k) { if (first + k < n) v[first + k] = run; run += c[k]; }
}

// ---- the query ----------------------------------------------------------------------------------------------------------------------
struct QueryArgs {
  const double* query;        // [n_query][3]
  int64_t n_query, n_ref;
  double h, m2;
  unsigned long long mask;
  const uint32_t* bucket_end; // [buckets]: bucket b owns the sorted slots [bucket_end[b - 1] (0 for b = 0), bucket_end[b])
  const double* sorted_xyz;
  const int32_t* sorted_idx;
  int32_t* nn_index;
  double* nn_dist2;
};

__global__ __launch_bounds__(CL_THREADS) void k_cloud_query(const QueryArgs a) {
  const int64_t i = (int64_t)blockIdx.x * CL_THREADS + threadIdx.x;
  if (i >= a.n_query) return;
  const double qx = a.query[3 * i], qy = a.query[3 * i + 1], qz = a.query[3 * i + 2];
  int32_t best = -1;
  double bd = INFINITY;
  if (a.n_ref > 0 && finite3(qx, qy, qz)) {
    const int32_t cx = cell_of(qx, a.h), cy = cell_of(qy, a.h), cz = cell_of(qz, a.h);
    for (int n = 0; n < 27; ++n) {
      const unsigned long long b = bucket_of(cx + n % 3 - 1, cy + (n / 3) % 3 - 1, cz + n / 9 - 1, a.mask);
      const uint32_t p0 = b ? a.bucket_end[b - 1] : 0u, p1 = a.bucket_end[b];
      for (uint32_t p = p0; p < p1; ++p) {
        const double dx = qx - a.sorted_xyz[3 * (int64_t)p], dy = qy - a.sorted_xyz[3 * (int64_t)p + 1], dz = qz - a.sorted_xyz[3 * (int64_t)p + 2];
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 <= a.m2) {
          const int32_t r = a.sorted_idx[p];
          if (best < 0 || d2 < bd || (d2 == bd && r < best)) { bd = d2; best = r; }
        }
      }
    }
  }
  a.nn_index[i] = best;
  a.nn_dist2[i] = bd;
}

// ---- voxels -------------------------------------------------------------------------------------------------------------------------
struct VoxelArgs {
  const double* xyz; const double* dist2;
  int64_t n;
  double v;                   // voxel side
  int32_t n_tol;
  double tt[PXR_CLOUD_MAX_TOLERANCES];    // t * t
  unsigned long long mask;    // slots - 1
  unsigned long long* keys;   // [slots], VOXEL_EMPTY where free
  uint32_t* counts;           // [slots][1 + n_tol]: n_v, w_v[t]
  unsigned long long* res;    // [RES_WORDS]: the sums of q_v[t], the number of voxels, the number of points out of range
};

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int mask = 32; mask >= 1; mask >>= 1) v += __shfl_xor(v, mask);
  return v;
}

__global__ __launch_bounds__(CL_THREADS) void k_voxel_insert(const VoxelArgs a) {
  const int64_t i = (int64_t)blockIdx.x * CL_THREADS + threadIdx.x;
  if (i >= a.n) return;
  const double x = a.xyz[3 * i], y = a.xyz[3 * i + 1], z = a.xyz[3 * i + 2];
  if (!finite3(x, y, z)) return;
  const double fx = floor(x / a.v), fy = floor(y / a.v), fz = floor(z / a.v);
  const double lim = 1048576.0;                                                    // 2^20
  if (!(fabs(fx) < lim && fabs(fy) < lim && fabs(fz) < lim)) { atomicAdd(&a.res[RES_BAD], 1ull); return; }
  const unsigned long long key = ((unsigned long long)((long long)fx + 1048576) << 42) | ((unsigned long long)((long long)fy + 1048576) << 21) |
                                 (unsigned long long)((long long)fz + 1048576);      // three fields of 21 bits: below 2^63, never VOXEL_EMPTY
  unsigned long long s = mix64(key) & a.mask;
  for (;;) {                                                                       // at most n < slots / 2 keys: a free slot is always met
    const unsigned long long was = atomicCAS(&a.keys[s], VOXEL_EMPTY, key);
    if (was == VOXEL_EMPTY || was == key) break;
    s = (s + 1) & a.mask;
  }
  uint32_t* c = a.counts + s * (unsigned long long)(1 + a.n_tol);
  atomicAdd(&c[0], 1u);
  const double d2 = a.dist2[i];
  for (int t = 0; t < a.n_tol; ++t) if (d2 <= a.tt[t]) atomicAdd(&c[1 + t], 1u);
}

__global__ __launch_bounds__(CL_THREADS) void k_voxel_reduce(const VoxelArgs a, int64_t stride) {
  unsigned long long q[PXR_CLOUD_MAX_TOLERANCES], nv = 0;
#pragma unroll
  for (int t = 0; t < PXR_CLOUD_MAX_TOLERANCES; ++t) q[t] = 0;
  for (unsigned long long s = (unsigned long long)blockIdx.x * CL_THREADS + threadIdx.x; s <= a.mask; s += (unsigned long long)stride) {
    if (a.keys[s] == VOXEL_EMPTY) continue;
    const uint32_t* c = a.counts + s * (unsigned long long)(1 + a.n_tol);
    const double n = (double)c[0];
    ++nv;
#pragma unroll
    for (int t = 0; t < PXR_CLOUD_MAX_TOLERANCES; ++t)
      if (t < a.n_tol) q[t] += (unsigned long long)llrint(((double)c[1 + t] / n) * 4294967296.0);
  }
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int t = 0; t < PXR_CLOUD_MAX_TOLERANCES; ++t) {
    if (t >= a.n_tol) continue;                                                      // the same on every lane
    const unsigned long long w = wave_sum(q[t]);
    if (lane == 0 && w) atomicAdd(&a.res[t], w);
  }
  nv = wave_sum(nv);
  if (lane == 0 && nv) atomicAdd(&a.res[RES_NVOX], nv);
}

__global__ __launch_bounds__(CL_THREADS) void k_voxel_plain(const VoxelArgs a, int64_t stride) {
  unsigned long long w[PXR_CLOUD_MAX_TOLERANCES], nv = 0;
#pragma unroll
  for (int t = 0; t < PXR_CLOUD_MAX_TOLERANCES; ++t) w[t] = 0;
  for (int64_t i = (int64_t)blockIdx.x * CL_THREADS + threadIdx.x; i < a.n; i += stride) {
    if (!finite3(a.xyz[3 * i], a.xyz[3 * i + 1], a.xyz[3 * i + 2])) continue;
    const double d2 = a.dist2[i];
    ++nv;
#pragma unroll
    for (int t = 0; t < PXR_CLOUD_MAX_TOLERANCES; ++t)
      if (t < a.n_tol && d2 <= a.tt[t]) ++w[t];
  }
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int t = 0; t < PXR_CLOUD_MAX_TOLERANCES; ++t) {
    if (t >= a.n_tol) continue;
    const unsigned long long s = wave_sum(w[t]);
    if (lane == 0 && s) atomicAdd(&a.res[t], s << 32);                             // q = llrint((1 / 1) 2^32) per point within
  }
  nv = wave_sum(nv);
  if (lane == 0 && nv) atomicAdd(&a.res[RES_NVOX], nv);
}

// ---- host drivers -------------------------------------------------------------------------------------------------------------------
unsigned long long table_size(int64_t n) {
  unsigned long long s = 1024;
  while (s < 2ull * (unsigned long long)n) s <<= 1;
  return s;
}

int cloud_nearest(pxr_ctx* ctx, int64_t n_ref, const double* d_ref, int64_t n_query, const double* d_query, double max_dist,
                  int32_t* d_nn_index, double* d_nn_dist2, double* h_ms) {
  const char* fn = "pxr_cloud_nearest";
  PXR_REQUIRE(ctx, "%s: NULL argument", fn);
  const int64_t lim = (int64_t)1 << 31;
  PXR_REQUIRE(n_ref >= 0 && n_ref < lim, "%s: n_ref = %lld is outside [0, 2^31)", fn, (long long)n_ref);
  PXR_REQUIRE(n_query >= 0 && n_query < lim, "%s: n_query = %lld is outside [0, 2^31)", fn, (long long)n_query);
  PXR_REQUIRE(std::isfinite(max_dist) && max_dist > 0.0, "%s: max_dist = %g is not finite and positive", fn, max_dist);
  PXR_REQUIRE(n_ref == 0 || d_ref, "%s: NULL d_ref_xyz", fn);
  PXR_REQUIRE(n_query == 0 || (d_query && d_nn_index && d_nn_dist2), "%s: NULL d_query_xyz / d_nn_index / d_nn_dist2", fn);
  if (h_ms) h_ms[0] = h_ms[1] = 0.0;
  if (n_query == 0) return PXR_OK;
  PXR_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;

  const double m2 = max_dist * max_dist;
  // (1), (2) and (4) of the coverage argument at the head of this file
  const double h = std::isfinite(m2) ? std::max(max_dist, 0x1p-400) * (1.0 + 0x1p-20) : std::numeric_limits<double>::infinity();
  const unsigned long long buckets = table_size(n_ref);
  const int64_t n_chunks = (int64_t)((buckets + SCAN_CHUNK - 1) / SCAN_CHUNK);
  GridArgs g;
  g.ref = d_ref; g.n_ref = n_ref; g.h = h; g.mask = buckets - 1;
  uint32_t* partial;
  Workspace ws;
  ws.take(g.bucket, (size_t)buckets); ws.take(partial, (size_t)n_chunks); ws.take(g.sorted_xyz, (size_t)n_ref * 3); ws.take(g.sorted_idx, (size_t)n_ref);
  if (int rc = ws.commit(ctx)) return rc;

  StageTimer<3> timer(st, h_ms);                                     // grid | query
  if (int rc = timer.create(fn)) return rc;
  timer.mark(0);
  if (n_ref > 0) {
    PXR_HIP(hipMemsetAsync(g.bucket, 0, sizeof(uint32_t) * (size_t)buckets, st));
    hipLaunchKernelGGL(k_cloud_grid<false>, blocks_for(n_ref, CL_THREADS), dim3(CL_THREADS), 0, st, g);
    hipLaunchKernelGGL(k_scan_reduce, dim3((unsigned)n_chunks), dim3(CL_THREADS), 0, st, (const uint32_t*)g.bucket, (int64_t)buckets, partial);
    hipLaunchKernelGGL((k_exclusive_scan<CL_THREADS, uint32_t, uint32_t>), dim3(1), dim3(CL_THREADS), 0, st, n_chunks, (const uint32_t*)partial, partial, 0);
    hipLaunchKernelGGL(k_scan_apply, dim3((unsigned)n_chunks), dim3(CL_THREADS), 0, st, g.bucket, (int64_t)buckets, (const uint32_t*)partial);
    hipLaunchKernelGGL(k_cloud_grid<true>, blocks_for(n_ref, CL_THREADS), dim3(CL_THREADS), 0, st, g);
  }
  timer.mark(1);
  QueryArgs q;
  q.query = d_query; q.n_query = n_query; q.n_ref = n_ref; q.h = h; q.m2 = m2; q.mask = g.mask; q.bucket_end = g.bucket;
  q.sorted_xyz = g.sorted_xyz; q.sorted_idx = g.sorted_idx; q.nn_index = d_nn_index; q.nn_dist2 = d_nn_dist2;
  hipLaunchKernelGGL(k_cloud_query, blocks_for(n_query, CL_THREADS), dim3(CL_THREADS), 0, st, q);
  timer.mark(2);
  const int rc = hip_check(hipGetLastError(), "k_cloud_query launch");
  const int from[2] = {0, 1};
  return rc == PXR_OK ? timer.read(from, 2) : rc;
}

int cloud_voxel_fractions(pxr_ctx* ctx, int64_t n, const double* d_xyz, const double* d_dist2, double voxel_size, int32_t n_tol,
                          const double* h_tol, double* h_fraction, int64_t* h_n_voxels, double* h_ms) {
  const char* fn = "pxr_cloud_voxel_fractions";
  PXR_REQUIRE(ctx && h_tol && h_fraction && h_n_voxels, "%s: NULL argument", fn);
  PXR_REQUIRE(n >= 0 && n < ((int64_t)1 << 30), "%s: n = %lld is outside [0, 2^30)", fn, (long long)n);
  PXR_REQUIRE(n_tol >= 1 && n_tol <= PXR_CLOUD_MAX_TOLERANCES, "%s: n_tol = %d is outside [1, %d]", fn, (int)n_tol, PXR_CLOUD_MAX_TOLERANCES);
  for (int32_t t = 0; t < n_tol; ++t)
    PXR_REQUIRE(std::isfinite(h_tol[t]) && h_tol[t] > 0.0, "%s: tolerance %d = %g is not finite and positive", fn, (int)t, h_tol[t]);
  PXR_REQUIRE(std::isfinite(voxel_size) && voxel_size >= 0.0, "%s: voxel_size = %g is not finite and non-negative", fn, voxel_size);
  PXR_REQUIRE(n == 0 || (d_xyz && d_dist2), "%s: NULL d_xyz / d_dist2", fn);
  if (h_ms) h_ms[0] = h_ms[1] = 0.0;
  PXR_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;

  const bool table = voxel_size > 0.0 && n > 0;
  const unsigned long long slots = table ? table_size(n) : 0;
  VoxelArgs a;
  a.xyz = d_xyz; a.dist2 = d_dist2; a.n = n; a.v = voxel_size; a.n_tol = n_tol; a.mask = slots - 1;
  for (int t = 0; t < PXR_CLOUD_MAX_TOLERANCES; ++t) a.tt[t] = t < n_tol ? h_tol[t] * h_tol[t] : 0.0;
  Workspace ws;
  ws.take(a.res, RES_WORDS); ws.take(a.keys, (size_t)slots); ws.take(a.counts, (size_t)slots * (1 + n_tol));
  if (int rc = ws.commit(ctx)) return rc;

  StageTimer<3> timer(st, h_ms);                                     // insert | reduce
  if (int rc = timer.create(fn)) return rc;
  PXR_HIP(hipMemsetAsync(a.res, 0, sizeof(unsigned long long) * RES_WORDS, st));
  timer.mark(0);
  if (table) {
    PXR_HIP(hipMemsetAsync(a.keys, 0xff, sizeof(unsigned long long) * (size_t)slots, st));
    PXR_HIP(hipMemsetAsync(a.counts, 0, sizeof(uint32_t) * (size_t)slots * (1 + n_tol), st));
    hipLaunchKernelGGL(k_voxel_insert, blocks_for(n, CL_THREADS), dim3(CL_THREADS), 0, st, a);
  }
  timer.mark(1);
  if (n > 0) {
    const int64_t items = table ? (int64_t)slots : n;
    const unsigned grid = (unsigned)std::min<int64_t>(blocks_for(items, CL_THREADS).x, (int64_t)std::max(ctx->num_cus, 1) * 8);
    const int64_t stride = (int64_t)grid * CL_THREADS;
    if (table) hipLaunchKernelGGL(k_voxel_reduce, dim3(grid), dim3(CL_THREADS), 0, st, a, stride);
    else hipLaunchKernelGGL(k_voxel_plain, dim3(grid), dim3(CL_THREADS), 0, st, a, stride);
  }
  timer.mark(2);
  PXR_HIP(hipGetLastError());
  unsigned long long res[RES_WORDS];
  PXR_HIP(hipMemcpyAsync(res, a.res, sizeof res, hipMemcpyDeviceToHost, st));
  PXR_HIP(hipStreamSynchronize(st));
  const int from[2] = {0, 1};
  if (int rc = timer.read(from, 2)) return rc;
  PXR_REQUIRE(res[RES_BAD] == 0, "%s: %llu points lie 2^20 or more voxels of side %g from the origin", fn, res[RES_BAD], voxel_size);
  const int64_t n_vox = (int64_t)res[RES_NVOX];
  for (int32_t t = 0; t < n_tol; ++t)
    h_fraction[t] = n_vox > 0 ? (double)(long long)res[t] * 0x1p-32 / (double)n_vox : std::numeric_limits<double>::quiet_NaN();
  *h_n_voxels = n_vox;
  return PXR_OK;
}

}  // namespace
}  // namespace pxr

extern "C" int pxr_cloud_nearest(pxr_ctx* ctx, int64_t n_ref, const double* d_ref_xyz, int64_t n_query, const double* d_query_xyz,
                                 double max_dist, int32_t* d_nn_index, double* d_nn_dist2) {
  return pxr::cloud_nearest(ctx, n_ref, d_ref_xyz, n_query, d_query_xyz, max_dist, d_nn_index, d_nn_dist2, nullptr);
}

extern "C" int pxr_cloud_nearest_timed(pxr_ctx* ctx, int64_t n_ref, const double* d_ref_xyz, int64_t n_query, const double* d_query_xyz,
                                       double max_dist, int32_t* d_nn_index, double* d_nn_dist2, double* h_kernel_ms) {
  PXR_REQUIRE(h_kernel_ms, "pxr_cloud_nearest_timed: NULL h_kernel_ms");
  return pxr::cloud_nearest(ctx, n_ref, d_ref_xyz, n_query, d_query_xyz, max_dist, d_nn_index, d_nn_dist2, h_kernel_ms);
}

extern "C" int pxr_cloud_voxel_fractions(pxr_ctx* ctx, int64_t n, const double* d_xyz, const double* d_dist2, double voxel_size,
                                         int32_t n_tol, const double* h_tolerances, double* h_fraction, int64_t* h_n_voxels) {
  return pxr::cloud_voxel_fractions(ctx, n, d_xyz, d_dist2, voxel_size, n_tol, h_tolerances, h_fraction, h_n_voxels, nullptr);
}

extern "C" int pxr_cloud_voxel_fractions_timed(pxr_ctx* ctx, int64_t n, const double* d_xyz, const double* d_dist2, double voxel_size,
                                               int32_t n_tol, const double* h_tolerances, double* h_fraction, int64_t* h_n_voxels,
                                               double* h_kernel_ms) {
  PXR_REQUIRE(h_kernel_ms, "pxr_cloud_voxel_fractions_timed: NULL h_kernel_ms");
  return pxr::cloud_voxel_fractions(ctx, n, d_xyz, d_dist2, voxel_size, n_tol, h_tolerances, h_fraction, h_n_voxels, h_kernel_ms);
}
