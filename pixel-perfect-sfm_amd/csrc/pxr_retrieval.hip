// pxr_retrieval.hip -- image retrieval: a VLAD global descriptor per image over a vocabulary learned from the scene's own local
// descriptors, and the top num_matched database images per query (pxr_vocab_train, pxr_vlad_aggregate, pxr_retrieval_topk; the
// specification is in include/pixsfm_hip.h and DESIGN.md section 26).
//
// k_sim_tiles<EPI, NT>  the one MFMA tile core, with two epilogues.  A workgroup of four wavefronts owns a strip of 128 rows of A (32
//                    per wavefront) and meets B in groups of NT tiles of 32 columns, one accumulator per tile; both operands go
//                    through LDS in chunks of RT_KC values of k, a chunk of A staged once for the NT tiles, stored in FRAGMENT
//                    order (word kk * 64 + l is what lane l feeds to instruction kk, as in pxr_match.hip).  The
//                    v_mfma_f32_32x32x2_f32 of a tile are issued in ascending k over all chunks on its one accumulator: the
//                    accumulator is the fmaf chain of the specification.
//                      EPI_ASSIGN  persistent workgroups stride over the strips; B is the centroids, NT = 1, 2, 4 or 8 covers all
//                                  of them (K <= 256).  A running (best, index) per accumulator register (columns arrive in
//                                  ascending order, so a strict '>' is "lowest index wins"), a 32-lane butterfly on the key
//                                  (value, -index), one int32 per row.  The loader flags rows that are not valid (an entry that is
//                                  not finite or above 1 in magnitude).
//                      EPI_SIM     NT = 1, one workgroup per (strip, tile): the tile of the n_query x n_db matrix is stored.
// k_vlad_accumulate  one workgroup per (chunk of <= 2048 rows of one group, block of centroids): the fixed-point sums of the block
//                    in LDS as 64-bit integers (LDS integer atomics), merged into global memory with 64-bit integer atomics.
//                    Integer addition commutes: the sums do not depend on any order.  No floating-point atomics.
// k_vocab_update, k_vlad_norms, k_vlad_write   one lane per (group, centroid): the sequential float64 chains of the specification.
// k_topk             one wavefront per query row: num_matched rounds of "the best candidate after the previous winner in the
//                    order (sim descending, j ascending)", a 64-lane butterfly per round.  No sort, no marks, nothing written but
//                    the result.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "pxr_batch.h"
#include "pxr_internal.h"

namespace pxr {
namespace {

constexpr int RT_THREADS = 256;   // four wavefronts
constexpr int RT_ROWS = 128;      // rows of a strip: 32 per wavefront
constexpr int RT_COLS = 32;       // columns of a tile
constexpr int RT_KC = 64;         // values of k per LDS chunk
constexpr int RT_KP = RT_KC / 2;  // instructions per chunk
constexpr int ACC_THREADS = 256;
constexpr int ACC_WORDS = 8192;   // int64 accumulators of a workgroup in LDS (64 KiB): ACC_WORDS / dim centroids per block
constexpr int ACC_ROWS = 2048;    // rows of one accumulation item
constexpr int64_t S_BATCH_WORDS = (int64_t)1 << 25;   // int64 sums of one batch of images in the workspace (256 MiB)

typedef float f32x16 __attribute__((ext_vector_type(16)));

enum { EPI_ASSIGN = 0, EPI_SIM = 1 };

struct TileArgs {
  const float* a; const float* b;   // a: na x dim, b: nb x dim, row-major
  int64_t na;
  int32_t nb, dim;
  int32_t n_col_tiles, grid;
  int64_t n_items;                  // EPI_ASSIGN: strips; EPI_SIM: strips x groups of column tiles
  int32_t* assign;                  // EPI_ASSIGN [na]
  float* sim;                       // EPI_SIM [na][nb]
};

// 32 rows x RT_KC values of k of x (row-major, `dim` wide), from (row0, k0), into fragment order: word (k >> 1) * 64 + (k & 1) * 32 +
// row.  Outside the matrix: zeros.  t of nt threads.  bad (or NULL): bad[row] is set for a row with an entry that is not finite or
// above 1 in magnitude.
__device__ __forceinline__ void stage_rows(float* dst, const float* x, int64_t row0, int64_t n_rows, int dim, int k0, int t, int nt, int* bad) {
  const bool vec = (dim & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  for (int e = t; e < 32 * (RT_KC / 4); e += nt) {
    const int r = e & 31, kq = 4 * (e >> 5), k = k0 + kq;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row0 + r < n_rows && k < dim) {
      const float* p = x + (row0 + r) * (int64_t)dim + k;
      if (vec) v = *reinterpret_cast<const float4*>(p);
      else {
        v.x = p[0];
        if (k + 1 < dim) v.y = p[1];
        if (k + 2 < dim) v.z = p[2];
        if (k + 3 < dim) v.w = p[3];
      }
      if (bad && !(fabsf(v.x) <= 1.0f && fabsf(v.y) <= 1.0f && fabsf(v.z) <= 1.0f && fabsf(v.w) <= 1.0f)) atomicOr(&bad[r], 1);
    }
    float* d = dst + (kq >> 1) * 64 + r;
    d[0] = v.x; d[32] = v.y; d[64] = v.z; d[96] = v.w;
  }
}

// the RT_KP instructions of one chunk on one accumulator, in k order (past dim the chunk holds zeros)
__device__ __forceinline__ f32x16 mfma_chunk(f32x16 acc, const float* a_frag, const float* b_frag) {
#pragma unroll
  for (int kk = 0; kk < RT_KP; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_frag[kk * 64], b_frag[kk * 64], acc, 0, 0, 0);
  return acc;
}

// NT: the column tiles a workgroup holds accumulators for at once.  A chunk of A is staged once for all of them.
template <int EPI, int NT>
__global__ __launch_bounds__(RT_THREADS) void k_sim_tiles(const TileArgs a) {
  __shared__ float as[4][RT_KP * 64];
  __shared__ float bs[NT][RT_KP * 64];
  __shared__ int32_t best_s[RT_ROWS];
  __shared__ int bad_s[RT_ROWS];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, c = lane & 31;
  const int dim = a.dim;
  const int n_chunks = (dim + RT_KC - 1) / RT_KC;
  const int n_groups = (a.n_col_tiles + NT - 1) / NT;                // groups of NT column tiles
  const float NEG = -INFINITY;

  for (int64_t item = blockIdx.x; item < a.n_items; item += a.grid) {
    // an item is one strip and one group of tiles: for an assignment NT covers every centroid (launch_tiles), the group is 0
    const int64_t strip = EPI == EPI_ASSIGN ? item : item / n_groups;
    const int g = EPI == EPI_ASSIGN ? 0 : (int)(item % n_groups);
    const int64_t row_w = strip * RT_ROWS + w * 32;                // the first row of this wavefront
    const int row_l = 4 * h;                                        // + (r & 3) + 8 (r >> 2): the rows of this lane's accumulators

    float bv[16];
    int32_t bi[16];
    if (EPI == EPI_ASSIGN) {
#pragma unroll
      for (int r = 0; r < 16; ++r) { bv[r] = NEG; bi[r] = -1; }
      if (tid < RT_ROWS) bad_s[tid] = 0;
    }

    {
      const int n_t = min(NT, a.n_col_tiles - g * NT);               // tiles of this group: the same on every lane
      f32x16 acc[NT];
#pragma unroll
      for (int u = 0; u < NT; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[u][r] = 0.0f;
      for (int ch = 0; ch < n_chunks; ++ch) {
        const int k0 = ch * RT_KC;
        __syncthreads();                                            // the reads of the previous chunk are done
        stage_rows(as[w], a.a, row_w, a.na, dim, k0, lane, 64, EPI == EPI_ASSIGN ? &bad_s[w * 32] : nullptr);
#pragma unroll
        for (int u = 0; u < NT; ++u)
          if (u < n_t) stage_rows(bs[u], a.b, (int64_t)(g * NT + u) * RT_COLS, a.nb, dim, k0, tid, RT_THREADS, nullptr);
        __syncthreads();
#pragma unroll
        for (int u = 0; u < NT; ++u)
          if (u < n_t) acc[u] = mfma_chunk(acc[u], &as[w][lane], &bs[u][lane]);
      }
#pragma unroll
      for (int u = 0; u < NT; ++u) {                                  // ascending tiles: ascending columns on every lane
        if (u >= n_t) continue;
        const int j = (g * NT + u) * RT_COLS + c;
        const bool col_ok = j < a.nb;
        if (EPI == EPI_ASSIGN) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float v = acc[u][r];
            if (col_ok && v == v && (bi[r] < 0 || v > bv[r])) { bv[r] = v; bi[r] = j; }   // a NaN never wins
          }
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int64_t row = row_w + row_l + (r & 3) + 8 * (r >> 2);
            if (col_ok && row < a.na) a.sim[row * a.nb + j] = acc[u][r];
          }
        }
      }
    }

    if (EPI == EPI_ASSIGN) {
      // the 32 lanes of a half hold the same 16 rows over different columns: key (value, -index), an empty side loses
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v = bv[r];
        int32_t i = bi[r];
#pragma unroll
        for (int mask = 16; mask >= 1; mask >>= 1) {
          const float ov = __shfl_xor(v, mask);
          const int32_t oi = __shfl_xor(i, mask);
          if (oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i))) { v = ov; i = oi; }
        }
        if (c == 0) best_s[w * 32 + row_l + (r & 3) + 8 * (r >> 2)] = i;
      }
      __syncthreads();
      if (tid < RT_ROWS) {
        const int64_t row = strip * RT_ROWS + tid;
        if (row < a.na) a.assign[row] = bad_s[tid] ? -1 : best_s[tid];
      }
    }
  }
}

// ---- fixed-point sums ---------------------------------------------------------------------------------------------------------------
struct AccItem { int64_t row0; int32_t n_rows, group; };

struct AccArgs {
  const float* desc; const int32_t* assign; const AccItem* items;
  unsigned long long* S;   // [groups of the batch][K][dim], zeroed
  int32_t* cnt;            // [groups][K] (all groups), zeroed
  int32_t group0;          // the first group of the batch: S is relative to it
  int32_t dim, K, cb, n_cblocks;
};

// q(x) = llrint((double)x 2^32), as the two's complement word the accumulators add
__device__ __forceinline__ unsigned long long fixed_point(float x) { return (unsigned long long)llrint((double)x * 4294967296.0); }

__global__ __launch_bounds__(ACC_THREADS) void k_vlad_accumulate(const AccArgs a) {
  __shared__ unsigned long long acc[ACC_WORDS];
  __shared__ int cn[PXR_VLAD_MAX_CLUSTERS];
  const int tid = threadIdx.x;
  const AccItem it = a.items[blockIdx.x / a.n_cblocks];
  const int c0 = (int)(blockIdx.x % a.n_cblocks) * a.cb, c1 = min(a.K, c0 + a.cb);
  const int dim = a.dim, n_words = (c1 - c0) * dim;
  for (int x = tid; x < n_words; x += ACC_THREADS) acc[x] = 0;
  for (int x = tid; x < c1 - c0; x += ACC_THREADS) cn[x] = 0;
  __syncthreads();
  if ((dim & 3) == 0 && (reinterpret_cast<uintptr_t>(a.desc) & 15) == 0) {       // four channels per lane and step
    const int dq = dim >> 2, n_q = it.n_rows * dq;                    // <= ACC_ROWS * PXR_VLAD_MAX_DIM / 4
#pragma unroll 4
    for (int e = tid; e < n_q; e += ACC_THREADS) {
      const int r = e / dq, k = 4 * (e - r * dq);
      const int cc = a.assign[it.row0 + r];
      const float4 v = *reinterpret_cast<const float4*>(a.desc + (it.row0 + r) * (int64_t)dim + k);   // not behind the test: both loads in flight
      if (cc >= c0 && cc < c1) {
        unsigned long long* d = &acc[(cc - c0) * dim + k];
        atomicAdd(d, fixed_point(v.x)); atomicAdd(d + 1, fixed_point(v.y)); atomicAdd(d + 2, fixed_point(v.z)); atomicAdd(d + 3, fixed_point(v.w));
      }
    }
  } else {
    const int n_el = it.n_rows * dim;                                 // <= ACC_ROWS * PXR_VLAD_MAX_DIM = 2^20
    for (int e = tid; e < n_el; e += ACC_THREADS) {
      const int r = e / dim, k = e - r * dim;
      const int cc = a.assign[it.row0 + r];
      if (cc >= c0 && cc < c1) atomicAdd(&acc[(cc - c0) * dim + k], fixed_point(a.desc[(it.row0 + r) * (int64_t)dim + k]));
    }
  }
  for (int r = tid; r < it.n_rows; r += ACC_THREADS) {
    const int cc = a.assign[it.row0 + r];
    if (cc >= c0 && cc < c1) atomicAdd(&cn[cc - c0], 1);
  }
  __syncthreads();
  unsigned long long* S = a.S + ((int64_t)(it.group - a.group0) * a.K + c0) * dim;
  for (int x = tid; x < n_words; x += ACC_THREADS)
    if (acc[x] != 0) atomicAdd(&S[x], acc[x]);
  for (int x = tid; x < c1 - c0; x += ACC_THREADS)
    if (cn[x] != 0) atomicAdd(&a.cnt[(int64_t)it.group * a.K + c0 + x], cn[x]);
}

// ---- the vocabulary -----------------------------------------------------------------------------------------------------------------
__global__ void k_gather_rows(const float* desc, int64_t n_total, int64_t n_train, int dim, float* out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_train * dim) return;
  const int64_t j = e / dim, k = e - j * dim;
  out[e] = desc[(j * n_total / n_train) * dim + k];
}

__global__ void k_vocab_init(const float* train, int64_t n_train, int K, int dim, float* C) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= K * dim) return;
  const int c = e / dim, k = e - c * dim;
  C[e] = train[((int64_t)c * n_train / K) * dim + k];
}

__global__ void k_vocab_update(const long long* S, const int32_t* cnt, int K, int dim, float* C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= K || cnt[c] <= 0) return;
  const long long* s = S + (int64_t)c * dim;
  double n2 = 0.0;
  for (int k = 0; k < dim; ++k) { const double v = (double)s[k]; n2 += v * v; }
  if (!(n2 > 0.0)) return;
  const double nrm = sqrt(n2);
  for (int k = 0; k < dim; ++k) C[(int64_t)c * dim + k] = (float)((double)s[k] / nrm);
}

// ---- VLAD ---------------------------------------------------------------------------------------------------------------------------
struct VladArgs {
  const long long* S;      // [images of the batch][K][dim]
  const int32_t* cnt;      // [all images][K]
  const float* C;
  double* b2;              // [images of the batch][K]
  float* G;                // [all images][K dim]
  int32_t m0, n_batch, K, dim;
};

__device__ __forceinline__ double vlad_residual(long long s, int32_t n, float c) { return (double)s * 0x1p-32 - (double)n * (double)c; }

__global__ void k_vlad_norms(const VladArgs a) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.n_batch * a.K) return;
  const int c = e % a.K;
  const int32_t n = a.cnt[(int64_t)a.m0 * a.K + e];
  double b2 = 0.0;
  if (n > 0) {
    const long long* s = a.S + (int64_t)e * a.dim;
    const float* cc = a.C + (int64_t)c * a.dim;
    for (int k = 0; k < a.dim; ++k) { const double v = vlad_residual(s[k], n, cc[k]); b2 += v * v; }
  }
  a.b2[e] = b2;
}

__global__ void k_vlad_write(const VladArgs a) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.n_batch * a.K) return;
  const int m = e / a.K, c = e - m * a.K;
  int nne = 0;
  for (int k = 0; k < a.K; ++k) nne += a.b2[(int64_t)m * a.K + k] > 0.0;
  const double b2 = a.b2[e];
  float* g = a.G + ((int64_t)(a.m0 + m) * a.K + c) * a.dim;
  if (b2 > 0.0) {
    const int32_t n = a.cnt[(int64_t)a.m0 * a.K + e];
    const long long* s = a.S + (int64_t)e * a.dim;
    const float* cc = a.C + (int64_t)c * a.dim;
    const double den = sqrt(b2) * sqrt((double)nne);
    for (int k = 0; k < a.dim; ++k) g[k] = (float)(vlad_residual(s[k], n, cc[k]) / den);
  } else {
    for (int k = 0; k < a.dim; ++k) g[k] = 0.0f;
  }
}

// ---- pair selection -----------------------------------------------------------------------------------------------------------------
struct TopkArgs {
  const float* sim; const int32_t* self; const uint8_t* mask;
  int32_t n_db, num_matched, use_min;
  float min_score;
  int32_t* top_index; float* top_sim; int32_t* n_found;
};

__global__ __launch_bounds__(64) void k_topk(const TopkArgs a) {
  const int64_t i = blockIdx.x;
  const int lane = threadIdx.x;
  const float* s = a.sim + i * a.n_db;
  const uint8_t* mk = a.mask ? a.mask + i * a.n_db : nullptr;
  const int32_t self = a.self ? a.self[i] : -1;
  float pv = 0.0f;
  int32_t pj = -1, found = 0;
  for (int r = 0; r < a.num_matched; ++r) {
    float bv = 0.0f;
    int32_t bj = -1;
    for (int32_t j = lane; j < a.n_db; j += 64) {
      const float v = s[j];
      const bool cand = v == v && j != self && (!mk || mk[j] != 0) && (!a.use_min || v >= a.min_score);
      const bool after = pj < 0 || v < pv || (v == pv && j > pj);
      if (cand && after && (bj < 0 || v > bv)) { bv = v; bj = j; }
    }
#pragma unroll
    for (int mask = 32; mask >= 1; mask >>= 1) {
      const float ov = __shfl_xor(bv, mask);
      const int32_t oj = __shfl_xor(bj, mask);
      if (oj >= 0 && (bj < 0 || ov > bv || (ov == bv && oj < bj))) { bv = ov; bj = oj; }
    }
    if (bj < 0) break;                                               // the same on every lane
    if (lane == 0) { a.top_index[i * a.num_matched + r] = bj; a.top_sim[i * a.num_matched + r] = bv; }
    pv = bv; pj = bj; ++found;
  }
  for (int r = found + lane; r < a.num_matched; r += 64) { a.top_index[i * a.num_matched + r] = -1; a.top_sim[i * a.num_matched + r] = 0.0f; }
  if (lane == 0) a.n_found[i] = found;
}

// ---- host drivers -------------------------------------------------------------------------------------------------------------------
int check_sizes(const char* fn, int64_t n_total, int32_t dim, int32_t K) {
  PXR_REQUIRE(dim >= 1 && dim <= PXR_VLAD_MAX_DIM, "%s: dim = %d is outside [1, %d]", fn, (int)dim, PXR_VLAD_MAX_DIM);
  PXR_REQUIRE(K >= 1 && K <= PXR_VLAD_MAX_CLUSTERS, "%s: n_clusters = %d is outside [1, %d]", fn, (int)K, PXR_VLAD_MAX_CLUSTERS);
  PXR_REQUIRE((int64_t)K * dim <= PXR_VLAD_MAX_GLOBAL_DIM, "%s: n_clusters * dim = %lld is above %d", fn, (long long)K * dim, PXR_VLAD_MAX_GLOBAL_DIM);
  PXR_REQUIRE(n_total >= 0 && n_total < ((int64_t)1 << 30), "%s: n_total = %lld is outside [0, 2^30)", fn, (long long)n_total);
  return PXR_OK;
}

void launch_tiles(pxr_ctx* ctx, int epi, const float* A, int64_t na, const float* B, int32_t nb, int32_t dim, int32_t* assign, float* sim) {
  if (na == 0 || nb == 0) return;
  TileArgs t;
  t.a = A; t.b = B; t.na = na; t.nb = nb; t.dim = dim; t.assign = assign; t.sim = sim;
  t.n_col_tiles = (nb + RT_COLS - 1) / RT_COLS;
  const int64_t strips = (na + RT_ROWS - 1) / RT_ROWS;
  // accumulators per workgroup: all centroids of an assignment (K <= 256: at most 8 tiles); one tile of a similarity, whose
  // n_query x n_db is small against the machine and wants the workgroups more than the reuse of A
  const int nt = epi == EPI_SIM ? 1 : t.n_col_tiles <= 1 ? 1 : t.n_col_tiles <= 2 ? 2 : t.n_col_tiles <= 4 ? 4 : 8;
  t.n_items = epi == EPI_ASSIGN ? strips : strips * ((t.n_col_tiles + nt - 1) / nt);
  t.grid = (int32_t)std::min<int64_t>(t.n_items, (int64_t)std::max(ctx->num_cus, 1) * 8);
  const dim3 grid((unsigned)t.grid), block(RT_THREADS);
  if (epi == EPI_SIM) hipLaunchKernelGGL((k_sim_tiles<EPI_SIM, 1>), grid, block, 0, ctx->stream, t);
  else if (nt == 1) hipLaunchKernelGGL((k_sim_tiles<EPI_ASSIGN, 1>), grid, block, 0, ctx->stream, t);
  else if (nt == 2) hipLaunchKernelGGL((k_sim_tiles<EPI_ASSIGN, 2>), grid, block, 0, ctx->stream, t);
  else if (nt == 4) hipLaunchKernelGGL((k_sim_tiles<EPI_ASSIGN, 4>), grid, block, 0, ctx->stream, t);
  else hipLaunchKernelGGL((k_sim_tiles<EPI_ASSIGN, 8>), grid, block, 0, ctx->stream, t);
}

// the accumulation items of groups [g0, g1) with the offsets `off`, of at most `rows` <= ACC_ROWS rows each, appended to `items`
void push_items(const std::vector<int64_t>& off, int64_t g0, int64_t g1, int64_t rows, std::vector<AccItem>& items) {
  for (int64_t g = g0; g < g1; ++g)
    for (int64_t r = off[g]; r < off[g + 1]; r += rows)
      items.push_back(AccItem{r, (int32_t)std::min<int64_t>(rows, off[g + 1] - r), (int32_t)g});
}

void launch_accumulate(pxr_ctx* ctx, const float* desc, const int32_t* assign, const AccItem* d_items, int64_t n_items, int32_t group0,
                       int32_t dim, int32_t K, unsigned long long* S, int32_t* cnt) {
  if (n_items == 0) return;
  AccArgs a;
  a.desc = desc; a.assign = assign; a.items = d_items; a.S = S; a.cnt = cnt; a.group0 = group0; a.dim = dim; a.K = K;
  a.cb = std::min<int32_t>(K, ACC_WORDS / dim);
  a.n_cblocks = (K + a.cb - 1) / a.cb;
  hipLaunchKernelGGL(k_vlad_accumulate, dim3((unsigned)(n_items * a.n_cblocks)), dim3(ACC_THREADS), 0, ctx->stream, a);
}

int vocab_train(pxr_ctx* ctx, int64_t n_total, int32_t dim, const float* d_desc, int32_t K, int32_t n_iterations, int64_t max_train,
                float* d_centroids, int32_t* d_counts, int32_t* h_n_empty, double* h_ms) {
  const char* fn = "pxr_vocab_train";
  PXR_REQUIRE(ctx && d_desc && d_centroids && d_counts && h_n_empty, "%s: NULL argument", fn);
  if (int rc = check_sizes(fn, n_total, dim, K)) return rc;
  PXR_REQUIRE(n_iterations >= 0, "%s: n_iterations = %d is negative", fn, (int)n_iterations);
  PXR_REQUIRE(max_train >= 1, "%s: max_train = %lld is below 1", fn, (long long)max_train);
  const int64_t n_train = std::min(n_total, max_train);
  PXR_REQUIRE(K <= n_train, "%s: n_clusters = %d is above the %lld training rows", fn, (int)K, (long long)n_train);
  if (h_ms) h_ms[0] = h_ms[1] = h_ms[2] = h_ms[3] = 0.0;
  PXR_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;

  std::vector<int64_t> off{0, n_train};
  std::vector<AccItem> items;
  // one group: chunks small enough that every CU gets two (the merge costs K dim global atomics per chunk)
  push_items(off, 0, 1, std::min<int64_t>(ACC_ROWS, std::max<int64_t>(256, (n_train + 2 * ctx->num_cus - 1) / (2 * std::max(ctx->num_cus, 1)))), items);
  const bool gather = n_train < n_total;
  float* train; int32_t* assign; unsigned long long* S; AccItem* d_items;
  Workspace ws;
  ws.take(train, gather ? (size_t)n_train * dim : 0); ws.take(assign, (size_t)n_train); ws.take(S, (size_t)K * dim); ws.take(d_items, items.size());
  if (int rc = ws.commit(ctx)) return rc;
  const float* rows = gather ? train : d_desc;
  PXR_HIP(hipMemcpyAsync(d_items, items.data(), sizeof(AccItem) * items.size(), hipMemcpyHostToDevice, st));
  PXR_HIP(hipMemsetAsync(d_counts, 0, sizeof(int32_t) * (size_t)K, st));     // (`items` outlives the copy: the counts are read back below)

  {
    StageTimer<2> timer(st, h_ms);                                   // gather and initial centroids
    if (int rc = timer.create(fn)) return rc;
    timer.mark(0);
    if (gather) hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)((n_train * dim + 255) / 256)), dim3(256), 0, st, d_desc, n_total, n_train, (int)dim, train);
    hipLaunchKernelGGL(k_vocab_init, dim3((unsigned)((K * dim + 255) / 256)), dim3(256), 0, st, rows, n_train, (int)K, (int)dim, d_centroids);
    timer.mark(1);
    const int from[1] = {0};
    if (int rc = timer.read(from, 1)) return rc;
  }
  for (int32_t iter = 0; iter < n_iterations; ++iter) {
    double ms[3] = {0.0, 0.0, 0.0};
    StageTimer<4> timer(st, h_ms ? ms : nullptr);                    // assign | accumulate | update
    if (int rc = timer.create(fn)) return rc;
    timer.mark(0);
    launch_tiles(ctx, EPI_ASSIGN, rows, n_train, d_centroids, K, dim, assign, nullptr);
    timer.mark(1);
    PXR_HIP(hipMemsetAsync(S, 0, sizeof(int64_t) * (size_t)K * dim, st));
    PXR_HIP(hipMemsetAsync(d_counts, 0, sizeof(int32_t) * (size_t)K, st));
    launch_accumulate(ctx, rows, assign, d_items, (int64_t)items.size(), 0, dim, K, S, d_counts);
    timer.mark(2);
    hipLaunchKernelGGL(k_vocab_update, dim3((unsigned)((K + 63) / 64)), dim3(64), 0, st, (const long long*)S, (const int32_t*)d_counts, (int)K, (int)dim, d_centroids);
    timer.mark(3);
    const int from[3] = {0, 1, 2};
    if (int rc = timer.read(from, 3)) return rc;
    if (h_ms) { h_ms[1] += ms[0]; h_ms[2] += ms[1]; h_ms[3] += ms[2]; }
  }
  PXR_HIP(hipGetLastError());
  std::vector<int32_t> cnt((size_t)K);
  PXR_HIP(hipMemcpyAsync(cnt.data(), d_counts, sizeof(int32_t) * (size_t)K, hipMemcpyDeviceToHost, st));
  PXR_HIP(hipStreamSynchronize(st));
  int32_t n_empty = 0;
  for (int32_t c = 0; c < K; ++c) n_empty += cnt[(size_t)c] == 0;
  *h_n_empty = n_empty;
  return PXR_OK;
}

int vlad_aggregate(pxr_ctx* ctx, int32_t n_images, const int64_t* d_image_offsets, int64_t n_total, int32_t dim, const float* d_desc,
                   int32_t K, const float* d_centroids, float* d_global, int32_t* d_assign, int32_t* d_counts, double* h_ms) {
  const char* fn = "pxr_vlad_aggregate";
  PXR_REQUIRE(ctx, "%s: NULL argument", fn);
  PXR_REQUIRE(n_images >= 0, "%s: negative size", fn);
  if (int rc = check_sizes(fn, n_total, dim, K)) return rc;
  PXR_REQUIRE(n_images == 0 || (d_image_offsets && d_global && d_centroids), "%s: NULL d_image_offsets / d_global / d_centroids", fn);
  PXR_REQUIRE(n_total == 0 || d_desc, "%s: NULL d_desc", fn);
  if (h_ms) h_ms[0] = h_ms[1] = h_ms[2] = 0.0;
  PXR_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (n_images == 0) { PXR_REQUIRE(n_total == 0, "%s: d_image_offsets ends at 0, not at n_total = %lld", fn, (long long)n_total); return PXR_OK; }

  std::vector<int64_t> off;
  std::vector<int32_t> order;
  const OffsetNames nm{fn, "d_image_offsets", "image", "n_total"};
  if (int rc = batch_order(ctx, nm, false, d_image_offsets, n_images, n_total, off, order, [](int64_t) { return PXR_OK; })) return rc;

  const int64_t per_image = (int64_t)K * dim;
  const int32_t batch = (int32_t)std::max<int64_t>(1, std::min<int64_t>(n_images, S_BATCH_WORDS / per_image));
  std::vector<AccItem> items;
  std::vector<int64_t> first_item;                                   // per batch, and the end
  for (int32_t m0 = 0; m0 < n_images; m0 += batch) {
    first_item.push_back((int64_t)items.size());
    push_items(off, m0, std::min<int64_t>(n_images, (int64_t)m0 + batch), ACC_ROWS, items);
  }
  first_item.push_back((int64_t)items.size());

  int32_t *ws_assign, *ws_cnt; unsigned long long* S; double* b2; AccItem* d_items;
  Workspace ws;
  ws.take(ws_assign, d_assign ? 0 : (size_t)n_total); ws.take(ws_cnt, d_counts ? 0 : (size_t)n_images * K);
  ws.take(S, (size_t)batch * per_image); ws.take(b2, (size_t)batch * K); ws.take(d_items, items.size());
  if (int rc = ws.commit(ctx)) return rc;
  int32_t* assign = d_assign ? d_assign : ws_assign;
  int32_t* cnt = d_counts ? d_counts : ws_cnt;
  if (!items.empty()) PXR_HIP(hipMemcpyAsync(d_items, items.data(), sizeof(AccItem) * items.size(), hipMemcpyHostToDevice, st));
  PXR_HIP(hipMemsetAsync(cnt, 0, sizeof(int32_t) * (size_t)n_images * K, st));
  PXR_HIP(hipStreamSynchronize(st));                                 // an untimed call waits for nothing after this: the copy out of `items` must be over before it returns

  {
    StageTimer<2> timer(st, h_ms);                                   // assign
    if (int rc = timer.create(fn)) return rc;
    timer.mark(0);
    launch_tiles(ctx, EPI_ASSIGN, d_desc, n_total, d_centroids, K, dim, assign, nullptr);
    timer.mark(1);
    const int from[1] = {0};
    if (int rc = timer.read(from, 1)) return rc;
  }
  for (size_t b = 0; b + 1 < first_item.size(); ++b) {
    const int32_t m0 = (int32_t)b * batch, nb = std::min<int32_t>(batch, n_images - m0);
    double ms[2] = {0.0, 0.0};
    StageTimer<3> timer(st, h_ms ? ms : nullptr);                    // accumulate | finalise
    if (int rc = timer.create(fn)) return rc;
    timer.mark(0);
    PXR_HIP(hipMemsetAsync(S, 0, sizeof(int64_t) * (size_t)nb * per_image, st));
    launch_accumulate(ctx, d_desc, assign, d_items + first_item[b], first_item[b + 1] - first_item[b], m0, dim, K, S, cnt);
    timer.mark(1);
    VladArgs v;
    v.S = (const long long*)S; v.cnt = cnt; v.C = d_centroids; v.b2 = b2; v.G = d_global;
    v.m0 = m0; v.n_batch = nb; v.K = K; v.dim = dim;
    const dim3 grid((unsigned)(((int64_t)nb * K + 63) / 64));
    hipLaunchKernelGGL(k_vlad_norms, grid, dim3(64), 0, st, v);
    hipLaunchKernelGGL(k_vlad_write, grid, dim3(64), 0, st, v);
    timer.mark(2);
    const int from[2] = {0, 1};
    if (int rc = timer.read(from, 2)) return rc;
    if (h_ms) { h_ms[1] += ms[0]; h_ms[2] += ms[1]; }
  }
  return hip_check(hipGetLastError(), "k_vlad_write launch");
}

int retrieval_topk(pxr_ctx* ctx, int32_t n_query, int32_t n_db, int32_t dim, const float* d_query, const float* d_db,
                   const int32_t* d_query_self, const uint8_t* d_mask, int32_t num_matched, double min_score, int32_t* d_top_index,
                   float* d_top_sim, int32_t* d_n_found, double* h_ms) {
  const char* fn = "pxr_retrieval_topk";
  PXR_REQUIRE(ctx, "%s: NULL argument", fn);
  PXR_REQUIRE(n_query >= 0 && n_db >= 0, "%s: negative size", fn);
  PXR_REQUIRE(dim >= 1 && dim <= PXR_VLAD_MAX_GLOBAL_DIM, "%s: dim = %d is outside [1, %d]", fn, (int)dim, PXR_VLAD_MAX_GLOBAL_DIM);
  PXR_REQUIRE(num_matched >= 1, "%s: num_matched = %d is below 1", fn, (int)num_matched);
  PXR_REQUIRE(!std::isnan(min_score), "%s: min_score is NaN (infinite: no threshold)", fn);
  PXR_REQUIRE((int64_t)n_query * num_matched < ((int64_t)1 << 31), "%s: more than 2^31 output entries", fn);
  PXR_REQUIRE(n_query == 0 || (d_query && d_top_index && d_top_sim && d_n_found), "%s: NULL d_query / d_top_index / d_top_sim / d_n_found", fn);
  PXR_REQUIRE(n_db == 0 || d_db, "%s: NULL d_db", fn);
  if (h_ms) h_ms[0] = h_ms[1] = 0.0;
  if (n_query == 0) return PXR_OK;
  PXR_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  float* sim;
  Workspace ws;
  ws.take(sim, (size_t)n_query * n_db);
  if (int rc = ws.commit(ctx)) return rc;

  StageTimer<3> timer(st, h_ms);                                     // similarity | select
  if (int rc = timer.create(fn)) return rc;
  timer.mark(0);
  launch_tiles(ctx, EPI_SIM, d_query, n_query, d_db, n_db, dim, nullptr, sim);
  timer.mark(1);
  TopkArgs a;
  a.sim = sim; a.self = d_query_self; a.mask = d_mask; a.n_db = n_db; a.num_matched = num_matched;
  a.use_min = std::isfinite(min_score); a.min_score = a.use_min ? (float)min_score : 0.0f;
  a.top_index = d_top_index; a.top_sim = d_top_sim; a.n_found = d_n_found;
  hipLaunchKernelGGL(k_topk, dim3((unsigned)n_query), dim3(64), 0, st, a);
  timer.mark(2);
  const int rc = hip_check(hipGetLastError(), "k_topk launch");
  const int from[2] = {0, 1};
  return rc == PXR_OK ? timer.read(from, 2) : rc;
}

}  // namespace
}  // namespace pxr

extern "C" int pxr_vocab_train(pxr_ctx* ctx, int64_t n_total, int32_t dim, const float* d_desc, int32_t n_clusters, int32_t n_iterations,
                               int64_t max_train, float* d_centroids, int32_t* d_counts, int32_t* h_n_empty) {
  return pxr::vocab_train(ctx, n_total, dim, d_desc, n_clusters, n_iterations, max_train, d_centroids, d_counts, h_n_empty, nullptr);
}

extern "C" int pxr_vocab_train_timed(pxr_ctx* ctx, int64_t n_total, int32_t dim, const float* d_desc, int32_t n_clusters,
                                     int32_t n_iterations, int64_t max_train, float* d_centroids, int32_t* d_counts, int32_t* h_n_empty,
                                     double* h_kernel_ms) {
  PXR_REQUIRE(h_kernel_ms, "pxr_vocab_train_timed: NULL h_kernel_ms");
  return pxr::vocab_train(ctx, n_total, dim, d_desc, n_clusters, n_iterations, max_train, d_centroids, d_counts, h_n_empty, h_kernel_ms);
}

extern "C" int pxr_vlad_aggregate(pxr_ctx* ctx, int32_t n_images, const int64_t* d_image_offsets, int64_t n_total, int32_t dim,
                                  const float* d_desc, int32_t n_clusters, const float* d_centroids, float* d_global, int32_t* d_assign,
                                  int32_t* d_counts) {
  return pxr::vlad_aggregate(ctx, n_images, d_image_offsets, n_total, dim, d_desc, n_clusters, d_centroids, d_global, d_assign, d_counts,
                             nullptr);
}

extern "C" int pxr_vlad_aggregate_timed(pxr_ctx* ctx, int32_t n_images, const int64_t* d_image_offsets, int64_t n_total, int32_t dim,
                                        const float* d_desc, int32_t n_clusters, const float* d_centroids, float* d_global,
                                        int32_t* d_assign, int32_t* d_counts, double* h_kernel_ms) {
  PXR_REQUIRE(h_kernel_ms, "pxr_vlad_aggregate_timed: NULL h_kernel_ms");
  return pxr::vlad_aggregate(ctx, n_images, d_image_offsets, n_total, dim, d_desc, n_clusters, d_centroids, d_global, d_assign, d_counts,
                             h_kernel_ms);
}

extern "C" int pxr_retrieval_topk(pxr_ctx* ctx, int32_t n_query, int32_t n_db, int32_t dim, const float* d_query, const float* d_db,
                                  const int32_t* d_query_self, const uint8_t* d_mask, int32_t num_matched, double min_score,
                                  int32_t* d_top_index, float* d_top_sim, int32_t* d_n_found) {
  return pxr::retrieval_topk(ctx, n_query, n_db, dim, d_query, d_db, d_query_self, d_mask, num_matched, min_score, d_top_index, d_top_sim,
                             d_n_found, nullptr);
}

extern "C" int pxr_retrieval_topk_timed(pxr_ctx* ctx, int32_t n_query, int32_t n_db, int32_t dim, const float* d_query, const float* d_db,
                                        const int32_t* d_query_self, const uint8_t* d_mask, int32_t num_matched, double min_score,
                                        int32_t* d_top_index, float* d_top_sim, int32_t* d_n_found, double* h_kernel_ms) {
  PXR_REQUIRE(h_kernel_ms, "pxr_retrieval_topk_timed: NULL h_kernel_ms");
  return pxr::retrieval_topk(ctx, n_query, n_db, dim, d_query, d_db, d_query_self, d_mask, num_matched, min_score, d_top_index, d_top_sim,
                             d_n_found, h_kernel_ms);
}
