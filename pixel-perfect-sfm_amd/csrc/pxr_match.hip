// pxr_match.hip -- batched descriptor matching: mutual nearest neighbours of image pairs (pxr_match_descriptors; the specification
// is in include/pixsfm_hip.h and DESIGN.md section 20).
//
// k_match_tiles    one workgroup of four wavefronts per (pair, strip of 128 rows of the first image).  A wavefront owns 32 rows and
//                  keeps their descriptors as MFMA A fragments in registers for the whole sweep (lane l: row l & 31, k = 2 kk + (l >> 5)
//                  in register kk).  The second image goes by in tiles of 32 columns through LDS, double-buffered and shared by the four
//                  wavefronts, stored in FRAGMENT order (word kk * 64 + l is what lane l feeds to instruction kk), so a fragment read is
//                  one linear ds_read_b32 per instruction and needs no padding.  One accumulator per tile, the v_mfma_f32_32x32x2_f32 of a
//                  tile issued in k order: the accumulator is the k-ordered fmaf chain of the specification.  The similarity tile lives in
//                  the 16 accumulator registers only (lane l: column l & 31, rows (r & 3) + 8 (r >> 2) + 4 (l >> 5)):
//                    rows     each lane keeps a running (s1, j1, s2) per register; it meets its columns in ascending order, so a strict
//                             '>' is "lowest index wins".  After the last tile a 32-lane butterfly merges the lanes of a row.
//                    columns  per tile each lane reduces its 16 registers to (s1, i1, s2) of its column, merges with lane l ^ 32, the four
//                             wavefronts meet in LDS and the workgroup writes one partial per column and strip.
//                  Every merge compares keys (value, -index) and takes the second as the maximum of the loser's best and both seconds:
//                  associative and commutative, so no result depends on an order of arrival.  No floating-point atomics.
// k_match_columns  one lane per (pair, column): merges the strips' partials, applies the tests, writes m1.
// k_match_mutual   one workgroup per (pair, strip), one lane per row: the mutual check, matches0 / scores0, one integer add per
//                  workgroup to n_matches.
// pxr_match_guided is the same three kernels with a geometric gate in the tile kernel's epilogue: an entry
// that the pair's two-view model does not admit is masked like a NaN similarity.  k_guided_records computes, once per (pair, row)
// and (pair, column), everything of the gate that depends on one side only; the tile loop has one text, a template over the
// argument struct (MatchArgs / GuidedMatchArgs).
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "pxr_batch.h"
#include "pxr_internal.h"

namespace pxr {
namespace {

constexpr int MT_THREADS = 256;   // four wavefronts
constexpr int MT_ROWS = 128;      // rows of a strip: 32 per wavefront
constexpr int MT_COLS = 32;       // columns of a tile
constexpr int MT_KSTEP = 8;       // instructions between two tests of the k bound: k is padded to a multiple of 2 * MT_KSTEP = 16

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct MatchItem { int32_t pair, strip; };

struct MatchPair {       // one pair, as the host laid it out
  int64_t a_row, b_row;  // first descriptor row of either image
  int64_t out;           // pair_offsets[p]
  int64_t col;           // prefix sum of nb: where the pair's m1 starts
  int64_t part;          // where the pair's partials start (strips x nb entries)
  int32_t na, nb;
};

struct MatchArgs {
  static constexpr bool guided = false;
  const float* desc;
  const MatchPair* pairs;
  const MatchItem* items;
  const int64_t* col_prefix;   // [n_pairs + 1]
  float* part_s1; int32_t* part_i1; float* part_s2;
  int32_t* m1;
  int32_t* matches0; float* scores0; int32_t* n_matches;
  int64_t n_cols;
  int32_t n_pairs, dim, kp;    // kp: k pairs (instructions per tile), a multiple of MT_KSTEP
  float r2, t2;
  int32_t use_ratio, use_dist, mutual;
};

struct GuidedMatchArgs : MatchArgs {   // pxr_match_guided: the gate's arrays on top; the unguided kernels keep the argument they had
  static constexpr bool guided = true;
  const int64_t* row_prefix;   // [n_pairs + 1]: d_pair_offsets
  const double* xy;            // n_total x 2
  const int32_t* kind;         // per pair
  const double* model;         // per pair 9, row-major
  const double* thr;           // per pair
  double* rec_row;             // 4 doubles per output row (at pair.out + row), see k_guided_records
  double* rec_col;             // 4 doubles per column (at pair.col + column)
  int64_t n_rows;
};

struct Top2 { float s1; int32_t i1; float s2; };

__device__ __forceinline__ void top2_push(Top2& t, float v, int32_t idx) {   // indices arrive in ascending order
  if (v > t.s1) { t.s2 = t.s1; t.s1 = v; t.i1 = idx; }
  else if (v > t.s2) t.s2 = v;
}

// key (value, -index); an empty side is (-inf, -1, -inf) and loses to anything but another empty side
__device__ __forceinline__ Top2 top2_merge(const Top2& x, const Top2& y) {
  const bool x_wins = x.s1 > y.s1 || (x.s1 == y.s1 && x.i1 < y.i1);
  Top2 r;
  r.s1 = x_wins ? x.s1 : y.s1;
  r.i1 = x_wins ? x.i1 : y.i1;
  r.s2 = fmaxf(x_wins ? y.s1 : x.s1, fmaxf(x.s2, y.s2));
  return r;
}

__device__ __forceinline__ Top2 top2_shfl_xor(const Top2& t, int mask) {
  Top2 o;
  o.s1 = __shfl_xor(t.s1, mask);
  o.i1 = __shfl_xor(t.i1, mask);
  o.s2 = __shfl_xor(t.s2, mask);
  return o;
}

// the comparisons of the specification: the index that stays, or -1
__device__ __forceinline__ int32_t match_tests(const Top2& t, bool ratio_on, bool dist_on, float r2, float t2) {
  if (t.i1 < 0) return -1;
  const float d1 = 2.0f * (1.0f - t.s1);
  if (ratio_on) {
    const float d2 = 2.0f * (1.0f - t.s2);
    if (!(d1 <= r2 * d2)) return -1;
  }
  if (dist_on && !(d1 <= t2)) return -1;
  return t.i1;
}

// The records of the geometric gate of pxr_match_guided, one lane per (pair, row) and per (pair, column), float64, every operation
// rounded once in the order of the specification (include/pixsfm_hip.h):
//   epipolar    row (l0, l1, l2, ra)    column (u, v, cb, -)
//   homography  row (px, py, valid, -)  column (u, v, -, -)       valid: 1.0 or 0.0
// A model with an entry that is not finite gives NaN records (valid = 0): nothing is admissible for it.
__global__ __launch_bounds__(256) void k_guided_records(const GuidedMatchArgs a) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= a.n_rows + a.n_cols) return;
  const bool is_row = g < a.n_rows;
  const int64_t* prefix = is_row ? a.row_prefix : a.col_prefix;
  const int64_t e = is_row ? g : g - a.n_rows;
  int lo = 0, hi = a.n_pairs;                 // the pair with prefix[pair] <= e < prefix[pair + 1]
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (prefix[mid] <= e) lo = mid; else hi = mid; }
  const MatchPair p = a.pairs[lo];
  const double* M = a.model + 9 * (int64_t)lo;
  bool finite = true;
  for (int k = 0; k < 9; ++k) finite = finite && isfinite(M[k]);
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const int64_t src = is_row ? p.a_row + (e - p.out) : p.b_row + (e - p.col);
  const double x = a.xy[2 * src], y = a.xy[2 * src + 1];
  double r0 = nan, r1 = nan, r2 = nan, r3 = nan;
  if (a.kind[lo] == PXR_GUIDE_EPIPOLAR) {
    if (is_row && finite) {
      r0 = (M[0] * x + M[1] * y) + M[2];
      r1 = (M[3] * x + M[4] * y) + M[5];
      r2 = (M[6] * x + M[7] * y) + M[8];
      r3 = r0 * r0 + r1 * r1;
    } else if (finite) {
      const double m0 = (M[0] * x + M[3] * y) + M[6];
      const double m1 = (M[1] * x + M[4] * y) + M[7];
      r0 = x; r1 = y; r2 = m0 * m0 + m1 * m1; r3 = 0.0;
    }
  } else {
    if (is_row) {
      r2 = 0.0;
      if (finite) {
        const double X = (M[0] * x + M[1] * y) + M[2];
        const double Y = (M[3] * x + M[4] * y) + M[5];
        const double Wd = (M[6] * x + M[7] * y) + M[8];
        r0 = X / Wd; r1 = Y / Wd; r2 = Wd > 0.0 ? 1.0 : 0.0; r3 = 0.0;
      }
    } else if (finite) { r0 = x; r1 = y; r2 = 0.0; r3 = 0.0; }
  }
  double* out = (is_row ? a.rec_row : a.rec_col) + 4 * e;
  out[0] = r0; out[1] = r1; out[2] = r2; out[3] = r3;
}

// KP: k pairs a wavefront can hold (registers of A fragments); the LDS tiles are sized by it too.  Args = GuidedMatchArgs (GUIDED): an
// entry that the pair's model does not admit is masked like a NaN similarity; the strip's 128 row records sit in LDS for the whole
// sweep (the 32 lanes of a half read the same row: a broadcast), the lane's one column record per tile in registers.
template <int KP, class Args>
__global__ __launch_bounds__(MT_THREADS) void k_match_tiles(const Args a) {
  constexpr bool GUIDED = Args::guided;
  __shared__ float bs[2][KP * 64];
  __shared__ double row_rec[GUIDED ? MT_ROWS * 4 : 1];
  __shared__ float cp_s1[2][4][MT_COLS];
  __shared__ int32_t cp_i1[2][4][MT_COLS];
  __shared__ float cp_s2[2][4][MT_COLS];

  const MatchItem it = a.items[blockIdx.x];
  const MatchPair p = a.pairs[it.pair];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, c = lane & 31;
  const int dim = a.dim, kp = a.kp;
  const float NEG = -INFINITY;

  // A fragments: row0 + c, k = 2 kk + h
  const int row_a = it.strip * MT_ROWS + w * 32 + c;            // the row this lane loads (as an A operand)
  float af[KP];
  {
    const bool row_ok = row_a < p.na;
    const float* ap = a.desc + (p.a_row + (row_ok ? row_a : 0)) * (int64_t)dim;
#pragma unroll
    for (int kk = 0; kk < KP; ++kk) {
      const int k = 2 * kk + h;
      af[kk] = (row_ok && k < dim) ? ap[k] : 0.0f;
    }
  }

  // the loader's share of a tile: column tid & 31, k = 4 (q * 8 + (tid >> 5)) .. + 3 for q = 0 .. KP / 16 - 1
  constexpr int NQ = KP / 16;
  const int lc = tid & 31, lk = tid >> 5;
  float4 pf[NQ];
  const bool dim4 = (dim & 3) == 0;
  auto fetch = [&](int tile) {
    const int j = tile * MT_COLS + lc;
    const bool col_ok = j < p.nb;
    const float* bp = a.desc + (p.b_row + (col_ok ? j : 0)) * (int64_t)dim;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int k0 = 4 * (q * 8 + lk);
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (k0 < 2 * kp && col_ok) {
        if (dim4 && k0 + 3 < dim) v = *reinterpret_cast<const float4*>(bp + k0);
        else {
          if (k0 < dim) v.x = bp[k0];
          if (k0 + 1 < dim) v.y = bp[k0 + 1];
          if (k0 + 2 < dim) v.z = bp[k0 + 2];
          if (k0 + 3 < dim) v.w = bp[k0 + 3];
        }
      }
      pf[q] = v;
    }
  };
  auto stash = [&](int buf) {     // k = k0 + e sits at word (k >> 1) * 64 + (k & 1) * 32 + column
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int k0 = 4 * (q * 8 + lk);
      if (k0 < 2 * kp) {
        float* d = &bs[buf][(k0 >> 1) * 64 + lc];
        d[0] = pf[q].x; d[32] = pf[q].y; d[64] = pf[q].z; d[96] = pf[q].w;
      }
    }
  };

  const int n_tiles = (p.nb + MT_COLS - 1) / MT_COLS;
  Top2 rt[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) { rt[r].s1 = NEG; rt[r].i1 = -1; rt[r].s2 = NEG; }

  if (n_tiles > 0) { fetch(0); stash(0); }
  int kind = 0;
  double thr2 = 0.0;
  if constexpr (GUIDED) {
    kind = a.kind[it.pair];
    const double thr = a.thr[it.pair];
    thr2 = thr * thr;
    for (int e = tid; e < MT_ROWS * 4; e += MT_THREADS) {       // rows past the pair's end are masked by row < p.na below
      const int row = it.strip * MT_ROWS + (e >> 2);
      row_rec[e] = row < p.na ? a.rec_row[4 * (p.out + row) + (e & 3)] : 0.0;
    }
  }
  __syncthreads();

  const int row_base = it.strip * MT_ROWS + w * 32 + 4 * h;     // + (r & 3) + 8 (r >> 2): the rows of this lane's accumulators
  for (int t = 0; t < n_tiles; ++t) {
    const int buf = t & 1;
    const bool more = t + 1 < n_tiles;
    if (more) fetch(t + 1);

    double cu = 0.0, cv = 0.0, ccb = 0.0;                       // the column's record: in flight under the instructions below
    if constexpr (GUIDED) {
      const int jc = t * MT_COLS + c;
      const double* cr = a.rec_col + 4 * (p.col + (jc < p.nb ? jc : 0));
      cu = cr[0]; cv = cr[1]; ccb = cr[2];
    }

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    const float* bt = &bs[buf][lane];
#pragma unroll
    for (int g = 0; g < KP / MT_KSTEP; ++g) {
      if (g * MT_KSTEP < kp) {
#pragma unroll
        for (int u = 0; u < MT_KSTEP; ++u) {
          const int kk = g * MT_KSTEP + u;
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[kk], bt[kk * 64], acc, 0, 0, 0);
        }
      }
    }

    const int j = t * MT_COLS + c;
    const bool col_ok = j < p.nb;
    Top2 ct; ct.s1 = NEG; ct.i1 = -1; ct.s2 = NEG;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = row_base + (r & 3) + 8 * (r >> 2);
      float v = acc[r];
      v = (col_ok && row < p.na && v == v) ? v : NEG;           // outside the pair, or NaN: never wins
      if constexpr (GUIDED) {                                   // nor does an entry the model does not admit
        const double* rr = &row_rec[4 * (w * 32 + 4 * h + (r & 3) + 8 * (r >> 2))];
        bool adm;
        if (kind == PXR_GUIDE_EPIPOLAR) {
          const double tt = (cu * rr[0] + cv * rr[1]) + rr[2];
          const double den = rr[3] + ccb;
          adm = den > 0.0 && tt * tt <= thr2 * den;
        } else {
          const double dx = rr[0] - cu, dy = rr[1] - cv;
          adm = rr[2] > 0.0 && dx * dx + dy * dy <= thr2;
        }
        v = adm ? v : NEG;
      }
      top2_push(rt[r], v, j);
      top2_push(ct, v, row);
    }
    if (a.mutual) {
      ct = top2_merge(ct, top2_shfl_xor(ct, 32));
      if (h == 0) { cp_s1[buf][w][c] = ct.s1; cp_i1[buf][w][c] = ct.i1; cp_s2[buf][w][c] = ct.s2; }
    }
    if (more) stash(buf ^ 1);
    __syncthreads();
    if (a.mutual && tid < MT_COLS && t * MT_COLS + tid < p.nb) {
      Top2 m; m.s1 = cp_s1[buf][0][tid]; m.i1 = cp_i1[buf][0][tid]; m.s2 = cp_s2[buf][0][tid];
#pragma unroll
      for (int ww = 1; ww < 4; ++ww) {
        Top2 o; o.s1 = cp_s1[buf][ww][tid]; o.i1 = cp_i1[buf][ww][tid]; o.s2 = cp_s2[buf][ww][tid];
        m = top2_merge(m, o);
      }
      const int64_t at = p.part + (int64_t)it.strip * p.nb + (t * MT_COLS + tid);
      a.part_s1[at] = m.s1; a.part_i1[at] = m.i1; a.part_s2[at] = m.s2;
    }
  }

  // rows: the 32 lanes of a half hold the same 16 rows over different columns
  const bool ratio_on = a.use_ratio && p.na != 1 && p.nb != 1;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    Top2 m = rt[r];
#pragma unroll
    for (int mask = 16; mask >= 1; mask >>= 1) m = top2_merge(m, top2_shfl_xor(m, mask));
    const int row = row_base + (r & 3) + 8 * (r >> 2);
    if (c == 0 && row < p.na) {
      a.matches0[p.out + row] = match_tests(m, ratio_on, a.use_dist != 0, a.r2, a.t2);
      a.scores0[p.out + row] = m.s1;                             // provisional: k_match_mutual turns it into the score
    }
  }
}

__global__ __launch_bounds__(256) void k_match_columns(const MatchArgs a) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= a.n_cols) return;
  int lo = 0, hi = a.n_pairs;                 // the pair with col_prefix[pair] <= g < col_prefix[pair + 1]
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (a.col_prefix[mid] <= g) lo = mid; else hi = mid; }
  const MatchPair p = a.pairs[lo];
  const int64_t j = g - p.col;
  const int n_strips = (p.na + MT_ROWS - 1) / MT_ROWS;
  Top2 m; m.s1 = -INFINITY; m.i1 = -1; m.s2 = -INFINITY;
  for (int s = 0; s < n_strips; ++s) {
    const int64_t at = p.part + (int64_t)s * p.nb + j;
    Top2 o; o.s1 = a.part_s1[at]; o.i1 = a.part_i1[at]; o.s2 = a.part_s2[at];
    m = top2_merge(m, o);
  }
  const bool ratio_on = a.use_ratio && p.na != 1 && p.nb != 1;
  a.m1[g] = match_tests(m, ratio_on, a.use_dist != 0, a.r2, a.t2);
}

__global__ __launch_bounds__(MT_ROWS) void k_match_mutual(const MatchArgs a) {
  const MatchItem it = a.items[blockIdx.x];
  const MatchPair p = a.pairs[it.pair];
  const int row = it.strip * MT_ROWS + threadIdx.x;
  int kept = 0;
  if (row < p.na) {
    int32_t m = a.matches0[p.out + row];
    const float s1 = a.scores0[p.out + row];
    if (m >= 0 && a.mutual && a.m1[p.col + m] != row) m = -1;
    a.matches0[p.out + row] = m;
    a.scores0[p.out + row] = m >= 0 ? (s1 + 1.0f) / 2.0f : 0.0f;
    kept = m >= 0;
  }
  const int total = __syncthreads_count(kept);
  if (threadIdx.x == 0 && total > 0) atomicAdd(&a.n_matches[it.pair], total);
}

struct GuideIn { const double* d_xy; const int32_t* d_kind; const double* d_model; const double* d_thr; };

// gd: the geometric gate of pxr_match_guided, or NULL for pxr_match_descriptors.  h_ms: [3] = tiles, columns, mutual without a gate,
// [4] = records, tiles, columns, mutual with one.
int match_descriptors(pxr_ctx* ctx, int32_t n_images, const int64_t* d_image_offsets, int64_t n_total, int32_t dim, const float* d_desc,
                      int32_t n_pairs, const int32_t* d_pairs, const int64_t* d_pair_offsets, const pxr_match_options* o,
                      int32_t* d_matches0, float* d_scores0, int32_t* d_n_matches, double* h_ms, const GuideIn* gd = nullptr) {
  const char* fn = gd ? "pxr_match_guided" : "pxr_match_descriptors";
  PXR_REQUIRE(ctx && o, "%s: NULL argument", fn);
  PXR_REQUIRE(n_images >= 0 && n_total >= 0 && n_pairs >= 0, "%s: negative size", fn);
  PXR_REQUIRE(dim >= 1 && dim <= PXR_MATCH_MAX_DIM, "%s: dim = %d is outside [1, %d]", fn, (int)dim, PXR_MATCH_MAX_DIM);
  PXR_REQUIRE(n_total < ((int64_t)1 << 31), "%s: n_total = %lld: more than 2^31 descriptors", fn, (long long)n_total);
  PXR_REQUIRE(std::isfinite(o->ratio_threshold) && std::isfinite(o->distance_threshold), "%s: options: a threshold is not finite", fn);
  PXR_REQUIRE(o->reserved == 0, "%s: options.reserved must be 0", fn);
  PXR_REQUIRE(n_images == 0 || d_image_offsets, "%s: NULL d_image_offsets", fn);
  PXR_REQUIRE(n_total == 0 || d_desc, "%s: NULL d_desc", fn);
  PXR_REQUIRE(n_pairs == 0 || (d_pairs && d_pair_offsets && d_n_matches), "%s: NULL d_pairs / d_pair_offsets / d_n_matches", fn);
  if (gd) {
    PXR_REQUIRE(n_total == 0 || gd->d_xy, "%s: NULL d_xy", fn);
    PXR_REQUIRE(n_pairs == 0 || (gd->d_kind && gd->d_model && gd->d_thr), "%s: NULL d_pair_kind / d_pair_model / d_pair_thr", fn);
  }
  if (h_ms) for (int k = 0; k < (gd ? 4 : 3); ++k) h_ms[k] = 0.0;
  PXR_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;

  // validation on a host copy of the offsets and the pairs
  std::vector<int64_t> off((size_t)n_images + 1, 0), pair_off((size_t)n_pairs + 1, 0);
  std::vector<int32_t> pairs((size_t)n_pairs * 2);
  if (n_images > 0) PXR_HIP(hipMemcpyAsync(off.data(), d_image_offsets, sizeof(int64_t) * off.size(), hipMemcpyDeviceToHost, st));
  if (n_pairs > 0) {
    PXR_HIP(hipMemcpyAsync(pairs.data(), d_pairs, sizeof(int32_t) * pairs.size(), hipMemcpyDeviceToHost, st));
    PXR_HIP(hipMemcpyAsync(pair_off.data(), d_pair_offsets, sizeof(int64_t) * pair_off.size(), hipMemcpyDeviceToHost, st));
  }
  std::vector<int32_t> kinds(gd ? (size_t)n_pairs : 0);
  std::vector<double> thrs(gd ? (size_t)n_pairs : 0);
  if (gd && n_pairs > 0) {
    PXR_HIP(hipMemcpyAsync(kinds.data(), gd->d_kind, sizeof(int32_t) * kinds.size(), hipMemcpyDeviceToHost, st));
    PXR_HIP(hipMemcpyAsync(thrs.data(), gd->d_thr, sizeof(double) * thrs.size(), hipMemcpyDeviceToHost, st));
  }
  PXR_HIP(hipStreamSynchronize(st));
  for (size_t p = 0; p < kinds.size(); ++p) {
    PXR_REQUIRE(kinds[p] == PXR_GUIDE_EPIPOLAR || kinds[p] == PXR_GUIDE_HOMOGRAPHY, "%s: d_pair_kind[%d] = %d is neither PXR_GUIDE_EPIPOLAR nor "
                "PXR_GUIDE_HOMOGRAPHY", fn, (int)p, (int)kinds[p]);
    PXR_REQUIRE(thrs[p] >= 0.0, "%s: d_pair_thr[%d] is NaN or negative", fn, (int)p);
  }
  PXR_REQUIRE(off[0] == 0, "%s: d_image_offsets[0] = %lld, not 0", fn, (long long)off[0]);
  for (int32_t m = 0; m < n_images; ++m)
    PXR_REQUIRE(off[m + 1] >= off[m], "%s: d_image_offsets is not monotone at image %d", fn, (int)m);
  PXR_REQUIRE(off[n_images] == n_total, "%s: d_image_offsets ends at %lld, not at n_total = %lld", fn, (long long)off[n_images], (long long)n_total);

  std::vector<MatchPair> hp((size_t)n_pairs);
  std::vector<MatchItem> items;
  std::vector<int64_t> col_prefix((size_t)n_pairs + 1, 0);
  int64_t rows = 0, cols = 0, parts = 0;
  for (int32_t p = 0; p < n_pairs; ++p) {
    const int32_t ia = pairs[2 * (size_t)p], ib = pairs[2 * (size_t)p + 1];
    PXR_REQUIRE(ia >= 0 && ia < n_images && ib >= 0 && ib < n_images, "%s: d_pairs[%d] = (%d, %d) names an image outside [0, n_images = %d)",
                fn, (int)p, (int)ia, (int)ib, (int)n_images);
    MatchPair& q = hp[(size_t)p];
    q.a_row = off[ia]; q.na = (int32_t)(off[ia + 1] - off[ia]);
    q.b_row = off[ib]; q.nb = (int32_t)(off[ib + 1] - off[ib]);
    PXR_REQUIRE(pair_off[p] == rows, "%s: d_pair_offsets[%d] = %lld is not the prefix sum of the first images' sizes (%lld)", fn, (int)p,
                (long long)pair_off[p], (long long)rows);
    q.out = rows; q.col = cols; q.part = parts;
    const int32_t n_strips = (q.na + MT_ROWS - 1) / MT_ROWS;
    for (int32_t s = 0; s < n_strips; ++s) items.push_back(MatchItem{p, s});
    rows += q.na;
    if (q.na > 0) { cols += q.nb; parts += (int64_t)n_strips * q.nb; }
    col_prefix[(size_t)p + 1] = cols;
  }
  PXR_REQUIRE(pair_off[n_pairs] == rows, "%s: d_pair_offsets ends at %lld, not at the sum of the first images' sizes (%lld)", fn,
              (long long)pair_off[n_pairs], (long long)rows);
  PXR_REQUIRE(rows < ((int64_t)1 << 31) && items.size() < ((size_t)1 << 31), "%s: more than 2^31 output rows", fn);
  PXR_REQUIRE(rows == 0 || (d_matches0 && d_scores0), "%s: NULL d_matches0 / d_scores0", fn);
  if (rows == 0) {                   // no pairs, or only empty first images: nothing to write but zero counts, nothing to launch
    if (n_pairs > 0) PXR_HIP(hipMemsetAsync(d_n_matches, 0, sizeof(int32_t) * (size_t)n_pairs, st));
    return PXR_OK;
  }
  const bool mutual = o->do_mutual_check != 0;

  GuidedMatchArgs a{};
  a.desc = d_desc;
  MatchPair* d_hp; MatchItem* d_items; int64_t* d_col_prefix;      // (the host fills these three; the kernels only read them)
  Workspace ws;
  ws.take(d_hp, hp.size()); ws.take(d_items, items.size()); ws.take(d_col_prefix, col_prefix.size()); ws.take(a.m1, (size_t)cols);
  ws.take(a.part_s1, (size_t)parts); ws.take(a.part_i1, (size_t)parts); ws.take(a.part_s2, (size_t)parts);
  ws.take(a.rec_row, gd ? (size_t)rows * 4 : 0); ws.take(a.rec_col, gd ? (size_t)cols * 4 : 0);
  if (int rc = ws.commit(ctx)) return rc;
  a.pairs = d_hp; a.items = d_items; a.col_prefix = d_col_prefix;
  a.matches0 = d_matches0; a.scores0 = d_scores0; a.n_matches = d_n_matches;
  a.n_cols = cols; a.n_pairs = n_pairs; a.dim = dim;
  a.kp = ((dim + 1) / 2 + MT_KSTEP - 1) / MT_KSTEP * MT_KSTEP;
  a.r2 = (float)(o->ratio_threshold * o->ratio_threshold);
  a.t2 = (float)(o->distance_threshold * o->distance_threshold);
  a.use_ratio = o->ratio_threshold > 0.0; a.use_dist = o->distance_threshold > 0.0; a.mutual = mutual;
  if (gd) {
    a.row_prefix = d_pair_offsets; a.xy = gd->d_xy; a.kind = gd->d_kind; a.model = gd->d_model; a.thr = gd->d_thr;
    a.n_rows = rows;
  }
  const MatchArgs& au = a;                               // what the unguided kernels take

  StageTimer<5> timer(st, h_ms);                         // records (with a gate) | tiles | columns | mutual
  if (int rc = timer.create(fn)) return rc;

  int rc = hip_check(hipMemcpyAsync(d_hp, hp.data(), sizeof(MatchPair) * hp.size(), hipMemcpyHostToDevice, st), "hipMemcpyAsync");
  if (rc == PXR_OK) rc = hip_check(hipMemcpyAsync(d_items, items.data(), sizeof(MatchItem) * items.size(), hipMemcpyHostToDevice, st), "hipMemcpyAsync");
  if (rc == PXR_OK) rc = hip_check(hipMemcpyAsync(d_col_prefix, col_prefix.data(), 8 * col_prefix.size(), hipMemcpyHostToDevice, st), "hipMemcpyAsync");
  if (rc == PXR_OK) rc = hip_check(hipMemsetAsync(d_n_matches, 0, sizeof(int32_t) * (size_t)n_pairs, st), "hipMemsetAsync");
  if (rc == PXR_OK) rc = hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");      // (the host vectors may go out of scope)
  if (rc != PXR_OK) return rc;

  const dim3 grid((unsigned)items.size());
  if (gd) {
    timer.mark(0);
    hipLaunchKernelGGL(k_guided_records, dim3((unsigned)((rows + cols + 255) / 256)), dim3(256), 0, st, a);
  }
  timer.mark(1);
  if (gd) {
    if (a.kp <= 64) hipLaunchKernelGGL((k_match_tiles<64, GuidedMatchArgs>), grid, dim3(MT_THREADS), 0, st, a);
    else if (a.kp <= 128) hipLaunchKernelGGL((k_match_tiles<128, GuidedMatchArgs>), grid, dim3(MT_THREADS), 0, st, a);
    else hipLaunchKernelGGL((k_match_tiles<256, GuidedMatchArgs>), grid, dim3(MT_THREADS), 0, st, a);
  } else {
    if (a.kp <= 64) hipLaunchKernelGGL((k_match_tiles<64, MatchArgs>), grid, dim3(MT_THREADS), 0, st, au);
    else if (a.kp <= 128) hipLaunchKernelGGL((k_match_tiles<128, MatchArgs>), grid, dim3(MT_THREADS), 0, st, au);
    else hipLaunchKernelGGL((k_match_tiles<256, MatchArgs>), grid, dim3(MT_THREADS), 0, st, au);
  }
  timer.mark(2);
  if (mutual && cols > 0) hipLaunchKernelGGL(k_match_columns, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, st, au);
  timer.mark(3);
  hipLaunchKernelGGL(k_match_mutual, grid, dim3(MT_ROWS), 0, st, au);
  timer.mark(4);
  rc = hip_check(hipGetLastError(), "k_match_mutual launch");
  const int from[4] = {0, 1, 2, 3};
  return rc == PXR_OK ? (gd ? timer.read(from, 4) : timer.read(from + 1, 3)) : rc;
}

}  // namespace
}  // namespace pxr

extern "C" void pxr_match_default_options(pxr_match_options* o) {
  if (!o) return;
  o->ratio_threshold = 0.0; o->distance_threshold = 0.0; o->do_mutual_check = 1; o->reserved = 0;
}

extern "C" int pxr_match_descriptors(pxr_ctx* ctx, int32_t n_images, const int64_t* d_image_offsets, int64_t n_total, int32_t dim,
                                     const float* d_desc, int32_t n_pairs, const int32_t* d_pairs, const int64_t* d_pair_offsets,
                                     const pxr_match_options* options, int32_t* d_matches0, float* d_scores0, int32_t* d_n_matches) {
  return pxr::match_descriptors(ctx, n_images, d_image_offsets, n_total, dim, d_desc, n_pairs, d_pairs, d_pair_offsets, options,
                                d_matches0, d_scores0, d_n_matches, nullptr);
}

extern "C" int pxr_match_descriptors_timed(pxr_ctx* ctx, int32_t n_images, const int64_t* d_image_offsets, int64_t n_total, int32_t dim,
                                           const float* d_desc, int32_t n_pairs, const int32_t* d_pairs, const int64_t* d_pair_offsets,
                                           const pxr_match_options* options, int32_t* d_matches0, float* d_scores0, int32_t* d_n_matches,
                                           double* h_kernel_ms) {
  PXR_REQUIRE(h_kernel_ms, "pxr_match_descriptors_timed: NULL h_kernel_ms");
  return pxr::match_descriptors(ctx, n_images, d_image_offsets, n_total, dim, d_desc, n_pairs, d_pairs, d_pair_offsets, options,
                                d_matches0, d_scores0, d_n_matches, h_kernel_ms);
}

extern "C" int pxr_match_guided(pxr_ctx* ctx, int32_t n_images, const int64_t* d_image_offsets, int64_t n_total, int32_t dim, const float* d_desc,
                                const double* d_xy, int32_t n_pairs, const int32_t* d_pairs, const int64_t* d_pair_offsets,
                                const int32_t* d_pair_kind, const double* d_pair_model, const double* d_pair_thr,
                                const pxr_match_options* options, int32_t* d_matches0, float* d_scores0, int32_t* d_n_matches) {
  const pxr::GuideIn gd = {d_xy, d_pair_kind, d_pair_model, d_pair_thr};
  return pxr::match_descriptors(ctx, n_images, d_image_offsets, n_total, dim, d_desc, n_pairs, d_pairs, d_pair_offsets, options,
                                d_matches0, d_scores0, d_n_matches, nullptr, &gd);
}

extern "C" int pxr_match_guided_timed(pxr_ctx* ctx, int32_t n_images, const int64_t* d_image_offsets, int64_t n_total, int32_t dim,
                                      const float* d_desc, const double* d_xy, int32_t n_pairs, const int32_t* d_pairs,
                                      const int64_t* d_pair_offsets, const int32_t* d_pair_kind, const double* d_pair_model,
                                      const double* d_pair_thr, const pxr_match_options* options, int32_t* d_matches0, float* d_scores0,
                                      int32_t* d_n_matches, double* h_kernel_ms) {
  PXR_REQUIRE(h_kernel_ms, "pxr_match_guided_timed: NULL h_kernel_ms");
  const pxr::GuideIn gd = {d_xy, d_pair_kind, d_pair_model, d_pair_thr};
  return pxr::match_descriptors(ctx, n_images, d_image_offsets, n_total, dim, d_desc, n_pairs, d_pairs, d_pair_offsets, options,
                                d_matches0, d_scores0, d_n_matches, h_kernel_ms, &gd);
}
