// pxr_sift.hip -- SIFT keypoints and descriptors of one grey image on gfx950: Gaussian scale space, extrema of the differences
// with sub-pixel refinement, orientations, 4 x 4 x 8 descriptors.  The definition is the comment above pxr_sift_pyramid in
// include/pixsfm_hip.h (restated from Lowe's paper and VLFeat's sift.c as remembered -- parity unpinned);
// tests/sift_cases.py is its transcription in numpy.
//
//   k_sift_upsample  the image as float32, doubled for first_octave = -1
//   k_sift_blur<0|1> one pass of a separable blur (rows | columns) through an LDS tile with a halo of r <= 18, borders replicated;
//                    the float32 sum runs over the taps in ascending order from 0, one rounding per product and per addition
//   k_sift_half      level 0 of an octave: level S of the octave before at even indices
//   k_sift_detect    <false> counts the keypoints of every block of 1024 DoG samples, <true> writes them behind the block's offset
//                    in sample order -- count, scan, write: the order (o, s, yi, xi) without an atomic.  The DoG is formed on the
//                    fly from two levels; the refinement of an extremum runs in float64 on its own lane
//   k_exclusive_scan (pxr_scan.h) the exclusive prefix sums (blocks -> keypoints, keypoints -> features)
//   k_sift_orient    one wavefront per keypoint: the 36-bin histogram, owner-computes (see below), then lane 0 smooths and picks
//   k_sift_emit      keypoint x orientation -> feature rows below `capacity`
//   k_sift_gather    rows of the detector's output by index, split into keypoints, scales, orientations, scores (the bindings)
//   k_sift_describe  128 lanes per feature, lane = the bin (by, bx, bo) it owns
//
// Owner-computes histograms: the samples of a chunk are staged in LDS as (value, bin coordinates) and every lane adds the share of
// its own bin in sample order, so a sum never depends on which lane arrived first; no float atomics.  Everything downstream of
// the float32 pyramid is float64.  Every branch that encloses __syncthreads or a shuffle is uniform over the workgroup.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "pxr_batch.h"
#include "pxr_internal.h"
#include "pxr_scan.h"

namespace pxr {

constexpr int SIFT_THREADS = 256;
constexpr int SIFT_WAVES = SIFT_THREADS / 64;
constexpr int SIFT_MAX_R = 18;                     // the largest increment of the allowed S: 4.5 px at S = 2
constexpr int SIFT_MAX_OCTAVES = 8;
constexpr int SIFT_MIN_SIDE = 16;
constexpr int SIFT_MAX_PLANES = SIFT_MAX_OCTAVES * 4;
constexpr int SIFT_BLOCK_SAMPLES = 4 * SIFT_THREADS;   // DoG samples per workgroup of k_sift_detect
constexpr int SIFT_ROW_TILE = 4, SIFT_COL_TILE = 16;   // rows of a tile of the row pass / the column pass (64 columns both)
constexpr int SIFT_MAX_GRID = 32768;                // workgroups of the per-keypoint kernels (they stride over the rest)
constexpr double SIFT_TWO_PI = 6.283185307179586476925286766559;

struct SiftTaps { int r; float w[2 * SIFT_MAX_R + 1]; };

// plane (k, s) of the pyramid: h[k] x w[k] float32 at off[k] + s h[k] w[k]; octave index k holds octave first + k
struct SiftLayout {
  int n_oct, S, first;
  int h[SIFT_MAX_OCTAVES], w[SIFT_MAX_OCTAVES];
  int64_t off[SIFT_MAX_OCTAVES];
  int64_t total;                                    // floats
};

struct SiftDetect {
  const float* pyr;
  SiftLayout L;
  double peak, edge_bound, sigma0;
  int max_steps, n_planes;
  int plane_k[SIFT_MAX_PLANES], plane_s[SIFT_MAX_PLANES], plane_first[SIFT_MAX_PLANES + 1];   // the blocks of plane p begin at plane_first[p]
  int32_t* block_count;                             // [n_blocks]
  const int64_t* block_off;                         // [n_blocks + 1]
  double* kp;                                       // [kp_cap][4] x, y, sigma, s + ds
  int32_t* rec;                                     // [kp_cap][4] o, s, xi, yi
  double* resp;                                     // [kp_cap]
  int64_t kp_cap;
};

struct SiftKp { double x, y, sigma, sref, resp; };

// ---- the image and the scale space ----------------------------------------------------------------------------------------------
__device__ __forceinline__ float sift_pixel(const void* img, int dtype, size_t i) {
  return dtype == PXR_U8 ? (float)static_cast<const uint8_t*>(img)[i] / 255.0f : static_cast<const float*>(img)[i];
}

// up = 1: u(2i) = I(i), u(2i + 1) = (I(i) + I(min(i + 1, n - 1))) / 2 along x, then along y; up = 0: the conversion alone
__global__ __launch_bounds__(SIFT_THREADS) void k_sift_upsample(const void* img, int dtype, int h, int w, int up, float* __restrict__ out) {
  const int H = up ? 2 * h : h, W = up ? 2 * w : w;
  const size_t i = (size_t)blockIdx.x * SIFT_THREADS + threadIdx.x;
  if (i >= (size_t)H * W) return;
  const int Y = (int)(i / W), X = (int)(i % W);
  if (!up) { out[i] = sift_pixel(img, dtype, i); return; }
  const int y0 = Y >> 1, x0 = X >> 1, y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
  float top = sift_pixel(img, dtype, (size_t)y0 * w + x0);
  if (X & 1) top = (top + sift_pixel(img, dtype, (size_t)y0 * w + x1)) * 0.5f;
  if (Y & 1) {
    float bot = sift_pixel(img, dtype, (size_t)y1 * w + x0);
    if (X & 1) bot = (bot + sift_pixel(img, dtype, (size_t)y1 * w + x1)) * 0.5f;
    top = (top + bot) * 0.5f;
  }
  out[i] = top;
}

// DIR = 0: along x, a tile of 64 x SIFT_ROW_TILE outputs; DIR = 1: along y, a tile of 64 x SIFT_COL_TILE outputs.  Every load is
// clamped into the level (replicated borders; also what keeps the halo of a tile at the edge inside the plane).
template <int DIR>
__global__ __launch_bounds__(SIFT_THREADS) void k_sift_blur(const float* __restrict__ src, float* __restrict__ dst, int h, int w, const SiftTaps t) {
  constexpr int ROWS = DIR == 0 ? SIFT_ROW_TILE : SIFT_COL_TILE + 2 * SIFT_MAX_R;
  constexpr int COLS = DIR == 0 ? 64 + 2 * SIFT_MAX_R : 64;
  __shared__ float s_tile[ROWS * COLS];
  const int tiles_x = (w + 63) / 64;
  const int tx = (int)(blockIdx.x % (unsigned)tiles_x) * 64, ty = (int)(blockIdx.x / (unsigned)tiles_x) * (DIR == 0 ? SIFT_ROW_TILE : SIFT_COL_TILE);
  const int r = t.r;
  const int rows = DIR == 0 ? SIFT_ROW_TILE : SIFT_COL_TILE + 2 * r, cols = DIR == 0 ? 64 + 2 * r : 64;
  for (int i = threadIdx.x; i < rows * cols; i += SIFT_THREADS) {
    const int row = i / cols, col = i % cols;
    const int gy = min(max(ty + row - (DIR == 0 ? 0 : r), 0), h - 1), gx = min(max(tx + col - (DIR == 0 ? r : 0), 0), w - 1);
    s_tile[row * COLS + col] = src[(size_t)gy * w + gx];
  }
  __syncthreads();
  const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
  const int x = tx + lx;
  if (x >= w) return;
  if (DIR == 0) {
    const int y = ty + ly;
    if (y >= h) return;
    float acc = 0.f;
    for (int k = 0; k <= 2 * r; ++k) acc = acc + t.w[k] * s_tile[ly * COLS + lx + k];
    dst[(size_t)y * w + x] = acc;
  } else {
    for (int j = 0; j < SIFT_COL_TILE / SIFT_WAVES; ++j) {
      const int row = ly + SIFT_WAVES * j, y = ty + row;
      if (y >= h) break;
      float acc = 0.f;
      for (int k = 0; k <= 2 * r; ++k) acc = acc + t.w[k] * s_tile[(row + k) * COLS + lx];
      dst[(size_t)y * w + x] = acc;
    }
  }
}

__global__ __launch_bounds__(SIFT_THREADS) void k_sift_half(const float* __restrict__ src, int ws, float* __restrict__ dst, int h, int w) {
  const size_t i = (size_t)blockIdx.x * SIFT_THREADS + threadIdx.x;
  if (i >= (size_t)h * w) return;
  const int y = (int)(i / w), x = (int)(i % w);
  dst[i] = src[(size_t)(2 * y) * ws + 2 * x];         // 2 y <= h_s - 1 and 2 x <= w_s - 1 because h = (h_s + 1) / 2
}

// ---- detection ------------------------------------------------------------------------------------------------------------------
// H d = b by Gaussian elimination with partial pivoting (the first largest pivot); false at a zero pivot
__device__ __forceinline__ bool sift_solve3(double A[3][4], double d[3]) {
  for (int c = 0; c < 3; ++c) {
    int p = c;
    for (int r = c + 1; r < 3; ++r) if (fabs(A[r][c]) > fabs(A[p][c])) p = r;
    if (A[p][c] == 0.0) return false;
    if (p != c) for (int j = 0; j < 4; ++j) { const double v = A[c][j]; A[c][j] = A[p][j]; A[p][j] = v; }
    for (int r = c + 1; r < 3; ++r) {
      const double f = A[r][c] / A[c][c];
      for (int j = c; j < 4; ++j) A[r][j] = A[r][j] - f * A[c][j];
    }
  }
  for (int c = 2; c >= 0; --c) {
    double v = A[c][3];
    for (int j = c + 1; j < 3; ++j) v = v - A[c][j] * d[j];
    d[c] = v / A[c][c];
  }
  return true;
}

// the DoG sample (k, s, y, x), 1 <= s <= S and one pixel inside the border: is it a keypoint, and which
__device__ bool sift_candidate(const SiftDetect& a, int k, int s, int x, int y, SiftKp& out) {
  const int h = a.L.h[k], w = a.L.w[k], S = a.L.S;
  const size_t plane = (size_t)h * w;
  const float* G = a.pyr + a.L.off[k];
  auto D = [&](int ss, int yy, int xx) -> double {
    const size_t i = (size_t)yy * w + xx;
    return (double)G[(size_t)(ss + 1) * plane + i] - (double)G[(size_t)ss * plane + i];
  };
  const double v0 = D(s, y, x);
  if (!(fabs(v0) > 0.8 * a.peak)) return false;
  bool above = true, below = true;
  for (int ds = -1; ds <= 1; ++ds)
    for (int dy = -1; dy <= 1; ++dy) {
      for (int dx = -1; dx <= 1; ++dx) {
        if (ds == 0 && dy == 0 && dx == 0) continue;
        const double n = D(s + ds, y + dy, x + dx);
        above = above && v0 > n;
        below = below && v0 < n;
      }
      if (!above && !below) return false;
    }
  int X = x, Y = y;
  double d[3], g[3], v = v0, hxx = 0, hyy = 0, hxy = 0;
  for (int step = 0;; ++step) {
    v = D(s, Y, X);
    const double xp = D(s, Y, X + 1), xm = D(s, Y, X - 1), yp = D(s, Y + 1, X), ym = D(s, Y - 1, X), sp = D(s + 1, Y, X), sm = D(s - 1, Y, X);
    g[0] = 0.5 * (xp - xm); g[1] = 0.5 * (yp - ym); g[2] = 0.5 * (sp - sm);
    hxx = xp + xm - 2.0 * v; hyy = yp + ym - 2.0 * v;
    const double hss = sp + sm - 2.0 * v;
    hxy = 0.25 * (D(s, Y + 1, X + 1) + D(s, Y - 1, X - 1) - D(s, Y + 1, X - 1) - D(s, Y - 1, X + 1));
    const double hxs = 0.25 * (D(s + 1, Y, X + 1) + D(s - 1, Y, X - 1) - D(s + 1, Y, X - 1) - D(s - 1, Y, X + 1));
    const double hys = 0.25 * (D(s + 1, Y + 1, X) + D(s - 1, Y - 1, X) - D(s + 1, Y - 1, X) - D(s - 1, Y + 1, X));
    double A[3][4] = {{hxx, hxy, hxs, -g[0]}, {hxy, hyy, hys, -g[1]}, {hxs, hys, hss, -g[2]}};
    if (!sift_solve3(A, d)) return false;
    if (step == a.max_steps) break;
    const int sx = (d[0] > 0.6 && X + 1 <= w - 2) ? 1 : (d[0] < -0.6 && X - 1 >= 1) ? -1 : 0;
    const int sy = (d[1] > 0.6 && Y + 1 <= h - 2) ? 1 : (d[1] < -0.6 && Y - 1 >= 1) ? -1 : 0;
    if (sx == 0 && sy == 0) break;
    X += sx; Y += sy;
  }
  const double val = v + 0.5 * (g[0] * d[0] + g[1] * d[1] + g[2] * d[2]);
  const double det = hxx * hyy - hxy * hxy, tr = hxx + hyy;
  const double sref = (double)s + d[2];
  if (!(fabs(d[0]) < 1.5 && fabs(d[1]) < 1.5 && fabs(d[2]) < 1.5)) return false;
  if (!(sref >= 0.0 && sref <= (double)(S + 1))) return false;
  if (!(fabs(val) > a.peak)) return false;
  if (!(det > 0.0 && a.edge_bound * det - tr * tr > 0.0)) return false;
  const int o = a.L.first + k;
  const double scale = o < 0 ? 0.5 : (double)(1 << o);
  out.x = ((double)X + d[0]) * scale;
  out.y = ((double)Y + d[1]) * scale;
  out.sref = sref;
  out.sigma = a.sigma0 * exp2((double)o + sref / (double)S);
  out.resp = fabs(val);
  return true;
}

template <bool WRITE>
__global__ __launch_bounds__(SIFT_THREADS) void k_sift_detect(const SiftDetect a) {
  __shared__ long long s_part[SIFT_WAVES];
  const int b = blockIdx.x;
  int p = 0;
  while (p + 1 < a.n_planes && a.plane_first[p + 1] <= b) ++p;
  const int k = a.plane_k[p], s = a.plane_s[p], h = a.L.h[k], w = a.L.w[k];
  const long long n = (long long)h * w, base = (long long)(b - a.plane_first[p]) * SIFT_BLOCK_SAMPLES;
  long long at = WRITE ? a.block_off[b] : 0;
  if (WRITE && a.block_off[b + 1] == at) return;          // (uniform) nothing to write
  for (int c = 0; c < SIFT_BLOCK_SAMPLES / SIFT_THREADS; ++c) {
    const long long i = base + c * SIFT_THREADS + threadIdx.x;
    SiftKp kp;
    bool found = false;
    int x = 0, y = 0;
    if (i < n) {
      y = (int)(i / w); x = (int)(i % w);
      if (x >= 1 && x <= w - 2 && y >= 1 && y <= h - 2) found = sift_candidate(a, k, s, x, y, kp);
    }
    long long total;
    const long long before = block_exclusive_scan<SIFT_THREADS>((long long)(found ? 1 : 0), s_part, total);
    if (WRITE && found) {
      const long long j = at + before;
      if (j < a.kp_cap) {
        a.kp[4 * j] = kp.x; a.kp[4 * j + 1] = kp.y; a.kp[4 * j + 2] = kp.sigma; a.kp[4 * j + 3] = kp.sref;
        a.rec[4 * j] = a.L.first + k; a.rec[4 * j + 1] = s; a.rec[4 * j + 2] = x; a.rec[4 * j + 3] = y;
        a.resp[j] = kp.resp;
      }
    }
    at += total;
  }
  if (!WRITE && threadIdx.x == 0) a.block_count[b] = (int32_t)at;
}

// ---- orientation and descriptor ---------------------------------------------------------------------------------------------------
// the clipped window of half-width R around (xo, yo): samples with all four neighbours inside the level, rows first
struct SiftWindow { int x0, y0, nx; long long n; };
__device__ __forceinline__ SiftWindow sift_window(double xo, double yo, double R, int h, int w) {
  const double lim = 1073741824.0;                 // (int conversions stay defined for any finite keypoint)
  const int xi = (int)floor(min(max(xo, -lim), lim) + 0.5), yi = (int)floor(min(max(yo, -lim), lim) + 0.5);
  const long long r = (long long)min(R, lim);
  const long long x0 = max((long long)xi - r, 1LL), x1 = min((long long)xi + r, (long long)w - 2);
  const long long y0 = max((long long)yi - r, 1LL), y1 = min((long long)yi + r, (long long)h - 2);
  SiftWindow win;
  win.x0 = (int)x0; win.y0 = (int)y0; win.nx = (int)max(x1 - x0 + 1, 0LL);
  win.n = win.nx > 0 && y1 >= y0 ? (long long)win.nx * (y1 - y0 + 1) : 0;
  return win;
}

__device__ __forceinline__ void sift_gradient(const float* L, int w, int px, int py, double& mag, double& ang) {
  const size_t i = (size_t)py * w + px;
  const double gx = 0.5 * ((double)L[i + 1] - (double)L[i - 1]), gy = 0.5 * ((double)L[i + w] - (double)L[i - w]);
  mag = sqrt(gx * gx + gy * gy);
  ang = atan2(gy, gx);
  if (ang < 0.0) ang += SIFT_TWO_PI;
}

// max(0, 1 - |d|) of the circular difference d of two coordinates on a ring of n bins
__device__ __forceinline__ double sift_ring_weight(double d, double n) {
  d = d - n * floor(d / n + 0.5);
  return max(0.0, 1.0 - fabs(d));
}

// one wavefront per keypoint; lanes 0 .. 35 own the bins
__global__ __launch_bounds__(64) void k_sift_orient(const float* __restrict__ pyr, const SiftLayout L, int64_t n_kp, int stride, int upright,
                                                    int max_orient, const double* __restrict__ kp, const int32_t* __restrict__ rec,
                                                    int32_t* __restrict__ n_orient, double* __restrict__ theta) {
  __shared__ double s_v[64], s_f[64], s_hist[36];
  const int lane = threadIdx.x;
  for (int64_t q = blockIdx.x; q < n_kp; q += stride) {
    if (upright) {
      if (lane == 0) { n_orient[q] = 1; theta[4 * q] = 0.0; }
      continue;
    }
    const int o = rec[4 * q], k = o - L.first, h = L.h[k], w = L.w[k];
    const double scale = o < 0 ? 2.0 : 1.0 / (double)(1 << o);
    const double xo = kp[4 * q] * scale, yo = kp[4 * q + 1] * scale, sw = 1.5 * kp[4 * q + 2] * scale;
    const int level = min(max((int)floor(kp[4 * q + 3] + 0.5), 0), L.S + 2);
    const float* G = pyr + L.off[k] + (size_t)level * h * w;
    const double R = floor(3.0 * sw);
    const SiftWindow win = sift_window(xo, yo, R, h, w);
    double acc = 0.0;
    for (long long base = 0; base < win.n; base += 64) {
      const long long i = base + lane;
      double v = 0.0, f = 0.0;
      if (i < win.n) {
        const int px = win.x0 + (int)(i % win.nx), py = win.y0 + (int)(i / win.nx);
        const double dx = (double)px - xo, dy = (double)py - yo, d2 = dx * dx + dy * dy;
        if (d2 < R * R + 0.5) {
          double mag, ang;
          sift_gradient(G, w, px, py, mag, ang);
          v = mag * exp(-d2 / (2.0 * sw * sw));
          f = 36.0 * ang / SIFT_TWO_PI - 0.5;
        }
      }
      __syncthreads();                          // (the gather of the chunk before is over)
      s_v[lane] = v; s_f[lane] = f;
      __syncthreads();
      if (lane < 36)
        for (int j = 0; j < 64; ++j) acc += s_v[j] * sift_ring_weight(s_f[j] - (double)lane, 36.0);
    }
    __syncthreads();
    if (lane < 36) s_hist[lane] = acc;
    __syncthreads();
    if (lane == 0) {
      double hist[36], tmp[36];
      for (int i = 0; i < 36; ++i) hist[i] = s_hist[i];
      for (int pass = 0; pass < 6; ++pass) {
        for (int i = 0; i < 36; ++i) tmp[i] = (hist[(i + 35) % 36] + hist[i] + hist[(i + 1) % 36]) / 3.0;
        for (int i = 0; i < 36; ++i) hist[i] = tmp[i];
      }
      double top = 0.0;
      for (int i = 0; i < 36; ++i) top = max(top, hist[i]);
      // the peaks by (height descending, bin ascending): an insertion into at most four places
      double ph[4], pt[4];
      int np = 0;
      for (int i = 0; i < 36; ++i) {
        const double h0 = hist[i], hm = hist[(i + 35) % 36], hp = hist[(i + 1) % 36];
        if (!(h0 > hm && h0 > hp && h0 >= 0.8 * top)) continue;
        const double di = -0.5 * (hp - hm) / (hp + hm - 2.0 * h0);
        const double th = SIFT_TWO_PI * ((double)i + di + 0.5) / 36.0;
        int at = np;
        while (at > 0 && ph[at - 1] < h0) --at;
        if (at >= max_orient) continue;
        for (int j = min(np, max_orient - 1); j > at; --j) { ph[j] = ph[j - 1]; pt[j] = pt[j - 1]; }
        ph[at] = h0; pt[at] = th;
        if (np < max_orient) ++np;
      }
      n_orient[q] = np;
      for (int j = 0; j < np; ++j) theta[4 * q + j] = pt[j];
    }
  }
}

__global__ __launch_bounds__(SIFT_THREADS) void k_sift_emit(int64_t n_kp, int stride, int64_t capacity, const double* __restrict__ kp,
                                                            const int32_t* __restrict__ rec, const double* __restrict__ resp,
                                                            const int32_t* __restrict__ n_orient, const double* __restrict__ theta,
                                                            const int64_t* __restrict__ feat_off, double* __restrict__ out_kp,
                                                            int32_t* __restrict__ out_rec, float* __restrict__ out_resp) {
  for (int64_t q = (int64_t)blockIdx.x * SIFT_THREADS + threadIdx.x; q < n_kp; q += (int64_t)stride * SIFT_THREADS)
    for (int j = 0; j < n_orient[q]; ++j) {
      const int64_t f = feat_off[q] + j;
      if (f >= capacity) break;
      out_kp[4 * f] = kp[4 * q]; out_kp[4 * f + 1] = kp[4 * q + 1]; out_kp[4 * f + 2] = kp[4 * q + 2]; out_kp[4 * f + 3] = theta[4 * q + j];
      for (int c = 0; c < 4; ++c) out_rec[4 * f + c] = rec[4 * q + c];
      out_resp[f] = (float)resp[q];
    }
}

// rows index[i] (or i) of the detector's output, split into the arrays the bindings return; a row whose index is out of range is skipped
__global__ __launch_bounds__(SIFT_THREADS) void k_sift_gather(int64_t n, int stride, int64_t n_in, const int64_t* __restrict__ index,
                                                              const double* __restrict__ kp, const float* __restrict__ resp, double offset,
                                                              double* __restrict__ out_kp, double* __restrict__ xy, double* __restrict__ scales,
                                                              double* __restrict__ orient, float* __restrict__ scores) {
  for (int64_t i = (int64_t)blockIdx.x * SIFT_THREADS + threadIdx.x; i < n; i += (int64_t)stride * SIFT_THREADS) {
    const int64_t j = index ? index[i] : i;
    if (j < 0 || j >= n_in) continue;
    if (out_kp) for (int c = 0; c < 4; ++c) out_kp[4 * i + c] = kp[4 * j + c];
    if (xy) { xy[2 * i] = kp[4 * j] + offset; xy[2 * i + 1] = kp[4 * j + 1] + offset; }
    if (scales) scales[i] = kp[4 * j + 2];
    if (orient) orient[i] = kp[4 * j + 3];
    if (scores && resp) scores[i] = resp[j];
  }
}

// the sum of the 128 values of s_h in index order, on every lane
__device__ __forceinline__ double sift_sum128(const double* s_h, bool squared) {
  double sum = 0.0;
  for (int i = 0; i < 128; ++i) sum += squared ? s_h[i] * s_h[i] : s_h[i];
  return sum;
}

// 128 lanes per feature; lane = by * 32 + bx * 8 + bo owns that bin
__global__ __launch_bounds__(128) void k_sift_describe(const float* __restrict__ pyr, const SiftLayout L, int64_t n, int stride, double sigma0,
                                                       double magnif, double clip, int l1_root, const double* __restrict__ kp,
                                                       float* __restrict__ desc, uint8_t* __restrict__ valid) {
  __shared__ double s_v[128], s_x[128], s_y[128], s_t[128], s_h[128];
  const int lane = threadIdx.x;
  const double bo = (double)(lane & 7), bx = (double)((lane >> 3) & 3), by = (double)(lane >> 5);
  for (int64_t q = blockIdx.x; q < n; q += stride) {
    const double x = kp[4 * q], y = kp[4 * q + 1], sigma = kp[4 * q + 2], theta = kp[4 * q + 3];
    bool ok = isfinite(x) && isfinite(y) && isfinite(sigma) && isfinite(theta) && sigma > 0.0;
    int k = 0, level = 0, o = 0;
    if (ok) {
      const double t = (double)L.S * log2(sigma / sigma0);
      const double fo = min(max(floor((t - 0.5) / (double)L.S), (double)L.first), (double)(L.first + L.n_oct - 1));
      const double fl = floor(t - fo * (double)L.S + 0.5);
      ok = L.n_oct > 0 && fl >= 0.0 && fl <= (double)(L.S + 2);
      if (ok) { o = (int)fo; k = o - L.first; level = (int)fl; }
    }
    double acc = 0.0;
    if (ok) {                                     // (uniform: it depends on the keypoint alone)
      const int h = L.h[k], w = L.w[k];
      const double scale = o < 0 ? 2.0 : 1.0 / (double)(1 << o);
      const double xo = x * scale, yo = y * scale, sbp = magnif * sigma * scale;
      const float* G = pyr + L.off[k] + (size_t)level * h * w;
      const SiftWindow win = sift_window(xo, yo, floor(sqrt(2.0) * sbp * 2.5 + 0.5), h, w);
      const double ct = cos(theta), st = sin(theta);
      for (long long base = 0; base < win.n; base += 128) {
        const long long i = base + lane;
        double v = 0.0, fx = 0.0, fy = 0.0, ft = 0.0;
        if (i < win.n) {
          const int px = win.x0 + (int)(i % win.nx), py = win.y0 + (int)(i / win.nx);
          const double dx = (double)px - xo, dy = (double)py - yo;
          double mag, ang;
          sift_gradient(G, w, px, py, mag, ang);
          const double nx = (ct * dx + st * dy) / sbp, ny = (-st * dx + ct * dy) / sbp;
          double rel = ang - theta;
          rel = rel - SIFT_TWO_PI * floor(rel / SIFT_TWO_PI);
          ft = 8.0 * rel / SIFT_TWO_PI;
          v = mag * exp(-(nx * nx + ny * ny) / 8.0);
          fx = nx + 1.5; fy = ny + 1.5;
        }
        __syncthreads();                        // (the gather of the chunk before is over)
        s_v[lane] = v; s_x[lane] = fx; s_y[lane] = fy; s_t[lane] = ft;
        __syncthreads();
        for (int j = 0; j < 128; ++j) {
          const double wxy = max(0.0, 1.0 - fabs(s_x[j] - bx)) * max(0.0, 1.0 - fabs(s_y[j] - by));
          if (wxy > 0.0 && s_v[j] != 0.0) acc += s_v[j] * wxy * sift_ring_weight(s_t[j] - bo, 8.0);
        }
      }
    }
    __syncthreads();
    s_h[lane] = acc;
    __syncthreads();
    const double n1 = sqrt(sift_sum128(s_h, true));
    ok = ok && n1 > 0.0;
    double v = 0.0;
    if (ok) {
      v = min(acc / n1, clip);
      __syncthreads();
      s_h[lane] = v;
      __syncthreads();
      v = v / sqrt(sift_sum128(s_h, true));
      if (l1_root) {
        __syncthreads();
        s_h[lane] = v;
        __syncthreads();
        v = sqrt(v / sift_sum128(s_h, false));
      }
    }
    desc[128 * q + lane] = (float)v;
    if (lane == 0) valid[q] = ok ? 1 : 0;
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
static double sift_peak(const pxr_sift_options* o) { return o->peak_threshold < 0.0 ? 0.02 / (double)o->octave_resolution : o->peak_threshold; }

// the options and the size, validated; the layout they give
static int sift_layout(const char* fn, int h, int w, const pxr_sift_options* o, SiftLayout* L) {
  PXR_REQUIRE(o, "%s: NULL options", fn);
  PXR_REQUIRE(h >= 1 && w >= 1, "%s: image size %d x %d is not positive", fn, h, w);
  PXR_REQUIRE(h <= (1 << 14) && w <= (1 << 14), "%s: image size %d x %d above 16384", fn, h, w);
  PXR_REQUIRE(o->first_octave == -1 || o->first_octave == 0, "%s: first_octave = %d outside {-1, 0}", fn, (int)o->first_octave);
  PXR_REQUIRE(o->octave_resolution >= 2 && o->octave_resolution <= 4, "%s: octave_resolution = %d outside {2, 3, 4}", fn, (int)o->octave_resolution);
  PXR_REQUIRE(std::isfinite(o->sigma0) && std::isfinite(o->sigma_in) && o->sigma_in >= 0.0 &&
              o->sigma0 > o->sigma_in * (o->first_octave < 0 ? 2.0 : 1.0), "%s: sigma0 = %g is not above sigma_in 2^-first_octave = %g", fn,
              o->sigma0, o->sigma_in * (o->first_octave < 0 ? 2.0 : 1.0));
  PXR_REQUIRE(o->max_num_orientations >= 1 && o->max_num_orientations <= 4, "%s: max_num_orientations = %d outside [1, 4]", fn,
              (int)o->max_num_orientations);
  PXR_REQUIRE(o->max_refine_steps >= 0 && o->max_refine_steps <= 16, "%s: max_refine_steps = %d outside [0, 16]", fn, (int)o->max_refine_steps);
  PXR_REQUIRE(o->normalization == 0 || o->normalization == 1, "%s: normalization = %d outside {0, 1}", fn, (int)o->normalization);
  PXR_REQUIRE(o->edge_threshold > 0.0 && o->magnif > 0.0 && o->clip > 0.0 && std::isfinite(o->edge_threshold) && std::isfinite(o->magnif) &&
              std::isfinite(o->clip) && std::isfinite(o->peak_threshold), "%s: edge_threshold, magnif and clip must be positive and finite", fn);
  L->S = o->octave_resolution; L->first = o->first_octave; L->n_oct = 0; L->total = 0;
  int ho = o->first_octave < 0 ? 2 * h : h, wo = o->first_octave < 0 ? 2 * w : w;
  while (std::min(ho, wo) >= SIFT_MIN_SIDE && L->n_oct < SIFT_MAX_OCTAVES) {
    L->h[L->n_oct] = ho; L->w[L->n_oct] = wo; L->off[L->n_oct] = L->total;
    L->total += (int64_t)(L->S + 3) * ho * wo;
    ++L->n_oct;
    ho = (ho + 1) / 2; wo = (wo + 1) / 2;
  }
  PXR_REQUIRE(o->num_octaves >= 0 && o->num_octaves <= L->n_oct, "%s: num_octaves = %d outside [0, %d] (octaves while the smaller side is >= %d, at most %d)",
              fn, (int)o->num_octaves, L->n_oct, SIFT_MIN_SIDE, SIFT_MAX_OCTAVES);
  if (o->num_octaves > 0) {
    L->n_oct = o->num_octaves;
    L->total = L->off[L->n_oct - 1] + (int64_t)(L->S + 3) * L->h[L->n_oct - 1] * L->w[L->n_oct - 1];
  }
  for (int k = L->n_oct; k < SIFT_MAX_OCTAVES; ++k) { L->h[k] = L->w[k] = 0; L->off[k] = L->total; }
  return PXR_OK;
}

// the taps of a blur by sigma: radius int(4 sigma + 0.5), normalised in float64 (summed in ascending order), rounded to float32
static int sift_taps(const char* fn, double sigma, SiftTaps* t) {
  const int r = (int)(4.0 * sigma + 0.5);
  PXR_REQUIRE(r <= SIFT_MAX_R, "%s: a blur by sigma = %g needs radius %d above %d", fn, sigma, r, SIFT_MAX_R);
  double w[2 * SIFT_MAX_R + 1], sum = 0.0;
  for (int k = 0; k <= 2 * r; ++k) { const double x = (double)(k - r); w[k] = std::exp(-x * x / (2.0 * sigma * sigma)); sum += w[k]; }
  t->r = r;
  for (int k = 0; k <= 2 * SIFT_MAX_R; ++k) t->w[k] = k <= 2 * r ? (float)(w[k] / sum) : 0.f;
  return PXR_OK;
}

static void sift_blur(hipStream_t st, const float* src, float* tmp, float* dst, int h, int w, const SiftTaps& t) {
  const unsigned tiles_x = (unsigned)((w + 63) / 64);
  hipLaunchKernelGGL(k_sift_blur<0>, dim3(tiles_x * (unsigned)((h + SIFT_ROW_TILE - 1) / SIFT_ROW_TILE)), dim3(SIFT_THREADS), 0, st, src, tmp, h, w, t);
  hipLaunchKernelGGL(k_sift_blur<1>, dim3(tiles_x * (unsigned)((h + SIFT_COL_TILE - 1) / SIFT_COL_TILE)), dim3(SIFT_THREADS), 0, st, (const float*)tmp, dst, h, w, t);
}

static int sift_pyramid(pxr_ctx* ctx, const void* d_image, int dtype, int h, int w, const pxr_sift_options* o, float* d_pyramid, double* h_ms) {
  const char* fn = "pxr_sift_pyramid";
  PXR_REQUIRE(ctx && d_image && d_pyramid, "%s: NULL argument", fn);
  PXR_REQUIRE(dtype == PXR_U8 || dtype == PXR_F32, "%s: image dtype %d is neither PXR_U8 nor PXR_F32", fn, dtype);
  SiftLayout L;
  if (int rc = sift_layout(fn, h, w, o, &L)) return rc;
  const int S = L.S;
  SiftTaps first, inc[6];
  const double in = o->sigma_in * (o->first_octave < 0 ? 2.0 : 1.0);
  if (int rc = sift_taps(fn, std::sqrt(o->sigma0 * o->sigma0 - in * in), &first)) return rc;
  for (int s = 1; s <= S + 2; ++s)
    if (int rc = sift_taps(fn, o->sigma0 * std::sqrt(std::pow(2.0, 2.0 * s / S) - std::pow(2.0, 2.0 * (s - 1) / S)), &inc[s - 1])) return rc;
  if (h_ms) h_ms[0] = 0.0;
  if (L.n_oct == 0) return PXR_OK;
  PXR_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int64_t n0 = (int64_t)L.h[0] * L.w[0];
  float *img, *tmp;
  Workspace ws;
  ws.take(img, (size_t)n0); ws.take(tmp, (size_t)n0);
  if (int rc = ws.commit(ctx)) return rc;
  StageTimer<2> timer(st, h_ms);
  if (int rc = timer.create(fn)) return rc;
  timer.mark(0);
  hipLaunchKernelGGL(k_sift_upsample, blocks_for(n0, SIFT_THREADS), dim3(SIFT_THREADS), 0, st, d_image, dtype, h, w, o->first_octave < 0 ? 1 : 0, img);
  for (int k = 0; k < L.n_oct; ++k) {
    const int ho = L.h[k], wo = L.w[k];
    const size_t plane = (size_t)ho * wo;
    float* G = d_pyramid + L.off[k];
    if (k == 0) sift_blur(st, img, tmp, G, ho, wo, first);
    else hipLaunchKernelGGL(k_sift_half, blocks_for((int64_t)plane, SIFT_THREADS), dim3(SIFT_THREADS), 0, st,
                            (const float*)(d_pyramid + L.off[k - 1] + (size_t)S * L.h[k - 1] * L.w[k - 1]), L.w[k - 1], G, ho, wo);
    for (int s = 1; s <= S + 2; ++s) sift_blur(st, G + (size_t)(s - 1) * plane, tmp, G + (size_t)s * plane, ho, wo, inc[s - 1]);
  }
  timer.mark(1);
  if (int rc = hip_check(hipGetLastError(), "k_sift_blur launch")) return rc;
  const int from[1] = {0};
  return timer.read(from, 1);
}

static int sift_detect(pxr_ctx* ctx, const float* d_pyramid, int h, int w, const pxr_sift_options* o, int64_t capacity, double* d_keypoints,
                       int32_t* d_record, float* d_response, int64_t* h_n_found, double* h_ms) {
  const char* fn = "pxr_sift_detect";
  PXR_REQUIRE(ctx && d_pyramid && h_n_found, "%s: NULL argument", fn);
  PXR_REQUIRE(capacity >= 0, "%s: capacity = %lld is negative", fn, (long long)capacity);
  PXR_REQUIRE(capacity == 0 || (d_keypoints && d_record && d_response), "%s: NULL output array", fn);
  SiftDetect a;
  if (int rc = sift_layout(fn, h, w, o, &a.L)) return rc;
  if (h_ms) for (int k = 0; k < 5; ++k) h_ms[k] = 0.0;
  if (a.L.n_oct == 0) { *h_n_found = 0; return PXR_OK; }
  a.pyr = d_pyramid; a.peak = sift_peak(o); a.edge_bound = (o->edge_threshold + 1.0) * (o->edge_threshold + 1.0) / o->edge_threshold;
  a.sigma0 = o->sigma0; a.max_steps = o->max_refine_steps; a.n_planes = 0;
  int64_t n_blocks = 0;
  for (int k = 0; k < a.L.n_oct; ++k)
    for (int s = 1; s <= a.L.S; ++s) {
      a.plane_k[a.n_planes] = k; a.plane_s[a.n_planes] = s; a.plane_first[a.n_planes++] = (int)n_blocks;
      n_blocks += ((int64_t)a.L.h[k] * a.L.w[k] + SIFT_BLOCK_SAMPLES - 1) / SIFT_BLOCK_SAMPLES;
    }
  for (int p = a.n_planes; p <= SIFT_MAX_PLANES; ++p) a.plane_first[p] = (int)n_blocks;
  for (int p = a.n_planes; p < SIFT_MAX_PLANES; ++p) a.plane_k[p] = a.plane_s[p] = 0;
  PXR_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  StageTimer<6> timer(st, h_ms);                        // count | scan | write | orient | scan + emit
  if (int rc = timer.create(fn)) return rc;

  // The keypoints are staged in the workspace, whose size must be known before the count is: a first guess, and when the count
  // exceeds it the workspace grows (which loses its contents) and count and scan run again.
  int64_t kp_cap = std::max<int64_t>(capacity, 4096), n_kp = 0;
  int64_t *block_off, *feat_off; int32_t* n_orient; double* theta;
  for (int attempt = 0;; ++attempt) {
    Workspace ws;                                       // (a second attempt lays out again: no pointer of the first is kept)
    ws.take(a.block_count, (size_t)n_blocks); ws.take(block_off, (size_t)n_blocks + 1);
    ws.take(a.kp, (size_t)kp_cap * 4); ws.take(a.rec, (size_t)kp_cap * 4); ws.take(a.resp, (size_t)kp_cap);
    ws.take(n_orient, (size_t)kp_cap); ws.take(theta, (size_t)kp_cap * 4); ws.take(feat_off, (size_t)kp_cap + 1);
    if (int rc = ws.commit(ctx)) return rc;
    a.block_off = block_off; a.kp_cap = kp_cap;
    timer.mark(0);
    hipLaunchKernelGGL(k_sift_detect<false>, dim3((unsigned)n_blocks), dim3(SIFT_THREADS), 0, st, a);
    timer.mark(1);
    hipLaunchKernelGGL((k_exclusive_scan<SIFT_THREADS, int32_t, int64_t>), dim3(1), dim3(SIFT_THREADS), 0, st, n_blocks, (const int32_t*)a.block_count,
                       block_off, 1);
    timer.mark(2);
    if (int rc = hip_check(hipGetLastError(), "k_sift_detect launch")) return rc;
    PXR_HIP(hipMemcpyAsync(&n_kp, a.block_off + n_blocks, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    PXR_HIP(hipStreamSynchronize(st));
    if (n_kp <= kp_cap) break;
    PXR_REQUIRE(attempt == 0, "%s: the number of keypoints changed between two counts", fn);
    kp_cap = n_kp;
  }
  int64_t total = 0;
  if (n_kp > 0) {
    hipLaunchKernelGGL(k_sift_detect<true>, dim3((unsigned)n_blocks), dim3(SIFT_THREADS), 0, st, a);
    timer.mark(3);
    const int grid = (int)std::min<int64_t>(n_kp, SIFT_MAX_GRID);
    hipLaunchKernelGGL(k_sift_orient, dim3((unsigned)grid), dim3(64), 0, st, d_pyramid, a.L, n_kp, grid, o->upright ? 1 : 0,
                       (int)o->max_num_orientations, (const double*)a.kp, (const int32_t*)a.rec, n_orient, theta);
    timer.mark(4);
    hipLaunchKernelGGL((k_exclusive_scan<SIFT_THREADS, int32_t, int64_t>), dim3(1), dim3(SIFT_THREADS), 0, st, n_kp, (const int32_t*)n_orient, feat_off, 1);
    const int egrid = (int)std::min<int64_t>(blocks_for(n_kp, SIFT_THREADS).x, SIFT_MAX_GRID);
    if (capacity > 0)
      hipLaunchKernelGGL(k_sift_emit, dim3((unsigned)egrid), dim3(SIFT_THREADS), 0, st, n_kp, egrid, capacity, (const double*)a.kp,
                         (const int32_t*)a.rec, (const double*)a.resp, (const int32_t*)n_orient, (const double*)theta,
                         (const int64_t*)feat_off, d_keypoints, d_record, d_response);
    timer.mark(5);
    if (int rc = hip_check(hipGetLastError(), "k_sift_orient launch")) return rc;
    PXR_HIP(hipMemcpyAsync(&total, feat_off + n_kp, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    PXR_HIP(hipStreamSynchronize(st));
  } else {
    timer.mark(3); timer.mark(4); timer.mark(5);
  }
  *h_n_found = total;
  const int from[5] = {0, 1, 2, 3, 4};
  return timer.read(from, 5);
}

static int sift_describe(pxr_ctx* ctx, const float* d_pyramid, int h, int w, const pxr_sift_options* o, int64_t n, const double* d_keypoints,
                         float* d_descriptors, uint8_t* d_valid, double* h_ms) {
  const char* fn = "pxr_sift_describe";
  PXR_REQUIRE(ctx && d_pyramid, "%s: NULL argument", fn);
  PXR_REQUIRE(n >= 0, "%s: n = %lld is negative", fn, (long long)n);
  PXR_REQUIRE(n == 0 || (d_keypoints && d_descriptors && d_valid), "%s: NULL keypoint / output array", fn);
  SiftLayout L;
  if (int rc = sift_layout(fn, h, w, o, &L)) return rc;
  if (h_ms) h_ms[0] = 0.0;
  if (n == 0) return PXR_OK;
  PXR_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  StageTimer<2> timer(st, h_ms);
  if (int rc = timer.create(fn)) return rc;
  timer.mark(0);
  const int grid = (int)std::min<int64_t>(n, SIFT_MAX_GRID);
  hipLaunchKernelGGL(k_sift_describe, dim3((unsigned)grid), dim3(128), 0, st, d_pyramid, L, n, grid, o->sigma0, o->magnif, o->clip,
                     o->normalization == 1 ? 1 : 0, d_keypoints, d_descriptors, d_valid);
  timer.mark(1);
  if (int rc = hip_check(hipGetLastError(), "k_sift_describe launch")) return rc;
  const int from[1] = {0};
  return timer.read(from, 1);
}

}  // namespace pxr

extern "C" void pxr_sift_default_options(pxr_sift_options* o) {
  if (!o) return;
  o->first_octave = -1; o->num_octaves = 0; o->octave_resolution = 3; o->max_refine_steps = 5; o->max_num_orientations = 2;
  o->upright = 0; o->normalization = 1; o->reserved = 0;
  o->sigma0 = 1.6; o->sigma_in = 0.5; o->peak_threshold = -1.0; o->edge_threshold = 10.0; o->magnif = 3.0; o->clip = 0.2;
}

extern "C" int pxr_sift_pyramid_layout(int h, int w, const pxr_sift_options* options, int32_t* h_n_octaves, int32_t* h_sizes, int64_t* h_offsets) {
  PXR_REQUIRE(h_n_octaves && h_sizes && h_offsets, "pxr_sift_pyramid_layout: NULL argument");
  pxr::SiftLayout L;
  if (int rc = pxr::sift_layout("pxr_sift_pyramid_layout", h, w, options, &L)) return rc;
  *h_n_octaves = L.n_oct;
  for (int k = 0; k < pxr::SIFT_MAX_OCTAVES; ++k) { h_sizes[2 * k] = L.h[k]; h_sizes[2 * k + 1] = L.w[k]; h_offsets[k] = L.off[k]; }
  return PXR_OK;
}

extern "C" int pxr_sift_pyramid_bytes(int h, int w, const pxr_sift_options* options, int64_t* h_bytes) {
  PXR_REQUIRE(h_bytes, "pxr_sift_pyramid_bytes: NULL argument");
  pxr::SiftLayout L;
  if (int rc = pxr::sift_layout("pxr_sift_pyramid_bytes", h, w, options, &L)) return rc;
  *h_bytes = L.total * 4;
  return PXR_OK;
}

extern "C" int pxr_sift_pyramid(pxr_ctx* ctx, const void* d_image, int image_dtype, int h, int w, const pxr_sift_options* options, float* d_pyramid) {
  return pxr::sift_pyramid(ctx, d_image, image_dtype, h, w, options, d_pyramid, nullptr);
}
extern "C" int pxr_sift_pyramid_timed(pxr_ctx* ctx, const void* d_image, int image_dtype, int h, int w, const pxr_sift_options* options,
                                      float* d_pyramid, double* h_kernel_ms) {
  PXR_REQUIRE(h_kernel_ms, "pxr_sift_pyramid_timed: NULL h_kernel_ms");
  return pxr::sift_pyramid(ctx, d_image, image_dtype, h, w, options, d_pyramid, h_kernel_ms);
}

extern "C" int pxr_sift_detect(pxr_ctx* ctx, const float* d_pyramid, int h, int w, const pxr_sift_options* options, int64_t capacity,
                               double* d_keypoints, int32_t* d_record, float* d_response, int64_t* h_n_found) {
  return pxr::sift_detect(ctx, d_pyramid, h, w, options, capacity, d_keypoints, d_record, d_response, h_n_found, nullptr);
}
extern "C" int pxr_sift_detect_timed(pxr_ctx* ctx, const float* d_pyramid, int h, int w, const pxr_sift_options* options, int64_t capacity,
                                     double* d_keypoints, int32_t* d_record, float* d_response, int64_t* h_n_found, double* h_kernel_ms) {
  PXR_REQUIRE(h_kernel_ms, "pxr_sift_detect_timed: NULL h_kernel_ms");
  return pxr::sift_detect(ctx, d_pyramid, h, w, options, capacity, d_keypoints, d_record, d_response, h_n_found, h_kernel_ms);
}

extern "C" int pxr_sift_gather(pxr_ctx* ctx, int64_t n, int64_t n_in, const int64_t* d_index, const double* d_keypoints, const float* d_response,
                              double offset, double* d_keypoints_out, double* d_xy, double* d_scales, double* d_orientations, float* d_scores) {
  PXR_REQUIRE(ctx, "pxr_sift_gather: NULL context");
  PXR_REQUIRE(n >= 0 && n_in >= 0, "pxr_sift_gather: negative size");
  PXR_REQUIRE(n == 0 || d_keypoints, "pxr_sift_gather: NULL keypoints");
  PXR_REQUIRE(std::isfinite(offset), "pxr_sift_gather: offset is not finite");
  if (n == 0) return PXR_OK;
  PXR_HIP(hipSetDevice(ctx->device));
  const int grid = (int)std::min<int64_t>(pxr::blocks_for(n, pxr::SIFT_THREADS).x, pxr::SIFT_MAX_GRID);
  hipLaunchKernelGGL(pxr::k_sift_gather, dim3((unsigned)grid), dim3(pxr::SIFT_THREADS), 0, ctx->stream, n, grid, n_in, d_index, d_keypoints, d_response,
                     offset, d_keypoints_out, d_xy, d_scales, d_orientations, d_scores);
  return pxr::hip_check(hipGetLastError(), "k_sift_gather launch");
}

extern "C" int pxr_sift_describe(pxr_ctx* ctx, const float* d_pyramid, int h, int w, const pxr_sift_options* options, int64_t n,
                                 const double* d_keypoints, float* d_descriptors, uint8_t* d_valid) {
  return pxr::sift_describe(ctx, d_pyramid, h, w, options, n, d_keypoints, d_descriptors, d_valid, nullptr);
}
extern "C" int pxr_sift_describe_timed(pxr_ctx* ctx, const float* d_pyramid, int h, int w, const pxr_sift_options* options, int64_t n,
                                       const double* d_keypoints, float* d_descriptors, uint8_t* d_valid, double* h_kernel_ms) {
  PXR_REQUIRE(h_kernel_ms, "pxr_sift_describe_timed: NULL h_kernel_ms");
  return pxr::sift_describe(ctx, d_pyramid, h, w, options, n, d_keypoints, d_descriptors, d_valid, h_kernel_ms);
}
