// pxr_dsift.h -- device helpers of the dense-SIFT producer (pxr_dsift.hip).
//
// The descriptor is the reference's weight-free `dsift` model (pixsfm/features/models/dsift.py: kornia's
// DenseSIFTDescriptor(num_ang_bins=8, num_spatial_bins=4, spatial_bin_size=s, rootsift, clipval, stride=1, padding=1) on
// the grey image).  Definition, as restated in DESIGN.md §16:
//   1. gx = 0.5 I(y, x+1) - 0.5 I(y, x-1), gy likewise (indices clamped into the image)
//   2. mag = sqrt(gx^2 + gy^2 + 1e-10), o = 8 (atan2(gy, gx + 1e-10) + 2 pi) / (2 pi), f = floor(o), w1 = o - f:
//      angle map A_{f mod 8} += (1 - w1) mag, A_{(f+1) mod 8} += w1 mag; A is zero outside the image
//   3. P_a(j, i) = sum_{u,v < s} k(u) k(v) A_a(j + u - s/2, i + v - s/2), 0 <= j <= h, 0 <= i <= w (zero elsewhere),
//      k(i) = (s/2 - |i + 0.5 - s/2|) / (s/2)
//   4. D_c(y, x) = P_a(y + sy - 1, x + sx - 1), c = 16 a + 4 sy + sx
//   5. per pixel: L2 normalise, clamp to [0, clipval], L2 normalise, rootsift: sqrt(n / |n|_1 + 1e-10)
//
// Both kernels -- the dense map and the fused arena producer -- compute a TILE of at most 16 x 16 output texels with
// ds_tile() and then every texel with ds_texel(): one code path with a fixed summation order, so that the fused arena equals
// "dense map -> pxr_arena_extract" bit for bit (the library is built with -ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>

namespace pxr {

constexpr int DS_T = 16;                  // output tile side (the largest patch)
constexpr int DS_SMAX = 8;                // largest spatial bin size
constexpr int DS_NI = DS_T + DS_SMAX + 4; // grey window side: the tile, the 4 x 4 gather (+3), the bin pooling (s - 1), the gradient (+2)
constexpr int DS_NA = DS_T + DS_SMAX + 2; // angle-map window side
constexpr int DS_NP = DS_T + 3;           // pooled-map window side
constexpr int DS_STAGE = 17;              // row stride of the dense kernel's output staging (channel-major, +1 against conflicts)

struct DsSmem {
  union {
    struct {
      float img[DS_NI * DS_NI];           // grey values, coordinates clamped into the image (replicate border of the gradient)
      float w0[DS_NA * DS_NA];            // (1 - w1) mag, to bin b0
      float w1[DS_NA * DS_NA];            // w1 mag, to bin (b0 + 1) mod 8
      int b0[DS_NA * DS_NA];
    } a;
    float P[8 * DS_NP * DS_NP];           // pooled maps (written once the angle maps are consumed)
  } u;
  union {
    float H[8 * DS_NA * DS_NP];           // horizontal pass of the bin pooling
    float stage[128 * DS_STAGE];          // dense kernel: one output row, channel-major (after H is consumed)
  } v;
};

__device__ __forceinline__ float ds_load(const unsigned char* p, size_t i) { return (float)p[i] / 255.0f; }  // to_tensor
__device__ __forceinline__ float ds_load(const float* p, size_t i) { return p[i]; }

// k(i) of the bin pooling kernel (kornia get_sift_pooling_kernel, separated)
__device__ __forceinline__ float ds_pool_weight(int i, int s) {
  const float hs = 0.5f * (float)s;
  return (hs - fabsf((float)i + 0.5f - hs)) / hs;
}

// Fills sm.u.P for the tile whose first output texel is (x0, y0): P window origin (x0 - 1, y0 - 1), (T + 3)^2 texels x 8 bins.
// All threads of the block take part (barriers inside).  Image reads are clamped: any (x0, y0) is safe.
template <typename SRC>
__device__ void ds_tile(const SRC* __restrict__ img, int h, int w, int x0, int y0, int T, int s, DsSmem& sm) {
  const int tid = threadIdx.x, nt = blockDim.x, hs = s / 2;
  const int NI = T + s + 4, NA = T + s + 2, NP = T + 3;
  const int iy0 = y0 - 2 - hs, ix0 = x0 - 2 - hs;            // grey window origin; the angle window starts one texel later
  for (int t = tid; t < NI * NI; t += nt) {
    const int r = t / NI, c = t - r * NI;
    const int yy = min(max(iy0 + r, 0), h - 1), xx = min(max(ix0 + c, 0), w - 1);
    sm.u.a.img[r * DS_NI + c] = ds_load(img, (size_t)yy * w + xx);
  }
  __syncthreads();
  for (int t = tid; t < NA * NA; t += nt) {
    const int r = t / NA, c = t - r * NA;
    const int y = iy0 + 1 + r, x = ix0 + 1 + c;
    float a0 = 0.f, a1 = 0.f;
    int b = 0;
    if (y >= 0 && y < h && x >= 0 && x < w) {
      const float* p = sm.u.a.img + (r + 1) * DS_NI + (c + 1);
      const float gx = 0.5f * p[1] - 0.5f * p[-1];
      const float gy = 0.5f * p[DS_NI] - 0.5f * p[-DS_NI];
      const float mag = sqrtf(gx * gx + gy * gy + 1e-10f);
      const float twopi = 6.28318530717958647692f;
      const float th = atan2f(gy, gx + 1e-10f) + twopi;
      const float o = 8.0f * th / twopi;
      const float f = floorf(o);
      const float wo1 = o - f;
      b = ((int)f) & 7;                                          // o in [4, 12]: f >= 0 (only ever compared, never an index)
      a0 = (1.0f - wo1) * mag;
      a1 = wo1 * mag;
    }
    sm.u.a.w0[r * DS_NA + c] = a0;
    sm.u.a.w1[r * DS_NA + c] = a1;
    sm.u.a.b0[r * DS_NA + c] = b;
  }
  __syncthreads();
  // horizontal pass: H_a(r, i) = sum_v k(v) A_a(r, i + v), v = 0 .. s-1 in order
  for (int t = tid; t < NA * NP; t += nt) {
    const int r = t / NP, i = t - r * NP;
    float acc[8];
#pragma unroll
    for (int a = 0; a < 8; ++a) acc[a] = 0.f;
    for (int v = 0; v < s; ++v) {
      const int q = r * DS_NA + i + v;
      const float kv = ds_pool_weight(v, s), a0 = sm.u.a.w0[q], a1 = sm.u.a.w1[q];
      const int b = sm.u.a.b0[q], b1 = (b + 1) & 7;
#pragma unroll
      for (int a = 0; a < 8; ++a) acc[a] = acc[a] + kv * (a == b ? a0 : (a == b1 ? a1 : 0.f));
    }
#pragma unroll
    for (int a = 0; a < 8; ++a) sm.v.H[(a * DS_NA + r) * DS_NP + i] = acc[a];
  }
  __syncthreads();
  // vertical pass: P_a(j, i) = sum_u k(u) H_a(j + u, i), u = 0 .. s-1 in order; zero outside [0, h] x [0, w]
  for (int t = tid; t < NP * NP; t += nt) {
    const int j = t / NP, i = t - j * NP;
    const int py = y0 - 1 + j, px = x0 - 1 + i;
    const bool inside = py >= 0 && py <= h && px >= 0 && px <= w;
    float acc[8];
#pragma unroll
    for (int a = 0; a < 8; ++a) acc[a] = 0.f;
    for (int u = 0; u < s; ++u) {
      const float ku = ds_pool_weight(u, s);
#pragma unroll
      for (int a = 0; a < 8; ++a) acc[a] = acc[a] + ku * sm.v.H[(a * DS_NA + j + u) * DS_NP + i];
    }
#pragma unroll
    for (int a = 0; a < 8; ++a) sm.u.P[(a * DS_NP + j) * DS_NP + i] = inside ? acc[a] : 0.f;
  }
  __syncthreads();
}

// sum over the 16 lanes of a texel group (xor-shuffles 8, 4, 2, 1: extract_kernel's order)
__device__ __forceinline__ float ds_sum16(float v) {
  for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// The descriptor of tile texel (ty, tx): lane `sub` (0 .. 15) of the texel's 16-lane group holds channels 8 sub .. 8 sub + 7
// (a = sub / 2, sy = 2 (sub & 1) + j / 4, sx = j & 3).  Every lane of the wave must call it (shuffles).
__device__ __forceinline__ void ds_texel(const DsSmem& sm, int ty, int tx, int sub, int rootsift, float clipval, float n[8]) {
  const float* P = sm.u.P + ((sub >> 1) * DS_NP + ty + 2 * (sub & 1)) * DS_NP + tx;
#pragma unroll
  for (int j = 0; j < 8; ++j) n[j] = P[(j >> 2) * DS_NP + (j & 3)];
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) ss = fmaf(n[j], n[j], ss);
  float den = fmaxf(sqrtf(ds_sum16(ss)), 1e-12f);
#pragma unroll
  for (int j = 0; j < 8; ++j) n[j] = fminf(fmaxf(n[j] / den, 0.f), clipval);
  ss = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) ss = fmaf(n[j], n[j], ss);
  den = fmaxf(sqrtf(ds_sum16(ss)), 1e-12f);
#pragma unroll
  for (int j = 0; j < 8; ++j) n[j] = n[j] / den;
  if (rootsift) {
    float l1 = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) l1 = l1 + fabsf(n[j]);
    den = fmaxf(ds_sum16(l1), 1e-12f);
#pragma unroll
    for (int j = 0; j < 8; ++j) n[j] = sqrtf(n[j] / den + 1e-10f);
  }
}

}  // namespace pxr
