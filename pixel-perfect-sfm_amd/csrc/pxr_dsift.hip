// pxr_dsift.hip -- dense SIFT (the reference's weight-free `dsift` model) on the GPU.
//
// Reference path: pixsfm/features/models/dsift.py runs kornia's DenseSIFTDescriptor on the grey image and returns a dense
// 128 x h x w fp32 map; FeatureExtractor.tensor_to_fmap (extractor.py:152-199) then L2-normalises it, casts it and keeps the
// ps x ps windows around the keypoints (sparse branch), copying them to the host.  Two kernels here:
//   dsift_dense_kernel    the dense map [128][h][w] fp32 (the model's output; the extractor's dense branch, the equality tests)
//   dsift_extract_kernel  the fused sparse producer: descriptors are computed ONLY on the patch windows, straight into the
//                         arena (corners / scales / L2 normalisation / cast exactly as extract_kernel in pxr_extract.hip):
//                         per keypoint ~0.6 KB of grey pixels in, ps^2 x 128 texels out; the dense map is never formed.
// Both go through ds_tile() / ds_texel() (pxr_dsift.h): the fused arena equals "dense kernel -> pxr_arena_extract" bit for bit.
// One workgroup of 256 threads per 16 x 16 tile / per keypoint; per output row the 16 texels of the row are 16 lane groups of
// 16 lanes, lane `sub` holding channels 8 sub .. 8 sub + 7 (extract_kernel's store mapping: one 16-B store per lane at fp16).
#include <hip/hip_runtime.h>

#include "pxr_dispatch.h"
#include "pxr_dsift.h"
#include "pxr_internal.h"

namespace pxr {

template <typename SRC>
__global__ __launch_bounds__(256) void dsift_dense_kernel(const SRC* __restrict__ img, int h, int w, int s, int rootsift,
                                                          float clipval, float* __restrict__ out) {
  __shared__ DsSmem sm;
  const int x0 = blockIdx.x * DS_T, y0 = blockIdx.y * DS_T;
  ds_tile(img, h, w, x0, y0, DS_T, s, sm);
  const int tid = threadIdx.x, px = tid >> 4, sub = tid & 15;
  const size_t plane = (size_t)h * w;
  const int sx = tid & 15, sc = tid >> 4;        // store mapping: 16 x-contiguous lanes, 16 channels per pass
  for (int ty = 0; ty < DS_T && y0 + ty < h; ++ty) {
    float n[8];
    ds_texel(sm, ty, px, sub, rootsift, clipval, n);
#pragma unroll
    for (int j = 0; j < 8; ++j) sm.v.stage[(sub * 8 + j) * DS_STAGE + px] = n[j];
    __syncthreads();
    if (x0 + sx < w) {
      float* row = out + (size_t)(y0 + ty) * w + x0 + sx;
#pragma unroll
      for (int j = 0; j < 8; ++j) row[(size_t)(sc + 16 * j) * plane] = sm.v.stage[(sc + 16 * j) * DS_STAGE + sx];
    }
    __syncthreads();
  }
}

// corner of keypoint k in map texels: pxr_extract.hip's ex_corner (extractor.py:192-193)
__device__ __forceinline__ void ds_corner(const double* kp, double sx, double sy, int ps, int w, int h, int& x0, int& y0) {
  x0 = (int)fmin(fmax(kp[0] * sx - ps / 2.0, -1.0), (double)w);
  y0 = (int)fmin(fmax(kp[1] * sy - ps / 2.0, -1.0), (double)h);
  x0 = min(max(x0, 0), w - ps - 1);
  y0 = min(max(y0, 0), h - ps - 1);
}

template <typename SRC, typename DST>
__global__ __launch_bounds__(256) void dsift_extract_kernel(const SRC* __restrict__ img, int h, int w, int s, int rootsift,
                                                            float clipval, const double* __restrict__ kps, double sx, double sy,
                                                            int l2_normalize, DST* __restrict__ out, int32_t* __restrict__ corners,
                                                            double* __restrict__ scales, int64_t first, int ps) {
  __shared__ DsSmem sm;
  const int64_t k = blockIdx.x;
  const int tid = threadIdx.x;
  int x0, y0;
  ds_corner(kps + 2 * k, sx, sy, ps, w, h, x0, y0);
  if (tid == 0) {
    corners[2 * (first + k)] = x0; corners[2 * (first + k) + 1] = y0;
    scales[2 * (first + k)] = sx; scales[2 * (first + k) + 1] = sy;
  }
  ds_tile(img, h, w, x0, y0, ps, s, sm);
  DST* patch = out + (size_t)(first + k) * ps * ps * 128;
  const int px = tid >> 4, sub = tid & 15, tx = min(px, ps - 1);
  for (int y = 0; y < ps; ++y) {
    float v[8];
    ds_texel(sm, y, tx, sub, rootsift, clipval, v);
    // the extractor's normalisation in extract_kernel's order: fmaf chain over the lane's 8 channels, xor-shuffles 8, 4, 2, 1
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) ss = fmaf(v[j], v[j], ss);
    if (l2_normalize) {
      ss = ds_sum16(ss);
      const float den = fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = v[j] / den;
    }
    typedef DST vec_t __attribute__((ext_vector_type(8)));
    vec_t o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (DST)v[j];
    if (px < ps) *reinterpret_cast<vec_t*>(patch + ((size_t)y * ps + px) * 128 + sub * 8) = o;
  }
}

static int ds_check(int image_dtype, int h, int w, int s, float clipval, const char* fn) {
  if (image_dtype != PXR_U8 && image_dtype != PXR_F32)
    return set_error(PXR_EUNSUPPORTED, "%s: image dtype %d not supported (PXR_U8 / PXR_F32 grey image)", fn, image_dtype);
  if (s < 2 || s > DS_SMAX || (s & 1))
    return set_error(PXR_EUNSUPPORTED, "%s: spatial_bin_size %d not supported (even, 2 .. %d)", fn, s, DS_SMAX);
  PXR_REQUIRE(h >= 1 && w >= 1, "%s: image %dx%d is empty", fn, h, w);
  PXR_REQUIRE(clipval == clipval, "%s: clipval is NaN", fn);
  return PXR_OK;
}

}  // namespace pxr

extern "C" int pxr_dsift_dense(pxr_ctx* ctx, const void* d_image, int image_dtype, int h, int w, int spatial_bin_size,
                               int rootsift, double clipval, float* d_out) {
  using namespace pxr;
  PXR_REQUIRE(ctx && d_image && d_out, "pxr_dsift_dense: NULL argument");
  int rc = ds_check(image_dtype, h, w, spatial_bin_size, (float)clipval, "pxr_dsift_dense");
  if (rc != PXR_OK) return rc;
  PXR_HIP(hipSetDevice(ctx->device));
  const dim3 grid((unsigned)((w + DS_T - 1) / DS_T), (unsigned)((h + DS_T - 1) / DS_T));
  for_storage<unsigned char, float>(image_dtype, [&](auto sr) {   // (the set ds_check admits)
    using SRC = typename decltype(sr)::type;
    hipLaunchKernelGGL(dsift_dense_kernel<SRC>, grid, dim3(256), 0, ctx->stream, (const SRC*)d_image, h, w, spatial_bin_size, rootsift,
                       (float)clipval, d_out);
  });
  return hip_check(hipGetLastError(), "dsift_dense_kernel launch");
}

extern "C" int pxr_dsift_extract(pxr_ctx* ctx, pxr_arena* a, int64_t first, int64_t n, const void* d_image, int image_dtype,
                                 int h, int w, int spatial_bin_size, int rootsift, double clipval, const double* d_keypoints,
                                 double image_w, double image_h, int l2_normalize) {
  using namespace pxr;
  PXR_REQUIRE(ctx && a && d_image && d_keypoints, "pxr_dsift_extract: NULL argument");
  PXR_REQUIRE(first >= 0 && n >= 0 && first + n <= a->n, "pxr_dsift_extract: range [%lld, %lld) outside arena of %lld patches",
              (long long)first, (long long)(first + n), (long long)a->n);
  if (a->C != 128)
    return set_error(PXR_EUNSUPPORTED, "pxr_dsift_extract: the arena has %d channels (dense SIFT has 128)", a->C);
  PXR_REQUIRE(a->H == a->W && a->H >= 1 && a->H <= DS_T, "pxr_dsift_extract: patch size %dx%d not supported (square, <= 16)",
              a->H, a->W);
  int rc = ds_check(image_dtype, h, w, spatial_bin_size, (float)clipval, "pxr_dsift_extract");
  if (rc != PXR_OK) return rc;
  PXR_REQUIRE(h > a->H && w > a->W, "pxr_dsift_extract: image %dx%d must exceed the patch size", h, w);
  PXR_REQUIRE(image_w > 0 && image_h > 0, "pxr_dsift_extract: image size must be positive");
  if (n == 0) return PXR_OK;
  PXR_REQUIRE(n < ((int64_t)1 << 31), "pxr_dsift_extract: %lld keypoints in one call (at most 2^31 - 1)", (long long)n);
  PXR_HIP(hipSetDevice(ctx->device));
  const double sx = (double)w / image_w, sy = (double)h / image_h;   // extractor.py:177
  bool ok = false;
  for_storage<unsigned char, float>(image_dtype, [&](auto sr) {   // (the set ds_check admits)
    using SRC = typename decltype(sr)::type;
    ok = for_storage<_Float16, float, double>(a->dtype, [&](auto ds) {
      using DST = typename decltype(ds)::type;
      hipLaunchKernelGGL((dsift_extract_kernel<SRC, DST>), dim3((unsigned)n), dim3(256), 0, ctx->stream, (const SRC*)d_image, h, w,
                         spatial_bin_size, rootsift, (float)clipval, d_keypoints, sx, sy, l2_normalize, (DST*)a->d_data, a->d_corners,
                         a->d_scales, first, a->H);
    });
  });
  if (!ok) return set_error(PXR_EINVAL, "pxr_dsift_extract: bad arena dtype");
  return hip_check(hipGetLastError(), "dsift_extract_kernel launch");
}
