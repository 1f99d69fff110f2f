/*
 * pixsfm_hip.h -- C-ABI of the MI355X-native featuremetric refinement engine
 * (libpixsfm_hip.so).  Drop-in boundary for pixsfm's keypoint-adjustment (KA) and
 * bundle-adjustment (BA) hot path.
 *
 * The reference has no C plugin ABI: its seam is the pybind11 module pixsfm._pixsfm
 * (pixsfm/_pixsfm/bindings.cc:34-63) and, at the finest grain,
 * ceres::CostFunction::Evaluate(parameters, residuals, jacobians) [upstream Ceres]
 * called once per residual block.  This ABI is the batched, flat-array replacement of
 * that seam: plain pointers and sizes, no torch / pybind / Eigen types.  Each entry
 * point cites the reference interface it replaces.  INTEGRATION.md shows the binding a
 * pixsfm maintainer would add on the reference side.
 *
 * Conventions
 *  - every function returns 0 on success, a negative PXR_E* code on failure;
 *    pxr_last_error() returns a thread-local message (the reference throws C++
 *    exceptions mapped to Python, util/src/log_exceptions.h:52-116).
 *  - pointers prefixed d_ are DEVICE pointers (HBM), h_ are host pointers.
 *  - all work is enqueued on the context's HIP stream; functions that return host
 *    values synchronise that stream.
 *  - parameters are optimised IN PLACE in the caller's (device) arrays, like the
 *    reference does in caller memory (featuremetric_keypoint_optimizer.h:195-196,
 *    feature_reference_bundle_optimizer.h:111-114).
 *  - layouts: patches H x W x C channel-fastest (features/src/featurepatch.cc:160-163);
 *    qvec w-first (COLMAP); cam_params padded to PXR_KPAD doubles per camera.
 */
#ifndef PIXSFM_HIP_H_
#define PIXSFM_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PXR_KPAD 12 /* camera parameter slots per camera (FULL_OPENCV has 12) */
#define PXR_OBS_REC 8 /* doubles per fused observation record */

enum { PXR_OK = 0, PXR_EINVAL = -1, PXR_EHIP = -2, PXR_ENOMEM = -3, PXR_EUNSUPPORTED = -4,
       PXR_ENUMERIC = -5 };
enum { PXR_F16 = 0, PXR_F32 = 1, PXR_F64 = 2, PXR_U8 = 3 /* grey images (pxr_dsift_*) */ };
/* COLMAP 3.8 camera model ids (CAMERA_MODEL_SWITCH_CASES, residuals/src/feature_reference.h:232) */
enum { PXR_SIMPLE_PINHOLE = 0, PXR_PINHOLE = 1, PXR_SIMPLE_RADIAL = 2, PXR_RADIAL = 3,
       PXR_OPENCV = 4, PXR_OPENCV_FISHEYE = 5, PXR_FULL_OPENCV = 6, PXR_FOV = 7,
       PXR_SIMPLE_RADIAL_FISHEYE = 8, PXR_RADIAL_FISHEYE = 9, PXR_THIN_PRISM_FISHEYE = 10 };
/* ceres loss functions reachable through options.loss
 * (keypoint_adjustment_options.h:53, bundle_adjustment_options.h:49) */
enum { PXR_LOSS_TRIVIAL = 0, PXR_LOSS_CAUCHY = 1, PXR_LOSS_HUBER = 2, PXR_LOSS_SOFTL1 = 3 };

typedef struct pxr_ctx pxr_ctx;
typedef struct pxr_arena pxr_arena;

/* InterpolationConfig (base/src/interpolation.h:39-51, base/bindings.cc:134-154).
 * Only mode = BICUBIC with one node is on the hot path; other modes are rejected. */
typedef struct {
  int32_t l2_normalize;   /* default 1 */
  int32_t use_float_simd; /* default 0: fp32 horizontal pass, fp64 vertical pass.  1: all splines in fp32 (interpolation.h:177-218 with
                           * the float instantiation); pxr_ba_solve then evaluates from the texels in that arithmetic -- the
                           * Gram-matrix cache (exact fp64 algebra) is not used for such a solve */
  int32_t check_bounds;   /* default 0.  1: PatchInterpolator::Evaluate reports whether 0 < u < W, 0 < v < H
                           * (patch_interpolator.h:125-135,160-166).  Like in the reference this FAILS an evaluation
                           * only where the functor passes it on: the BA functor WITHOUT a reference descriptor, i.e.
                           * the cost-map BA (feature_reference.h:128-130) -- the block's squared norm is NaN, the
                           * solvers reject a non-finite trial cost and report PXR_TERM_FAILURE for a non-finite
                           * initial cost, like Ceres when Evaluate returns false.  With a reference descriptor
                           * (feature_reference.h:132-136) and in keypoint adjustment (featuremetric.h:61,
                           * feature_reference.h:59) the functors return true regardless: no effect. */
} pxr_interp_cfg;

typedef struct {
  int32_t type; /* PXR_LOSS_* */
  double a;     /* scale (Cauchy(0.25) is the reference default) */
} pxr_loss;

/* ---- context / errors ------------------------------------------------------------- */
int pxr_version(void);
const char* pxr_last_error(void);
/* device: HIP device ordinal; stream: a hipStream_t (e.g. torch's current stream
 * handle) or NULL for the device's default stream. */
int pxr_ctx_create(int device, void* stream, pxr_ctx** out);
int pxr_ctx_destroy(pxr_ctx* ctx);
int pxr_ctx_sync(pxr_ctx* ctx);
/* plain device-memory plumbing so that a host without torch can drive the library */
int pxr_malloc(pxr_ctx* ctx, size_t bytes, void** d_ptr);
int pxr_free(pxr_ctx* ctx, void* d_ptr);
int pxr_memcpy_h2d(pxr_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
int pxr_memcpy_d2h(pxr_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);
int pxr_memset(pxr_ctx* ctx, void* d_dst, int value, size_t bytes);
/* HIP-event timer on the context's stream: start/stop bracket enqueued work;
 * pxr_timer_stop synchronises and returns elapsed milliseconds. */
int pxr_timer_start(pxr_ctx* ctx);
int pxr_timer_stop(pxr_ctx* ctx, double* ms);

/* ---- patch arena --------------------------------------------------------------------
 * Flat HBM-resident replacement of the FeaturePatch/FeatureMap/FeatureSet/FeatureView
 * container hierarchy (features/src/featurepatch.h:40-156, featureview.cc:44-55): n
 * patches of identical H x W x C and dtype, patch i at data + i*H*W*C, with per-patch
 * corner_ (x0,y0) and scale_ (sx,sy) (upsampling_factor_ is 1 for feature patches). */
int pxr_arena_create(pxr_ctx* ctx, int dtype, int C, int H, int W, int64_t n_patches,
                     void* d_data_or_null /* adopt caller's device buffer, non-owning */,
                     pxr_arena** out);
int pxr_arena_destroy(pxr_arena* a);
/* copy `count` patches (host, HWC) and their metadata; corners int32[count][2],
 * scales double[count][2].  h_patches may be NULL to only set metadata. */
int pxr_arena_upload(pxr_arena* a, int64_t first, int64_t count, const void* h_patches,
                     const int32_t* h_corners, const double* h_scales);
/* The same from `count` SEPARATE host patches (h_patch_ptrs[i]: H*W*C elements, HWC) -- the FeaturePatch objects a
 * FeatureView hands out one by one (features/src/featureview.cc:44-55, featurepatch.h:40-156): gathered by all host cores
 * into pinned staging buffers and uploaded double-buffered, without a stacked host copy of the set. */
int pxr_arena_upload_gather(pxr_arena* a, int64_t first, int64_t count, const void* const* h_patch_ptrs,
                            const int32_t* h_corners, const double* h_scales);
/* Sparse patch producer on the device: replaces FeatureExtractor.tensor_to_fmap's
 * sparse branch + extract_patches_torch/_numpy (pixsfm/features/extractor.py:152-199,
 * features/extract_patches.py:13-44) and the GPU -> CPU -> optimiser copies behind them.
 * d_fmap: ONE image's dense feature map on the device, torch layout [C][h][w], src_dtype PXR_F16 or
 * PXR_F32, C = the arena's channels (128 / 64: CNN features; 3 / 1: the `image` model's colour / grey values,
 * features/models/image.py).  d_keypoints [n][2]: COLMAP image coordinates.  scale =
 * (w / image_w, h / image_h); corner = clip((int)(kp * scale - 8), 0, (w, h) - 16 - 1) (C truncation,
 * like astype(np.int32)); l2_normalize: torch.nn.functional.normalize over channels (fp32,
 * eps 1e-12) before the cast to the arena dtype (extractor.py:173-175).  Fills patches
 * [first, first + n) of the arena (square patches of side ps <= 16; "8" / "16" above read ps / 2 and
 * ps) with their corners and scales; asynchronous on the context's stream. */
int pxr_arena_extract(pxr_ctx* ctx, pxr_arena* a, int64_t first, int64_t n, const void* d_fmap,
                      int src_dtype, int h, int w, const double* d_keypoints, double image_w,
                      double image_h, int l2_normalize);
/* Dense SIFT, the reference's weight-free `dsift` model (pixsfm/features/models/dsift.py, pixsfm/configs/dsift.yaml):
 * kornia >= 0.6.4 DenseSIFTDescriptor(num_ang_bins=8, num_spatial_bins=4, spatial_bin_size, rootsift, clipval, stride=1,
 * padding=1) on the grey image (PIL convert("L"), to_tensor).  Definition restated in DESIGN.md §16.
 * d_image: the grey image on the device, row-major h x w, image_dtype PXR_U8 (value / 255, as to_tensor) or PXR_F32.
 * spatial_bin_size: even, 2 .. 8 (other values: PXR_EUNSUPPORTED); 128 channels (8 angle x 4 x 4 spatial bins).
 * pxr_dsift_dense writes the model's output, d_out [128][h][w] fp32 (torch layout); asynchronous on the context's stream. */
int pxr_dsift_dense(pxr_ctx* ctx, const void* d_image, int image_dtype, int h, int w, int spatial_bin_size, int rootsift,
                    double clipval, float* d_out);
/* The fused sparse producer: pxr_arena_extract (FeatureExtractor.tensor_to_fmap sparse branch, extractor.py:152-199) of the
 * dense SIFT map of d_image, computed only on the patch windows.  The map is the image itself (h x w), so scale =
 * (w / image_w, h / image_h) with (image_w, image_h) the ORIGINAL image size; corners, l2_normalize and the cast as in
 * pxr_arena_extract; the arena must have C = 128 (else PXR_EUNSUPPORTED) and square patches of side ps <= 16 with
 * h, w > ps.  Fills patches [first, first + n) bit-identical to pxr_dsift_dense followed by pxr_arena_extract;
 * asynchronous on the context's stream. */
int pxr_dsift_extract(pxr_ctx* ctx, pxr_arena* a, int64_t first, int64_t n, const void* d_image, int image_dtype, int h,
                      int w, int spatial_bin_size, int rootsift, double clipval, const double* d_keypoints, double image_w,
                      double image_h, int l2_normalize);
/* ---- SIFT: keypoints and descriptors of one grey image (csrc/pxr_sift.hip) ----
 * The sparse sibling of dsift: what hloc's `sift` configuration or a COLMAP SIFT database hands to the reference.  Restated from
 * Lowe's paper and VLFeat's sift.c as remembered -- parity with VLFeat / COLMAP is unpinned.  This comment
 * is the specification; tests/sift_cases.py transcribes it in numpy float64.  Coordinates are pixel indices (pixel centres at
 * integers, x along columns, y along rows); angles run from x towards y.
 *  Input      h x w row-major, PXR_U8 (the float32 quotient (float)u / 255.0f) or PXR_F32.  One image per call.
 *  Octaves    octave first_octave starts from the image (0) or from its doubling (-1): u(2i) = I(i), u(2i+1) = (I(i) +
 *             I(min(i+1, n-1))) / 2 along x, then along y, so coordinates scale by exactly 0.5.  Octave o+1 is (h_o+1)/2 x (w_o+1)/2:
 *             its level 0 is level S of octave o at even indices.  Automatic count: octaves while min(h_o, w_o) >= 16, at most 8
 *             (an image smaller than that has no octave and no feature); num_octaves > 0 takes the first num_octaves of them.
 *  Levels     s = 0 .. S+2 with sigma(s) = sigma0 2^(s/S) in the octave's pixels.  Level 0 of the first octave blurs the (doubled)
 *             input by sqrt(sigma0^2 - (sigma_in 2^-first_octave)^2); level s blurs level s-1 by sigma0 sqrt(2^(2s/S) - 2^(2(s-1)/S)).
 *  Blur       by sigma: rows (along x), then columns; radius r = int(4 sigma + 0.5) <= 18 (else PXR_EINVAL); weights
 *             exp(-x^2 / 2 sigma^2) divided by their sum (added in ascending x) in float64 on the host, rounded to float32; borders
 *             replicated; the float32 sum acc = 0, acc = acc + w[k] v[k] for k = -r .. r in that order, product and sum each
 *             rounded once.  (scipy.ndimage.gaussian_filter1d(truncate=4, mode="nearest") up to rounding.)
 *  Pyramid    d_pyramid: plane (k, s) of octave index k = o - first_octave is h_k x w_k float32 at float offset
 *             offsets[k] + s h_k w_k, offsets[k] = sum over k' < k of (S+3) h_k' w_k' (pxr_sift_pyramid_layout reports sizes and
 *             offsets for 8 octaves, pxr_sift_pyramid_bytes the total).  Everything below reads it as float32 and computes in float64.
 *  Detection  D(s) = G(s+1) - G(s), s = 0 .. S+1.  A candidate is a sample at s in 1 .. S, at least one pixel inside the border,
 *             with |D| > 0.8 peak_threshold, strictly above or strictly below all 26 neighbours.  Refinement at (X, Y) = (xi, yi):
 *             gradient and Hessian of D in (x, y, s) by central differences (mixed terms: a quarter of the four diagonal samples),
 *             H d = -g by Gaussian elimination with partial pivoting (the first largest pivot; a zero pivot rejects).  While fewer
 *             than max_refine_steps moves were made: X moves by +-1 if d_x > 0.6 / < -0.6 and stays in [1, w-2], Y likewise (s never
 *             moves); if either moved, repeat at the new (X, Y).  Accept iff |d_x|, |d_y|, |d_s| < 1.5, 0 <= s + d_s <= S+1,
 *             |D + g.d / 2| > peak_threshold, and the spatial Hessian has det > 0 and ((e+1)^2 / e) det - tr^2 > 0, e = edge_threshold.
 *             Keypoint: x = (X + d_x) 2^o, y = (Y + d_y) 2^o, sigma = sigma0 2^(o + (s + d_s) / S), response |D + g.d / 2|, record
 *             (o, s, xi, yi) = the extremum's own sample (before any move), which is unique and orders the output.
 *             peak_threshold < 0 stands for 0.02 / S.
 *  Orientation on level min(max(floor(s + d_s + 0.5), 0), S+2) of the keypoint's octave, in its pixels (xo, yo, sigma_oct):
 *             sigma_w = 1.5 sigma_oct, R = floor(3 sigma_w); the integer samples (px, py) within R of (floor(xo+0.5), floor(yo+0.5))
 *             in both axes that lie in [1, w-2] x [1, h-2] and have d^2 = (px-xo)^2 + (py-yo)^2 < R^2 + 0.5, rows first.  Gradient by
 *             central differences / 2, angle a = atan2(gy, gx) in [0, 2 pi); a sample adds |g| exp(-d^2 / 2 sigma_w^2) at the bin
 *             coordinate 36 a / 2 pi - 0.5, split linearly over the two nearest of 36 circular bins.  Six circular passes of
 *             (a + b + c) / 3.  A peak is a bin above both neighbours and >= 0.8 of the maximum; theta = 2 pi (i + di + 0.5) / 36
 *             with di = -(h+ - h-) / (2 (h+ + h- - 2 h0)).  At most max_num_orientations peaks by (height descending, bin
 *             ascending), each a feature; features are ordered by (keypoint, rank).  upright: one feature, theta = 0.
 *  Descriptor of (x, y, sigma, theta) alone: t = S log2(sigma / sigma0), octave o = floor((t - 0.5) / S) clamped to the pyramid's
 *             octaves, level floor(t - o S + 0.5) (outside 0 .. S+2: not valid; a keypoint of pxr_sift_detect never is).  Bin width b = magnif sigma_oct, W = floor(sqrt(2) b 2.5 + 0.5);
 *             samples as above within W (no circular cut).  (nx, ny) = the offset rotated by -theta, divided by b; a sample adds
 *             |g| exp(-(nx^2 + ny^2) / 8) (a window of sigma = 2 bins) at the bin coordinates (ny + 1.5, nx + 1.5, 8 ((a - theta)
 *             mod 2 pi) / 2 pi), trilinearly over 4 x 4 x 8 bins (the last circular; shares outside the 4 x 4 are dropped).  Then
 *             L2-normalise, clamp at clip, L2 again; normalization 1 (L1_ROOT, "rootsift"): divide by the L1 norm, square root.
 *             A zero histogram is not valid.  Output float32 (n, 128), unit L2 norm, channel = by * 32 + bx * 8 + bo: the layout
 *             pxr_match_descriptors takes.  No uint8 quantisation.
 *  All sums over samples run in sample order, whatever the lane: two runs give the same bits in every output. */
typedef struct {
  int32_t first_octave;          /* -1  (hloc's and COLMAP's default); {-1, 0}                              */
  int32_t num_octaves;           /* 0   automatic                                                          */
  int32_t octave_resolution;     /* 3   S in {2, 3, 4}                                                     */
  int32_t max_refine_steps;      /* 5   0 .. 16                                                            */
  int32_t max_num_orientations;  /* 2   1 .. 4                                                             */
  int32_t upright;               /* 0                                                                      */
  int32_t normalization;         /* 1   0 = L2, 1 = L1_ROOT                                                */
  int32_t reserved;              /* 0                                                                      */
  double sigma0;                 /* 1.6                                                                    */
  double sigma_in;               /* 0.5                                                                    */
  double peak_threshold;         /* -1  = 0.02 / S                                                         */
  double edge_threshold;         /* 10                                                                     */
  double magnif;                 /* 3                                                                      */
  double clip;                   /* 0.2                                                                    */
} pxr_sift_options;
/* Writes the defaults above. */
void pxr_sift_default_options(pxr_sift_options* options);
/* Every entry point below returns PXR_EINVAL, with nothing launched and every output untouched, for: h or w < 1 (or > 16384), an
 * option outside the range given above, sigma0 <= sigma_in 2^-first_octave, num_octaves above the automatic count, a blur radius
 * above 18, a negative capacity or n, a NULL pointer that is needed. */
/* The layout: *h_n_octaves, h_sizes [8][2] (h_k, w_k; 0 past the last octave), h_offsets [8] (in floats).  Host arrays. */
int pxr_sift_pyramid_layout(int h, int w, const pxr_sift_options* options, int32_t* h_n_octaves, int32_t* h_sizes, int64_t* h_offsets);
int pxr_sift_pyramid_bytes(int h, int w, const pxr_sift_options* options, int64_t* h_bytes);
/* Fills d_pyramid (pxr_sift_pyramid_bytes of device memory) from the image on the device; asynchronous on the context's stream. */
int pxr_sift_pyramid(pxr_ctx* ctx, const void* d_image, int image_dtype, int h, int w, const pxr_sift_options* options, float* d_pyramid);
/* The same, and the HIP-event time of all its kernels in milliseconds: h_kernel_ms[1]. */
int pxr_sift_pyramid_timed(pxr_ctx* ctx, const void* d_image, int image_dtype, int h, int w, const pxr_sift_options* options,
                           float* d_pyramid, double* h_kernel_ms);
/* Keypoints with orientations, in ascending (o, s, yi, xi), then rank of the orientation: d_keypoints double [capacity][4]
 * (x, y, sigma, theta), d_record int32 [capacity][4] (o, s, xi, yi), d_response float32 [capacity].  Writes the first
 * min(*h_n_found, capacity) features and never a byte past capacity; *h_n_found is always the number found.  With capacity = 0
 * the three arrays may be NULL.  Synchronises the context's stream. */
int pxr_sift_detect(pxr_ctx* ctx, const float* d_pyramid, int h, int w, const pxr_sift_options* options, int64_t capacity,
                    double* d_keypoints, int32_t* d_record, float* d_response, int64_t* h_n_found);
/* The same, and h_kernel_ms[5] = count, scan, write, orient, emit. */
int pxr_sift_detect_timed(pxr_ctx* ctx, const float* d_pyramid, int h, int w, const pxr_sift_options* options, int64_t capacity,
                          double* d_keypoints, int32_t* d_record, float* d_response, int64_t* h_n_found, double* h_kernel_ms);
/* Rows d_index[i] (NULL: i) of the n_in rows pxr_sift_detect wrote, i < n, split into what the Python layer returns: d_keypoints_out
 * double [n][4], d_xy double [n][2] = (x + offset, y + offset) (offset 0.5: COLMAP's convention, pixel centres at +0.5), d_scales
 * double [n], d_orientations double [n], d_scores float32 [n] (needs d_response).  An output that is NULL is not written; a row
 * whose index lies outside [0, n_in) is left untouched.  Asynchronous. */
int pxr_sift_gather(pxr_ctx* ctx, int64_t n, int64_t n_in, const int64_t* d_index, const double* d_keypoints, const float* d_response,
                    double offset, double* d_keypoints_out, double* d_xy, double* d_scales, double* d_orientations, float* d_scores);
/* Descriptors of the given keypoints double [n][4] (x, y, sigma, theta) -- those of pxr_sift_detect, or keypoints that moved since:
 * d_descriptors float32 [n][128], d_valid uint8 [n].  A keypoint that is not finite, has sigma <= 0, a scale outside the pyramid
 * or an empty window gets zeros and valid = 0; it never faults and leaves its neighbours alone.  Asynchronous. */
int pxr_sift_describe(pxr_ctx* ctx, const float* d_pyramid, int h, int w, const pxr_sift_options* options, int64_t n,
                      const double* d_keypoints, float* d_descriptors, uint8_t* d_valid);
/* The same, and h_kernel_ms[1]. */
int pxr_sift_describe_timed(pxr_ctx* ctx, const float* d_pyramid, int h, int w, const pxr_sift_options* options, int64_t n,
                            const double* d_keypoints, float* d_descriptors, uint8_t* d_valid, double* h_kernel_ms);

void* pxr_arena_data(pxr_arena* a);     /* device pointer of patch 0 */
int32_t* pxr_arena_corners(pxr_arena* a); /* device int32[n][2] */
double* pxr_arena_scales(pxr_arena* a);   /* device double[n][2] */
int64_t pxr_arena_size(pxr_arena* a);

/* ---- BA evaluation -------------------------------------------------------------------
 * Batched replacement of FeatureReferenceCostFunctor / ...ConstantPoseCostFunctor
 * ::operator() under ceres::AutoDiffCostFunction
 * (residuals/src/feature_reference.h:71-148,157-207), one unit = one observation =
 * one residual block of C residuals.  All arrays are device pointers. */
typedef struct {
  int64_t n_obs;
  const int32_t* d_obs_image; /* [n_obs] index into qvec/tvec/image_camera */
  const int32_t* d_obs_point; /* [n_obs] index into xyz/refs */
  const int64_t* d_obs_patch; /* [n_obs] index into the arena */
  int32_t n_images;
  const int32_t* d_image_camera; /* [n_images] */
  const double* d_qvec;          /* [n_images][4] */
  const double* d_tvec;          /* [n_images][3] */
  int32_t n_cameras;
  const int32_t* d_cam_model;    /* [n_cameras] PXR_* model id */
  const double* d_cam_params;    /* [n_cameras][PXR_KPAD] */
  int64_t n_points;
  const double* d_xyz;           /* [n_points][3] */
  const double* d_refs;          /* [n_points][C]  Reference::descriptor (references.h:65); NULL = no reference
                                    is subtracted (cost-map BA, costmap_bundle_optimizer.h:104-119) */
} pxr_ba_view;

/* Fused evaluation.  Per observation i writes the record d_rec[i][0..7]:
 *   [0] s = r.r   [1] gx.gx  [2] gx.gy  [3] gy.gy  [4] gx.r  [5] gy.r  [6] x  [7] y
 * where r = f(x,y) - ref (C residuals), gx = dr/dx, gy = dr/dy (image coordinates) and
 * (x,y) = WorldToPixel(...) (base/src/projection.h:60-75).  The C x n Jacobian of the
 * block is J = [gx gy] * d(x,y)/d(params) (Jet bridge, base/src/interpolation.h:130-140),
 * so J^T J, J^T r and the robustifier's corrector are functions of this record and of
 * the 2 x n projection Jacobian only; the 128-row Jacobian is never materialised.
 * with_jacobian = 0 evaluates only s, x, y (trial-point cost evaluation).
 * Optional materialised outputs for parity checks (NULL to skip):
 *   d_r [n_obs][C], d_gx [n_obs][C], d_gy [n_obs][C]. */
int pxr_ba_eval(pxr_ctx* ctx, pxr_arena* arena, const pxr_ba_view* view,
                const pxr_interp_cfg* cfg, int with_jacobian, double* d_rec, double* d_r,
                double* d_gx, double* d_gy);

/* Projection Jacobians for parity checks: d_P [n_obs][2][10 + PXR_KPAD], columns
 * q(4, ambient) t(3) X(3) k(PXR_KPAD); row 0 = dx/d., row 1 = dy/d. */
int pxr_ba_projection_jacobian(pxr_ctx* ctx, const pxr_ba_view* view, double* d_P);

/* Sum of 0.5 * rho(s_i) over the records (ceres cost), robustifier A20. */
int pxr_ba_cost(pxr_ctx* ctx, const double* d_rec, int64_t n_obs, const pxr_loss* loss,
                double* h_cost);


/* ---- BA solve -------------------------------------------------------------------------
 * Replaces BundleOptimizer::SolveProblem -> ceres::Solve
 * (bundle_adjustment/src/bundle_optimizer.h:172-245) for the feature-reference cost:
 * trust-region Levenberg-Marquardt [upstream Ceres 2.1 semantics: Jacobi scaling, LM
 * diagonal clamp, step acceptance, radius update, tolerances] with the point blocks
 * eliminated (Schur complement, what DENSE_SCHUR / SPARSE_SCHUR do, :181-191) and a dense
 * Cholesky of the reduced camera system on the GPU. */
enum { PXR_TERM_CONVERGENCE = 0, PXR_TERM_NO_CONVERGENCE = 1, PXR_TERM_FAILURE = 2 };

typedef struct {
  int32_t max_iterations;        /* 100 (bundle_adjustment_options.h:54)                */
  double function_tolerance;     /* 0                                                   */
  double gradient_tolerance;     /* 0                                                   */
  double parameter_tolerance;    /* 0                                                   */
  double initial_radius;         /* 1e4  [upstream ceres::Solver::Options defaults]     */
  double max_radius;             /* 1e16                                                */
  double min_radius;             /* 1e-32                                               */
  double min_relative_decrease;  /* 1e-3                                                */
  double min_lm_diagonal;        /* 1e-6                                                */
  double max_lm_diagonal;        /* 1e32                                                */
  int32_t max_consecutive_invalid_steps; /* 10 (bundle_adjustment_options.h:56)         */
  int32_t jacobi_scaling;        /* 1                                                   */
  int32_t use_inner_iterations;  /* BA: refine every variable point on its own after each trust-region step
                                    (bundle_adjustment/main.py:43 default True; [upstream Ceres]
                                    coordinate descent); ignored by pxr_ka_solve          */
  double inner_iteration_tolerance; /* 1e-3 [upstream]: disabled once the relative gain falls below */
  /* linear solver of the reduced camera system (BA only; bundle_optimizer.h:180-191 overrides the user's choice
   * by image count: <= 50 DENSE_SCHUR, <= 1000 SPARSE_SCHUR -- both = exact Schur complement + Cholesky, here the
   * dense GPU Cholesky -- and above ITERATIVE_SCHUR + SCHUR_JACOBI) */
  int32_t linear_solver;         /* PXR_LINEAR_AUTO: that rule on view->n_images; _DIRECT / _ITERATIVE force one   */
  int32_t max_linear_solver_iterations; /* 200 (bundle_adjustment_options.h:55)                                   */
  double eta;                    /* 0.1 [upstream Solver::Options::eta]: CG stops at i (Q_i - Q_{i-1}) / Q_i < eta,
                                    Q = x.Sx/2 - x.b (the only test the LM strategy leaves enabled [upstream])    */
  double linear_r_tolerance;     /* -1 = off like [upstream]; > 0: also stop at |r| <= tol |b| (parity tests)     */
} pxr_lm_options;
enum { PXR_LINEAR_AUTO = 0, PXR_LINEAR_DIRECT = 1, PXR_LINEAR_ITERATIVE = 2 };
#define PXR_MAX_IMAGES_DIRECT 1000 /* kMaxNumImagesDirectSparseSolver, bundle_optimizer.h:179 */

typedef struct {
  int32_t iterations;      /* LM iterations attempted                                   */
  int32_t num_successful;
  int32_t termination;     /* PXR_TERM_*                                                */
  int32_t num_camera_unknowns; /* size of the reduced camera system                     */
  int64_t num_point_unknowns;
  double initial_cost, final_cost, final_radius;
  double total_ms;         /* wall time of the LM loop (set-up excluded)                */
  double setup_ms;         /* host-side index construction + allocations                */
  int32_t linear_solver;   /* PXR_LINEAR_DIRECT / _ITERATIVE actually used (BA)         */
  int32_t collective_kib;   /* several ranks, direct solver: KiB moved per [S | rhs] all-reduce (packed upper triangle), else 0 */
  int64_t linear_iterations; /* pxr_ba_solve: conjugate-gradient iterations summed over the LM attempts (iterative solver);
                                pxr_ka_solve: node stencils (4 x 4 texels x C) interpolated over the solve -- its
                                algorithmic traffic is that count x 16 x C x sizeof(storage type)                 */
  int32_t accumulation;      /* how the sums over observations / points / ranks were formed in THIS solve: 1 = fixed-point integers
                                (the deterministic default: same bits for every run, launch shape and rank count), 2 = ordered
                                partial sums (the iterative solver's deterministic form: same bits per rank count), 0 = floating-
                                point atomics (pxr_set_deterministic(ctx, 0), or a direct solve WITHOUT Jacobi scaling, whose
                                columns no single grid can serve -- pxr_get_deterministic() alone does not tell)        */
  int32_t initial_us;        /* pxr_ba_solve: microseconds of total_ms spent BEFORE the first LM iteration -- the evaluation at the initial
                                point, the unscaled linearisation the Jacobi scaling is read from and the scaled one (device idle at
                                the end of it: the fixed-point check synchronises); 0 for pxr_ka_solve                    */
} pxr_lm_summary;

/* ceres::IterationCallback of the BA solve (the `solver.callbacks` of pixsfm's option dicts, base/src/callbacks.h; the
 * reference also keeps Ctrl-C responsive this way, util/src/py_interrupt.h): called on the host by pxr_ba_solve after the
 * initial evaluation (iteration 0) and after every LM iteration.  Return 0 to continue, 1 to abort (SOLVER_ABORT: the solve
 * ends with PXR_TERM_FAILURE, parameters as of the last accepted step), 2 to stop as converged (SOLVER_TERMINATE_SUCCESSFULLY).
 * With several ranks every rank calls its own callback and all must return the same value.  pxr_ka_solve runs its LM loops
 * inside one kernel and does not call back. */
typedef struct {
  int32_t iteration;            /* 0 = the initial evaluation                                            */
  int32_t step_is_valid;        /* the linear solve succeeded and the model cost decreased              */
  int32_t step_is_successful;   /* the step was accepted                                                */
  double cost;                  /* cost after this iteration (unchanged when the step was not accepted) */
  double cost_change;           /* cost before - candidate cost (0 for iteration 0 / invalid steps)     */
  double relative_decrease;     /* cost_change / model cost change                                      */
  double trust_region_radius;   /* radius the NEXT iteration starts with                                */
  double step_norm;
} pxr_iteration_summary;
typedef int (*pxr_iteration_callback)(const pxr_iteration_summary* summary, void* user);
int pxr_set_iteration_callback(pxr_ctx* ctx, pxr_iteration_callback fn /* NULL removes it */, void* user);

/* Deterministic mode: ON by default since round 5 (pxr_set_deterministic(ctx, 0) or PXR_DETERMINISTIC=0 in the environment of a
 * new context opt out).  Ceres sums each parameter block's Jacobian rows in a fixed order: the reference is run-to-run reproducible
 * for a fixed thread count (residuals/src/feature_reference.h:91-93 through AutoDiffCostFunction).  With the mode on, pxr_ba_solve
 * (direct solver) and pxr_ka_solve produce bit-identical results from run to run, for every launch shape AND for every number of
 * ranks: matrix / vector accumulations round each addend to a fixed-point grid and add 64-bit integers (associative; the grid is
 * derived from the measured diagonal of the previous linearisation and every linearisation is checked for overflow and repeated on
 * a coarser grid if need be), scalar sums are four 40-bit limbs per scalar, and several ranks all-reduce the integers (ncclInt64).
 * The iterative solver (> 1000 images) sums ORDERED PARTIALS instead -- every chunk of an image's observations leaves its part in a
 * buffer, the parts are added per image and per reduced-system column in a fixed order -- which gives the same bits on every run
 * for a given number of ranks (the ranks' parts are all-reduced as doubles).  The grids need the Jacobi scaling of the options (the
 * default); a direct solve without it falls back to floating-point atomics: fast, but the order of the additions -- hence the last
 * bits, hence now and then an accept / reject decision of the trust-region loop -- varies from run to run.  Costs ~3 % of an LM
 * iteration (1 % with the iterative solver), 8 % of a KA solve (bench.py reports both modes). */
int pxr_set_deterministic(pxr_ctx* ctx, int on);
int pxr_get_deterministic(pxr_ctx* ctx);

/* Gram-matrix cache of pxr_ba_solve: ON by default since round 5 (pxr_set_gram_cache(ctx, 0) or PXR_GRAM_CACHE=0 in the environment
 * of a new context switch it off).
 * The solver only consumes the 64-byte record of a residual block (pxr_ba_eval), and bicubic interpolation is linear in the
 * sixteen texels of the stencil: with the stencil's Gram matrix G = T T^t (16 x 16, over the channels) and D = T ref the
 * record is a set of quadratic / linear forms in the Catmull-Rom weights of the fractional position.  With the cache on,
 * pxr_ba_solve builds G and D once per observation (1 408 bytes each, HBM of the context, grow-only; rebuilt for the
 * observations whose projection moves to another texel) and evaluates every LM iteration from them instead of from the
 * 4 x 4 x C texels: ~3x less HBM traffic per iteration (the evaluation at the initial point of a solve still reads the
 * texels: the first step usually moves most projections to another texel).  The algebra on G is exact in double precision where the reference
 * interpolates with an fp32 horizontal pass (cubic_hermite_spline_simd.h), so a record differs from pxr_ba_eval's by that
 * pass's own rounding (1e-7 of the descriptor norm per channel): costs agree to ~1e-9 relative on sums over many blocks,
 * trajectories to the solver's tolerances; pxr_ba_eval itself, the other solvers and cost maps are unaffected.  Used for
 * feature patches of 128 / 64 channels in fp16 / fp32 storage with reference descriptors; otherwise the flag is ignored.
 * pxr_set_gram_cache(ctx, 0) also releases the storage.
 * Memory: 1 408 bytes per observation (+ 12 per observation of bookkeeping) in a grow-only buffer of the context -- 1.4 GB at 1M
 * observations -- allocated by the first solve that uses it and kept until the flag is cleared or the context is destroyed.  The
 * inner iterations (pxr_lm_options.use_inner_iterations) use the same buffer whenever the patches qualify, flag or no flag (set
 * PXR_INNER_NO_CACHE=1 to keep them from it); if it cannot be allocated they rebuild their matrices at every call instead. */
int pxr_set_gram_cache(pxr_ctx* ctx, int on);
int pxr_get_gram_cache(pxr_ctx* ctx);
/* The records of pxr_ba_eval(with_jacobian = 1) through that cache, outside a solve (parity tests, bench): reset != 0
 * (or a cache that does not fit the view yet) starts from an empty cache -- every observation's G is built -- otherwise the
 * matrices of the previous call are reused for the observations still in their cell.  The cache is keyed by observation
 * index: reuse it only with the same arena, observations and reference descriptors.  h_rebuilt (may be NULL; a non-NULL
 * pointer synchronises): how many observations' matrices this call built. */
int pxr_ba_eval_gram(pxr_ctx* ctx, pxr_arena* arena, const pxr_ba_view* view, const pxr_interp_cfg* cfg, int reset,
                     double* d_rec, int32_t* h_rebuilt);

/* ---- multi-GPU: one process per GPU ---------------------------------------------
 * With N ranks every rank holds ALL images and cameras (replicated) and a disjoint shard of the points with
 * all their observations, patches and references; the only exchange of the BA path is an in-place
 * all-reduce(sum) of doubles on the context's stream: [S | rhs] per linear solve (direct solver) or one
 * camera-sized vector per conjugate-gradient iteration (iterative solver), diag(U) | g_c per linearisation and
 * 16 scalars per LM attempt.  KA / reference extraction shard over independent sub-problems / points and
 * need no collective during the solve (base/src/parallel_optimizer.h:77-211 is the reference's shape).
 *
 * Native path: an RCCL communicator owned by the context.  Rank 0 calls pxr_comm_unique_id and hands the 128
 * bytes to the other ranks by any side channel (torch.distributed broadcast, a file, MPI, ...); then EVERY
 * rank calls pxr_comm_init (collective).  librccl is resolved at run time (the copy already loaded by the
 * process, e.g. PyTorch's, else /opt/rocm/lib/librccl.so.1), so the library has no link-time dependency. */
#define PXR_COMM_ID_BYTES 128
int pxr_comm_unique_id(void* h_id /* [PXR_COMM_ID_BYTES] */);
int pxr_comm_init(pxr_ctx* ctx, const void* h_id, int rank, int nranks);
int pxr_comm_destroy(pxr_ctx* ctx);
/* rank / size of the context: set by pxr_comm_init, or by pxr_comm_set_rank when the collective is a
 * caller-supplied callback (below); (0, 1) by default. */
int pxr_comm_set_rank(pxr_ctx* ctx, int rank, int nranks);
int pxr_comm_rank(pxr_ctx* ctx, int* rank, int* nranks);
/* in-place sum over the ranks of `count` doubles at device pointer d_buf, ordered with the context's stream
 * (ncclAllReduce on that stream); a no-op on a context without communicator / with one rank. */
int pxr_comm_allreduce_sum(pxr_ctx* ctx, double* d_buf, int64_t count);
/* Diagnostics.  pxr_comm_force(ctx, 1) (or PXR_FORCE_COLLECTIVE=1 in the environment when the context is created): a context
 * whose communicator has ONE rank still takes the multi-rank branch of the solvers -- pack, ncclAllReduce(ncclInt64 /
 * ncclFloat64) on the context's stream, unpack -- so that the native collective path can be exercised and timed on a single
 * GPU; results must be bit-identical to the plain one-rank solve (tests/test_zz_multi_rank_gpu.py).
 * pxr_comm_stats: ncclAllReduce calls / payload bytes issued through the context so far (NULL pointers are skipped). */
int pxr_comm_force(pxr_ctx* ctx, int on);
int pxr_comm_stats(pxr_ctx* ctx, int64_t* calls, int64_t* bytes, int reset);

/* Caller-supplied collective (same contract as pxr_comm_allreduce_sum), for hosts that bring their own
 * transport -- the CPU/gloo tests, MPI.  Passed to pxr_ba_solve it takes precedence over the context's
 * communicator; NULL = use the communicator (or run single-GPU). */
typedef int (*pxr_allreduce_fn)(void* user, double* d_buf, int64_t count);

/* Parameterisation (host arrays, bundle_optimizer.h:335-453):
 *   h_pose_const[img]      1 = qvec,tvec constant (HasConstantPose / !refine_extrinsics)
 *   h_tvec_const_mask[img] bit a = tvec[a] constant (SubsetManifold, ConstantTvec)
 *   h_cam_const_mask[cam]  bit a = camera parameter a constant (SubsetManifold / constant camera)
 *   h_point_const[pt]      1 = constant point
 * The qvec / tvec / cam_params / xyz device arrays of `view` are updated IN PLACE. */
int pxr_ba_solve(pxr_ctx* ctx, pxr_arena* arena, const pxr_ba_view* view, const pxr_interp_cfg* cfg,
                 const pxr_loss* loss, const uint8_t* h_pose_const, const uint8_t* h_tvec_const_mask,
                 const uint16_t* h_cam_const_mask, const uint8_t* h_point_const,
                 const pxr_lm_options* options, pxr_allreduce_fn allreduce, void* allreduce_user,
                 pxr_lm_summary* summary);

/* ---- geometric BA (strategy "geometric") ------------------------------------------------------
 * The reprojection residual r = WorldToPixel(camera, q, t, X) - xy_observed of
 * GeometricBundleOptimizer::AddResiduals (bundle_adjustment/src/geometric_bundle_optimizer.h:39-88; residuals/src/geometric.h
 * -> [upstream COLMAP 3.8] BundleAdjustmentCostFunction / BundleAdjustmentConstantPoseCostFunction), two residuals per
 * observation, no feature patches: view->d_obs_patch and view->d_refs are ignored and may be NULL.
 * d_obs_xy [n_obs][2]: the observed keypoint of every observation, image pixels, COLMAP convention (device pointer).
 *
 * pxr_ba_geom_eval replaces the evaluation of those cost functions: per observation the record of pxr_ba_eval,
 *   [rx^2 + ry^2, 1, 0, 1, rx, ry, x, y]   (gx = (1, 0), gy = (0, 1): the Jacobian of the block IS the projection Jacobian),
 * and optionally the residual itself, d_res [n_obs][2] (NULL to skip).  pxr_ba_cost and pxr_ba_projection_jacobian work on
 * such a view / such records unchanged. */
int pxr_ba_geom_eval(pxr_ctx* ctx, const pxr_ba_view* view, const double* d_obs_xy, double* d_rec, double* d_res);

/* Replaces GeometricBundleOptimizer::Run -> BundleOptimizer::SolveProblem -> ceres::Solve
 * (geometric_bundle_optimizer.h:22-37, bundle_optimizer.h:172-245).  The same LM loop as pxr_ba_solve with the same meaning of
 * the parameterisation arrays, options (PXR_LINEAR_AUTO by image count, inner iterations), summary, iteration callback,
 * deterministic mode and collectives; a non-finite evaluation ends the solve with PXR_TERM_FAILURE at the last accepted point.
 * The qvec / tvec / cam_params / xyz device arrays of `view` are updated IN PLACE. */
int pxr_ba_solve_geometric(pxr_ctx* ctx, const pxr_ba_view* view, const double* d_obs_xy, const pxr_loss* loss,
                           const uint8_t* h_pose_const, const uint8_t* h_tvec_const_mask,
                           const uint16_t* h_cam_const_mask, const uint8_t* h_point_const,
                           const pxr_lm_options* options, pxr_allreduce_fn allreduce, void* allreduce_user,
                           pxr_lm_summary* summary);

/* ---- covariance of a bundle adjustment (pose, intrinsics and point uncertainty) ------------------
 * What ceres::Covariance / COLMAP's EstimateBACovariance give: blocks of inv(H), H = J~^T J~ the Gauss-Newton matrix the LM loop
 * linearises at the parameters in `view` -- the same corrector, the same tangent columns in the same order (per image 3
 * rotation columns, then the variable tvec components; then per camera the variable intrinsics), no LM diagonal.
 *   Sigma_c = inv(S),  S = U - W inv(V) W^T the reduced camera matrix;
 *   Sigma_p = inv(V_p) + Y_p Sigma_c[cols(p), cols(p)] Y_p^T,  Y_p = inv(V_p) W_p^T, for a variable point p.
 * d_rec [n_obs][8]: the records of an evaluation at these parameters -- pxr_ba_eval (with Jacobians, on feature or cost-map
 * patches) or pxr_ba_geom_eval: the entry takes records, not a residual type; the caller evaluates first.  Nothing in `view` is
 * written.  The parameterisation arrays are those of pxr_ba_solve.
 * ROTATION UNITS: the rotation tangent is the solver's own, delta of QuaternionManifold::Plus, q <- (cos|d|, sin|d| d/|d|) * q:
 * the HALF-angle vector.  A rotation covariance in radians is 4 x the rotation block (2 x the rotation-translation block).
 * Outputs (device pointers, each may be NULL):
 *   d_cov_cameras    [n_c][n_c], n_c = summary->num_camera_unknowns, the dense Sigma_c in column order (not touched when n_c = 0)
 *   d_cov_pose       [n_images][6][6] in the order (rotation tangent, tx, ty, tz); rows and columns of constant components
 *                    (a constant pose, a tvec component under the mask) are zero
 *   d_cov_intrinsics [n_cameras][PXR_KPAD][PXR_KPAD], rows and columns of constant parameters zero
 *   d_cov_points     [n_points][3][3]; zero for a constant point and for a point without observation; NaN for a SINGULAR point:
 *                    one whose 3 x 3 block V_p meets, in its Cholesky factorisation, a pivot not above 64 u times its diagonal
 *                    entry (u = 2^-53; a point seen from one image).  Such points are counted and left out of S, as constant.
 * summary->info: 0, or the 1-based column at which S is rank deficient -- a gauge that is not fixed: the first pivot of the
 * Cholesky factorisation of the power-of-two scaled S that is not positive, or not above 64 n_c u times its diagonal entry.
 * The call then returns 0 and the outputs are unspecified.
 * Sums are those of the solver (fixed point in the deterministic mode); the new kernels use no atomics on floating-point
 * numbers: two calls give the same bits.  Not available on a context with several ranks (PXR_EINVAL). */
typedef struct {
  int32_t num_camera_unknowns;
  int32_t info;                    /* pivot index of a rank-deficient S, else 0 */
  int64_t num_singular_points;     /* variable points whose 3x3 block V is not positive definite */
  double ms_linearise, ms_factor_inverse, ms_points;
} pxr_cov_summary;

int pxr_ba_covariance(pxr_ctx* ctx, const pxr_ba_view* view, const double* d_rec /* [n_obs][8] */, const pxr_loss* loss,
                      const uint8_t* h_pose_const, const uint8_t* h_tvec_const_mask, const uint16_t* h_cam_const_mask,
                      const uint8_t* h_point_const,
                      double* d_cov_cameras /* [n_c][n_c] or NULL */, double* d_cov_pose /* [n_images][6][6] or NULL */,
                      double* d_cov_intrinsics /* [n_cameras][PXR_KPAD][PXR_KPAD] or NULL */,
                      double* d_cov_points /* [n_points][3][3] or NULL */, pxr_cov_summary* summary);

/* ---- track triangulation (known poses in, points and tracks out) ------------------------------
 * The middle stage of the reference's pipeline between keypoint adjustment and bundle adjustment, which PixSfM.triangulation
 * hands to COLMAP: pycolmap.triangulate_points as called by hloc.triangulation.main from pixsfm/refine_hloc.py:112-114.
 * Tracks are given in CSR form over the observations (observations of one track are contiguous); images and cameras exactly
 * as in pxr_ba_view.  All arrays are device pointers. */
typedef struct {
  int64_t n_tracks;
  const int64_t* d_track_offsets; /* [n_tracks + 1] monotone, last = n_obs: track t owns observations [offsets[t], offsets[t+1]) */
  int64_t n_obs;
  const int32_t* d_obs_image;     /* [n_obs] index into qvec/tvec/image_camera */
  const double* d_obs_xy;         /* [n_obs][2] the keypoints, image pixels, COLMAP convention */
  int32_t n_images;
  const int32_t* d_image_camera;  /* [n_images] */
  const double* d_qvec;           /* [n_images][4] */
  const double* d_tvec;           /* [n_images][3] */
  int32_t n_cameras;
  const int32_t* d_cam_model;     /* [n_cameras] PXR_* model id */
  const double* d_cam_params;     /* [n_cameras][PXR_KPAD] */
} pxr_tri_view;

/* [upstream COLMAP 3.8] IncrementalTriangulator::Options / EstimateTriangulationOptions values that the reference inherits
 * through hloc; max_hypotheses is this estimator's own bound (pairs are enumerated, not sampled). */
typedef struct {
  double min_tri_angle;     /* 1.5  degrees: smallest parallax of a hypothesis pair and of an accepted track        */
  double max_angle_error;   /* 2.0  degrees: angular inlier threshold between a ray and the point                    */
  double max_reproj_error;  /* 4.0  pixels: reprojection filter on the angular inliers                              */
  int32_t min_track_len;    /* 2    final inliers a track needs (never fewer than 2)                                */
  int32_t max_hypotheses;   /* 256  two-view hypotheses per track: all P = n (n - 1) / 2 pairs when P <= this, else
                                    pair number floor(h P / max_hypotheses), h = 0 .. max_hypotheses - 1            */
} pxr_tri_options;

/* Replaces [upstream COLMAP 3.8] Camera::ImageToWorld (<Model>::ImageToWorld of the eleven models), batched: the normalised
 * image point d_uv[i] whose projection under camera d_cam_index[i] (NULL: camera 0) is the pixel d_xy[i].  The pinholes are
 * closed form; every other model runs Newton on WorldToImage(u, v) - (x, y) with the model's analytic 2 x 2 Jacobian from the
 * pinhole normalisation, until the squared step is below 1e-20, 32 steps at most.  d_ok[i] (may be NULL) = 0 and d_uv[i] = NaN
 * where the iteration does not converge, meets a singular Jacobian or a non-finite value, or the camera index is out of range. */
int pxr_image_to_world(pxr_ctx* ctx, int64_t n, const int32_t* d_cam_index, int32_t n_cameras, const int32_t* d_cam_model,
                       const double* d_cam_params, const double* d_xy, double* d_uv, uint8_t* d_ok);

/* Replaces pycolmap.triangulate_points (hloc.triangulation.main, pixsfm/refine_hloc.py:112-114) for given tracks: every
 * observation becomes a world-frame ray (unit bearing d, camera centre c; an observation that cannot be undistorted is left
 * out), and every track is estimated on its own, deterministically:
 *   solve(S) = (sum_S (I - d d^t))^-1 sum_S (I - d d^t) c;  cos_i(X) = d_i . (X - c_i) / |X - c_i|, inlier: cos_i >= cos(max_angle_error)
 *   1. hypotheses X = solve({a, b}) over pairs a < b in lexicographic order (subsampled as in pxr_tri_options), skipped when
 *      d_a . d_b > cos(min_tri_angle) or when a or b is not an inlier of X;  2. the one with the largest (inlier count,
 *      -sum over inliers of (1 - cos_i), -index);  3. X' = solve(inliers), kept if it has at least as many inliers;
 *   4. final set = angular inliers with pixel error <= max_reproj_error; if that removed any and >= 2 remain, X = solve(final set);
 *   5. kept if the final set has >= max(2, min_track_len) members and two of them see X under >= min_tri_angle.
 * Outputs: d_status[t] 0 = point written to d_xyz[t], 1 = fewer than two usable observations, 2 = no hypothesis survived,
 * 3 = rejected in step 4 / 5; d_xyz[t] is left untouched unless status is 0; d_n_inliers[t] = size of the final set (0 unless
 * status is 0); per observation d_obs_inlier (member of the final set; 0 unless status is 0) and d_obs_err (pixel error of
 * every usable observation of a track with a point against the final X; NaN elsewhere).
 * PXR_EINVAL (nothing launched on the tracks): offsets not monotone or not ending at n_obs, an image or camera index out of range.
 * Synchronises the context's stream (the offsets are validated and the tracks ordered by length on the host). */
int pxr_triangulate_tracks(pxr_ctx* ctx, const pxr_tri_view* view, const pxr_tri_options* options, double* d_xyz,
                           int32_t* d_status, int32_t* d_n_inliers, uint8_t* d_obs_inlier, double* d_obs_err);
/* The same, and the HIP-event times of its kernels in milliseconds: h_kernel_ms[4] = validation, rays, compaction, tracks. */
int pxr_triangulate_tracks_timed(pxr_ctx* ctx, const pxr_tri_view* view, const pxr_tri_options* options, double* d_xyz,
                                 int32_t* d_status, int32_t* d_n_inliers, uint8_t* d_obs_inlier, double* d_obs_err,
                                 double* h_kernel_ms);

/* ---- absolute pose estimation (2D-3D correspondences in, one pose per query out) ---------------
 * The middle stage of the reference's QueryLocalizer.localize between query keypoint adjustment and query bundle adjustment:
 * pycolmap.absolute_pose_estimation (pixsfm/localization/main.py:458).  A batch of queries in CSR form over the correspondences
 * (correspondences of one query are contiguous), laid out like pxr_tri_view.  All arrays are device pointers.
 *
 * [upstream COLMAP 3.8] AbsolutePoseEstimationOptions / RANSACOptions / AbsolutePoseRefinementOptions values as pycolmap 0.x
 * exposes them, with the one override the reference makes (QueryLocalizer.default_conf.PnP.estimation.ransac.max_error = 12);
 * round_size, seed and lo_rounds are this estimator's own. */
#define PXR_ABSPOSE_LDS_CORR 1024 /* correspondences of a query the estimator stages on chip; a longer query reads the rest from memory */
typedef struct {
  double max_error;             /* 12.0     pixels: inlier threshold                                                      */
  double min_inlier_ratio;      /* 0.01     success needs n_inliers >= max(min_num_inliers, ceil(min_inlier_ratio n))      */
  double confidence;            /* 0.99999  of the stop rule                                                              */
  double refine_loss_scale;     /* 1.0      pixels: Cauchy scale of the refinement                                        */
  uint64_t seed;                /* 0        of the sample hash                                                            */
  int32_t min_num_inliers;      /* 4                                                                                      */
  int32_t min_num_trials;       /* 64       lower clamp of the stop rule                                                  */
  int32_t max_num_trials;       /* 4096     upper clamp of the stop rule, rounded up to a multiple of round_size          */
  int32_t round_size;           /* 64       samples per round: the stop rule is evaluated at round boundaries only        */
  int32_t refine_max_iterations;/* 100      Levenberg-Marquardt iterations per refinement                                 */
  int32_t lo_rounds;            /* 4        at most this many refine / re-classify repetitions                            */
} pxr_abspose_options;
/* Writes the defaults above. */
void pxr_abspose_default_options(pxr_abspose_options* options);

/* Replaces pycolmap.absolute_pose_estimation for a batch of queries.  This is NOT COLMAP's LO-RANSAC: the estimator has no
 * random state and reproduces bit for bit; a query alone and the same query inside any batch give the same bits (DESIGN.md
 * section 19).  Query q owns correspondences [d_query_offsets[q], d_query_offsets[q+1]): pixel d_xy[i] (COLMAP convention) of
 * camera d_query_camera[q] sees the point d_xyz[i].  Per query:
 *   1. every pixel goes through ImageToWorld (pxr_image_to_world); a correspondence that cannot be undistorted or holds a
 *      non-finite coordinate is unusable for the whole call; n = the usable ones, in order; n < 4: status 1.
 *   2. sample h = 0, 1, ... is three distinct indices: draw d = mix(mix(seed + G (h + 1)) + G (d + 1)) mod n, d = 0, 1, ..., with
 *      mix = the output function of splitmix64 and G = 0x9E3779B97F4A7C15 (64-bit wrap-around), a repeated index drawn again;
 *      the three are used in ascending order.  Neither q nor the batch enters.
 *   3. P3P (Grunert's quartic in v = s3 / s1, or the same coefficients reversed -- the quartic in 1 / v -- where |A0| > |A4|;
 *      Ferrari's real roots in the order (+,+) (+,-) (-,+) (-,-), a discriminant counting as zero down to -1e-7 of its terms;
 *      three Newton steps on the quartic each, a step kept only where |f| does not grow) gives up to four poses with positive
 *      distances; a degenerate sample gives none.  u = s2 / s1 = N(v) / D(v), except for a root with another root within 1e-3
 *      of it and |D(v)| <= 1e-3 (|D0| + |D1 v|), where N / D tends to 0 / 0: there u = cos(gamma) +- sqrt(cos^2(gamma) - 1 +
 *      (c^2 / b^2) (1 + v^2 - 2 v cos(beta))), + for the root with the smaller index of the two.  Then three Newton steps on
 *      the three equations (s_i - s_j)^2 + 2 s_i s_j (1 - cos) = side^2 in (s1, s2, s3), with 1 - cos = |f_i - f_j|^2 / 2 and each
 *      3 x 3 system by Cramer's rule (a step skipped where the determinant vanishes or the step is not finite); the pose from
 *      the polished distances.  Each is scored over all n in the normalised image plane:
 *      err = |(u, v) - (X/Z, Y/Z)|^2, inlier iff Z > 0 and err <= (max_error / mean focal)^2; the largest key
 *      (inlier count, -sum min(err, thr^2), -h, -root) wins.
 *   4. after each round of round_size samples: stop once samples done >= clamp(log(1 - confidence) / log(1 - w^3),
 *      min_num_trials, max_num_trials), w = best count / n.  No pose at all: status 2.
 *   5. local optimisation: Levenberg-Marquardt on the pixel residuals of the inliers through the full camera model (Cauchy
 *      weights rho'(|r|^2) of scale refine_loss_scale, pose on the quaternion manifold, intrinsics constant, step norm <= 1e-12
 *      or refine_max_iterations), then all n classified by pixel error <= max_error; repeated until the set stands still or
 *      lo_rounds; a refined pose with fewer inliers than the one before it is dropped.  The final set is pixel error <=
 *      max_error under the pose that stays.
 *   6. n_inliers < max(min_num_inliers, ceil(min_inlier_ratio n)): status 3.
 * Outputs: d_status[q] 0 = pose written to d_qvec[q] (unit, w >= 0) / d_tvec[q], which are left untouched otherwise;
 * d_n_inliers[q] (0 unless status is 0); d_n_trials[q] samples drawn; per correspondence d_inlier (0 unless status is 0) and
 * d_err (pixel error under the final pose of the usable correspondences of a status-0 query; NaN elsewhere and behind the camera).
 * PXR_EINVAL (nothing launched): offsets not starting at 0, not monotone or not ending at n_corr, a camera index out of range.
 * Synchronises the context's stream (offsets and cameras are validated and the queries ordered by size on the host). */
int pxr_absolute_pose(pxr_ctx* ctx, int32_t n_queries, const int64_t* d_query_offsets, int64_t n_corr, const double* d_xy,
                      const double* d_xyz, const int32_t* d_query_camera, int32_t n_cameras, const int32_t* d_cam_model,
                      const double* d_cam_params, const pxr_abspose_options* options, double* d_qvec, double* d_tvec,
                      int32_t* d_status, int32_t* d_n_inliers, int32_t* d_n_trials, uint8_t* d_inlier, double* d_err);
/* The same, and the HIP-event times of its kernels in milliseconds: h_kernel_ms[4] = records, compaction, hypotheses, refinement. */
int pxr_absolute_pose_timed(pxr_ctx* ctx, int32_t n_queries, const int64_t* d_query_offsets, int64_t n_corr, const double* d_xy,
                            const double* d_xyz, const int32_t* d_query_camera, int32_t n_cameras, const int32_t* d_cam_model,
                            const double* d_cam_params, const pxr_abspose_options* options, double* d_qvec, double* d_tvec,
                            int32_t* d_status, int32_t* d_n_inliers, int32_t* d_n_trials, uint8_t* d_inlier, double* d_err,
                            double* h_kernel_ms);

/* ---- two-view geometry (the matches of image pairs in, one relative pose and one inlier mask per pair out) ----
 * Geometric verification of matches, which the reference hands to COLMAP: pycolmap.verify_matches
 * (examples/refine_sift_aachen.py:51) and the same step inside hloc's reconstruction and triangulation -- for calibrated cameras.
 * A batch of image pairs in CSR form over their matches (matches of one pair are contiguous), laid out like pxr_absolute_pose.
 * All arrays are device pointers.
 *
 * max_error, confidence, max_num_trials, min_inlier_ratio and min_num_inliers are COLMAP 3.8's two-view geometry options as
 * remembered; COLMAP is not available where this library is built, so parity with it is UNPINNED.  min_num_trials, round_size,
 * seed, refine_max_iterations and lo_rounds are this estimator's own. */
#define PXR_TWOVIEW_LDS_MATCHES 1024 /* matches of a pair the estimator stages on chip; a longer pair reads the rest from memory */
/* The options of the three estimators over image pairs (essential matrix here, homography and fundamental matrix below): one
 * struct under three names.  What max_error measures is the estimator's: see its *_default_options. */
typedef struct {
  double max_error;             /* 4.0      pixels: inlier threshold on the estimator's error                             */
  double min_inlier_ratio;      /* 0.25     success needs n_inliers >= max(min_num_inliers, ceil(min_inlier_ratio n))      */
  double confidence;            /* 0.999    of the stop rule                                                              */
  uint64_t seed;                /* 0        of the sample hash                                                            */
  int32_t min_num_inliers;      /* 15                                                                                     */
  int32_t min_num_trials;       /* 64       lower clamp of the stop rule                                                  */
  int32_t max_num_trials;       /* 10000    upper clamp of the stop rule, rounded up to a multiple of round_size          */
  int32_t round_size;           /* 64       samples per round: the stop rule is evaluated at round boundaries only        */
  int32_t refine_max_iterations;/* 100      Levenberg-Marquardt iterations per refinement                                 */
  int32_t lo_rounds;            /* 4        at most this many refine / re-classify repetitions                            */
} pxr_pair_options;
typedef pxr_pair_options pxr_two_view_options;
/* Writes the defaults above; max_error is a threshold on the Sampson distance. */
void pxr_two_view_default_options(pxr_two_view_options* options);

/* Essential-matrix estimation and verification for a batch of image pairs.  This is NOT COLMAP's LO-RANSAC: the estimator has no
 * random state and reproduces bit for bit; a pair alone and the same pair inside any batch give the same bits (DESIGN.md section
 * 21).  Pair p owns matches [d_pair_offsets[p], d_pair_offsets[p+1]): pixel d_xy1[i] (COLMAP convention) of camera
 * d_pair_camera[2p] and pixel d_xy2[i] of camera d_pair_camera[2p+1] show one point.  The pose (q, t) is that of camera 2
 * relative to camera 1: X2 = R(q) X1 + t, |t| = 1, E = [t]x R.  Per pair:
 *   1. both pixels go through ImageToWorld (pxr_image_to_world); a match that cannot be undistorted on either side or holds a
 *      non-finite coordinate is unusable for the whole call; n = the usable ones, in order; n < 5: status 1.
 *   2. sample h = 0, 1, ... is five distinct indices: draw d = mix(mix(seed + G (h + 1)) + G (d + 1)) mod n, d = 0, 1, ..., with
 *      mix = the output function of splitmix64 and G = 0x9E3779B97F4A7C15 (64-bit wrap-around), a repeated index drawn again;
 *      the five are used in ascending order.  Neither p nor the batch enters.
 *   3. the five-point solver (Nister 2004): null space of the 5 x 9 epipolar system (rows x2 (x) x1) by Gauss-Jordan with full
 *      pivoting (the largest entry, the first of equals in row-major order; vector k = (-C[:, k], e_k) of [I | C] in the permuted
 *      columns), orthonormalised by modified Gram-Schmidt in the order k = 0 .. 3 and mixed by the 4 x 4 Hadamard matrix / 2
 *      (signs ++++ +-+- ++-- +--+) into X, Y, Z, W, so that no single entry of E decides the size of the constant term;
 *      E = x X + y Y + z Z + W; the ten cubic constraints (the nine of
 *      (E E^t - tr(E E^t) / 2) E row by row, then det E) as a 10 x 20 matrix in the monomial order x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2
 *      xyz xy xz^2 xz x yz^2 yz y z^3 z^2 z 1, Gauss-Jordan with partial pivoting on its first ten columns; B(z) from rows (4) - z (5), (6) - z (7),
 *      (8) - z (9); det B(z) of degree 10 scaled by its largest coefficient; Cauchy's bound 1 + max |c_k / c_10|; a Sturm chain
 *      with every remainder scaled to a largest coefficient of 1 (a leading coefficient <= 1e-12 after that is dropped); the k-th
 *      real root by 64 bisection steps on the sign-change count from (-bound, bound), then 4 Newton steps, each kept only inside
 *      the last interval; roots ascending, at most ten; (x, y, 1) = the cross product of the two rows of B(z) with the largest third
 *      component; then Gauss-Newton steps over (x, y, z), until one is no larger than 1e-10 max(1, |x|, |y|, |z|) and eight at the
 *      most, on the ten cubic constraints evaluated on the 3 x 3 matrix E itself (the 3 x 3 normal equations by the adjugate; a
 *      step skipped where their determinant vanishes or the step is not finite, and then ends the iteration), which returns the
 *      digits that the elimination loses.  Hypotheses are accurate to 600 kappa u (kappa: the norm of d E / d sample, u = 2^-53)
 *      at a baseline of at least 0.1 of the median depth and on planar scenes, forward motion, small rotations, wide and narrow
 *      fields (FIVE_POINT_MIN_PARALLAX of tests/twoview_cases.py); below that baseline the elimination loses whole roots, which no
 *      polish returns.  No hypothesis (and no NaN) from a sample with a pivot <= 1e-12 of its system's largest entry, a leading
 *      coefficient <= 1e-9 of the largest, or any value that is not finite.
 *   4. each E is scored over all n in the normalised image plane by the squared Sampson error err = (x2^t E x1)^2 / ((E x1)_0^2 +
 *      (E x1)_1^2 + (E^t x2)_0^2 + (E^t x2)_1^2); inlier iff err <= thr^2, thr = (max_error / f1 + max_error / f2) / 2 with f the
 *      mean focal length; the largest key (inlier count, -sum min(err, thr^2), -h, -root) wins, the sum taken in index order.
 *   5. after each round of round_size samples: stop once samples done >= clamp(log(1 - confidence) / log(1 - w^5),
 *      min_num_trials, max_num_trials), w = best count / n.  No hypothesis at all: status 2.
 *   6. the winner's E becomes (R, +-t) in closed form (Horn 1990, no SVD): t t^t = tr(E E^t) / 2 I - E E^t, t from the row of
 *      the largest diagonal entry; with E scaled to tr(E E^t) = 2, Ra = Cof(E) - [t]x E and Rb = Cof(E) + [t]x E (Cof: row i = row
 *      i+1 x row i+2).  Of (Ra, t) (Ra, -t) (Rb, t) (Rb, -t) the one with the most of the winner's inliers in front of both cameras
 *      stays (ties: the first).  Local optimisation: Levenberg-Marquardt on the inliers' signed Sampson residuals over five
 *      parameters (rotation on the quaternion manifold as in pxr_absolute_pose; t + a b1 + b b2 re-normalised, b1 = t x e_m /
 *      |t x e_m| for the axis m of the smallest |t_m|, b2 = t x b1; step norm <= 1e-12 or refine_max_iterations), then all n
 *      classified under E = [t]x R; repeated until the set stands still or lo_rounds; a refined pose with fewer inliers than
 *      the one before it is dropped.
 *   7. n_inliers < max(min_num_inliers, ceil(min_inlier_ratio n)): status 3.
 * With d_prior_qvec [n_pairs][4] / d_prior_tvec [n_pairs][3] non-NULL (both or neither; any length of t) steps 2-6 are skipped:
 * d_n_trials is 0, the matches are classified under the given pose (q and t normalised for E), and d_qvec / d_tvec come back
 * as they were given, bit for bit: not unit unless the prior was, and w may be negative; a prior that is not finite or has a zero
 * quaternion or translation gives status 2.
 * Outputs: d_status[p] 0 = pose written to d_qvec[p] (unit, w >= 0) / d_tvec[p] (unit; with a prior: as given) and E = [t]x R (row-major, Frobenius
 * norm sqrt 2) to d_E[p], all three left untouched otherwise; d_n_inliers[p] (0 unless status is 0); d_n_trials[p] samples drawn;
 * per match d_inlier (0 unless status is 0) and d_err (sqrt(err) max_error / thr, i.e. the Sampson distance in pixels, of the
 * usable matches of a status-0 pair; NaN elsewhere).
 * PXR_EINVAL (nothing launched): offsets not starting at 0, not monotone or not ending at n_matches, a camera index out of
 * range, an option out of range, one prior array without the other.
 * Synchronises the context's stream (offsets and cameras are validated and the pairs ordered by size on the host). */
int pxr_two_view_geometry(pxr_ctx* ctx, int32_t n_pairs, const int64_t* d_pair_offsets, int64_t n_matches, const double* d_xy1,
                          const double* d_xy2, const int32_t* d_pair_camera, int32_t n_cameras, const int32_t* d_cam_model,
                          const double* d_cam_params, const double* d_prior_qvec, const double* d_prior_tvec,
                          const pxr_two_view_options* options, double* d_qvec, double* d_tvec, double* d_E, int32_t* d_status,
                          int32_t* d_n_inliers, int32_t* d_n_trials, uint8_t* d_inlier, double* d_err);
/* The same, and the HIP-event times of its kernels in milliseconds: h_kernel_ms[4] = records, compaction, hypotheses, refinement. */
int pxr_two_view_geometry_timed(pxr_ctx* ctx, int32_t n_pairs, const int64_t* d_pair_offsets, int64_t n_matches, const double* d_xy1,
                                const double* d_xy2, const int32_t* d_pair_camera, int32_t n_cameras, const int32_t* d_cam_model,
                                const double* d_cam_params, const double* d_prior_qvec, const double* d_prior_tvec,
                                const pxr_two_view_options* options, double* d_qvec, double* d_tvec, double* d_E, int32_t* d_status,
                                int32_t* d_n_inliers, int32_t* d_n_trials, uint8_t* d_inlier, double* d_err, double* h_kernel_ms);

/* ---- homography estimation (the matches of image pairs in, one homography, one rotation-only model and one inlier mask per
 * pair out) ----
 * The planar / panoramic half of geometric verification: pycolmap.verify_matches classifies a pair from the ratio of homography
 * inliers to essential-matrix inliers, because an essential matrix fits a pure-rotation or a planar pair with a translation
 * direction that means nothing.  For calibrated cameras (fundamental-matrix estimation: pxr_fundamental below).  The batch is laid
 * out like pxr_two_view_geometry's, and the options are its options with its defaults (COLMAP 3.8's values as remembered, parity
 * UNPINNED; min_num_trials, round_size, seed, refine_max_iterations and lo_rounds are this estimator's own). */
typedef pxr_pair_options pxr_homography_options;
/* Writes the defaults of pxr_pair_options; max_error is a threshold on the forward transfer error in image 2. */
void pxr_homography_default_options(pxr_homography_options* options);

/* Homography estimation for a batch of image pairs, deterministic like pxr_two_view_geometry: no random state, a pair alone and the
 * same pair inside any batch give the same bits.  Pair p owns matches [d_pair_offsets[p],
 * d_pair_offsets[p+1]).  H maps the normalised plane of camera 1 to that of camera 2: x2 ~ H (x1, y1, 1).  Per pair:
 *   1. usable matches and records exactly as in step 1 of pxr_two_view_geometry: both pixels go through ImageToWorld, the record
 *      is (x1, y1, x2, y2) in the normalised plane; n = the usable ones, in order; n < 4: status 1.
 *   2. sample h = 0, 1, ... is four distinct indices from the hash of pxr_two_view_geometry's step 2, used in ascending order.
 *   3. the four-point solver: the 8 x 9 DLT system, per match the rows (0, 0, 0, -x1, -y1, -1, y2 x1, y2 y1, y2) and
 *      (x1, y1, 1, 0, 0, 0, -x2 x1, -x2 y1, -x2); its null vector by Gauss-Jordan with full pivoting (the largest entry, the first
 *      of equals in row-major order; the vector (-C[:, 0], e_0) of [I | C] in the permuted columns), scaled to Frobenius norm 1
 *      (the squares summed in index order).  No hypothesis from a pivot <= 1e-12 of the system's largest entry or a value that
 *      is not finite.  Sign: w_i = H[2] . (x1_i, y1_i, 1) over the four sample matches; all positive keeps H, all negative
 *      negates it, mixed signs or a zero give no hypothesis.
 *   4. each H is scored over all n by the squared forward transfer error in image 2, err = |pi(H x1) - x2|^2 with
 *      pi(X, Y, W) = (X / W, Y / W), and +inf where W <= 0; inlier iff err <= thr^2, thr = max_error / f2 with f2 the mean focal
 *      length of camera 2; the largest key (inlier count, -sum min(err, thr^2), -h) wins, the sum taken in index order.
 *   5. after each round of round_size samples: stop once samples done >= clamp(log(1 - confidence) / log(1 - (w w) (w w)),
 *      min_num_trials, max_num_trials), w = min(max(best count, need) / n, 1), need = max(min_num_inliers,
 *      ceil(min_inlier_ratio n)).  The floor `need` is deliberate: a pair that admits no homography -- the usual case in a general
 *      scene -- stops once a model that could pass step 8 would have been found at the configured confidence (1765 samples at
 *      ratio 0.25, rounded up to the round: 1792) and does not run to max_num_trials.  No hypothesis at all: status 2.
 *   6. local optimisation: Levenberg-Marquardt on the inliers' two residuals pi(H x1) - x2 per match over eight parameters: the
 *      entry of largest magnitude of the unit-norm H is held fixed (the first of equals), the other eight move additively;
 *      lambda from 1e-4, x 0.1 (not below 1e-12) on a kept step, x 10 on a refused or unsolvable one, until lambda > 1e12, a step
 *      of norm <= 1e-12 or refine_max_iterations; a step is kept unless the cost grows by more than 1e-12 of itself; H is scaled
 *      back to Frobenius norm 1 after the refinement, then all n are classified again; repeated until the set stands still or
 *      lo_rounds; a refined H with fewer inliers than the one before it is dropped.
 *   7. the rotation-only model (the panoramic test), on the final H of a pair that passes step 8: H with its sign chosen so that det H >= 0; R0 from
 *      its rows by modified Gram-Schmidt (row 0, row 1, then their cross product; a row of norm <= 1e-12 ends the step with
 *      n_rot_inliers = 0 and d_rot_qvec untouched); its quaternion refined by the Levenberg-Marquardt of step 6 over the three
 *      parameters of the quaternion manifold (as in pxr_absolute_pose) on the H inliers' transfer residuals under H = R; all n
 *      classified under R with the same thr: that count is n_rot_inliers.
 *   8. n_inliers < need: status 3.
 * Outputs: d_status[p] 0 = H (row-major, normalised plane, Frobenius norm 1, third component positive on every inlier) written to
 * d_H[p] and the rotation to d_rot_qvec[p] (unit, w >= 0), both left untouched otherwise; d_n_inliers[p] and d_n_rot_inliers[p]
 * (0 unless status is 0); d_n_trials[p] samples drawn; per match d_inlier (0 unless status is 0) and d_err (sqrt(err) max_error /
 * thr, i.e. the transfer error in pixels, of the usable matches of a status-0 pair; NaN elsewhere and where W <= 0).
 * PXR_EINVAL (nothing launched): offsets not starting at 0, not monotone or not ending at n_matches, a camera index out of
 * range, an option out of range.
 * Synchronises the context's stream (offsets and cameras are validated and the pairs ordered by size on the host). */
int pxr_homography(pxr_ctx* ctx, int32_t n_pairs, const int64_t* d_pair_offsets, int64_t n_matches, const double* d_xy1,
                   const double* d_xy2, const int32_t* d_pair_camera, int32_t n_cameras, const int32_t* d_cam_model,
                   const double* d_cam_params, const pxr_homography_options* options, double* d_H, double* d_rot_qvec,
                   int32_t* d_status, int32_t* d_n_inliers, int32_t* d_n_rot_inliers, int32_t* d_n_trials, uint8_t* d_inlier,
                   double* d_err);
/* The same, and the HIP-event times of its kernels in milliseconds: h_kernel_ms[4] = records, compaction, hypotheses, refinement. */
int pxr_homography_timed(pxr_ctx* ctx, int32_t n_pairs, const int64_t* d_pair_offsets, int64_t n_matches, const double* d_xy1,
                         const double* d_xy2, const int32_t* d_pair_camera, int32_t n_cameras, const int32_t* d_cam_model,
                         const double* d_cam_params, const pxr_homography_options* options, double* d_H, double* d_rot_qvec,
                         int32_t* d_status, int32_t* d_n_inliers, int32_t* d_n_rot_inliers, int32_t* d_n_trials, uint8_t* d_inlier,
                         double* d_err, double* h_kernel_ms);

/* ---- fundamental-matrix estimation (the matches of image pairs in, one fundamental matrix and one inlier mask per pair out) ----
 * The uncalibrated half of geometric verification: pycolmap.verify_matches estimates F and H only for a camera without a prior
 * focal length, and next to E otherwise (a pair whose E explains noticeably fewer matches than its F is UNCALIBRATED).  The batch
 * is laid out like pxr_two_view_geometry's, and the options are its options with its defaults (COLMAP 3.8's values as remembered,
 * parity UNPINNED; min_num_trials, round_size, seed, refine_max_iterations and lo_rounds are this estimator's own). */
typedef pxr_pair_options pxr_fundamental_options;
/* Writes the defaults of pxr_pair_options; max_error is a threshold on the Sampson distance. */
void pxr_fundamental_default_options(pxr_fundamental_options* options);

/* Fundamental-matrix estimation for a batch of image pairs, deterministic like pxr_two_view_geometry: no random state, a pair alone
 * and the same pair inside any batch give the same bits.  This is NOT COLMAP's LO-RANSAC, and parity with
 * COLMAP is UNPINNED.  Pair p owns matches [d_pair_offsets[p], d_pair_offsets[p+1]).  Per pair:
 *   1. usable matches and records exactly as in step 1 of pxr_two_view_geometry: both pixels go through ImageToWorld, the record
 *      is (x1, y1, x2, y2) in the normalised planes of the cameras given; F relates those planes: x2^t F x1 = 0.  For an
 *      uncalibrated pair the "cameras" are conditioning transforms -- a SIMPLE_PINHOLE with a guessed or data-derived focal length
 *      and centre -- which is what keeps the 7 x 9 system well scaled: there is no Hartley step inside.  n = the usable ones, in
 *      order; n < 7: status 1.
 *   2. sample h = 0, 1, ... is seven distinct indices from the hash of pxr_two_view_geometry's step 2, used in ascending order.
 *   3. the seven-point solver: the 7 x 9 system with rows x2 (x) x1 = (x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1); its two
 *      null vectors by Gauss-Jordan with full pivoting (the largest entry, the first of equals in row-major order; vector k =
 *      (-C[:, k], e_k) of [I | C] in the permuted columns), orthonormalised by modified Gram-Schmidt in the order k = 0, 1 into N0,
 *      N1 and mixed into A = (N0 + N1) r and B = (N0 - N1) r, r = 0.70710678118654752440 (1 / sqrt 2 as a double): with F = x A + B,
 *      neither null vector being the answer on its own sends a root to infinity (that takes N0 + N1).  The cubic det(x A + B) =
 *      c3 x^3 + c2 x^2 + c1 x + c0 by expansion along row 0: for a = 0, 1, 2 with b = a + 1, c = a + 2 (mod 3) the minor of rows
 *      1, 2 is q2 x^2 + q1 x + q0, q2 = A1b A2c - A1c A2b, q1 = (A1b B2c + B1b A2c) - (A1c B2b + B1c A2b), q0 = B1b B2c - B1c B2b,
 *      and, from zero, c3 += A0a q2, c2 += (A0a q1 + B0a q2), c1 += (A0a q0 + B0a q1), c0 += B0a q0.  The coefficients are scaled
 *      by the largest; the real roots by the routine of pxr_two_view_geometry's step 3 at degree 3 (Cauchy's bound 1 + max
 *      |c_k / c_3|, the Sturm chain with rescaled remainders, 64 bisection steps on the sign-change count, 4 guarded Newton
 *      steps), ascending, at most three.  F = x A[m] + B[m] entry by entry, scaled to Frobenius norm 1 (the squares summed in
 *      index order).  No hypothesis from a pivot <= 1e-12 of the system's largest entry, a leading coefficient <= 1e-9 of the
 *      largest, or a value that is not finite.  The roots are walked one at a time, each scored over all n before the next.
 *   4. each F is scored over all n by the squared Sampson error and the thr of pxr_two_view_geometry's step 4; the largest key
 *      (inlier count, -sum min(err, thr^2), -h, -root) wins, the sum taken in index order.
 *   5. after each round of round_size samples: stop once samples done >= clamp(log(1 - confidence) / log(1 - (w2 w2) (w2 w)),
 *      min_num_trials, max_num_trials), w = best count / n, w2 = w w.  There is no floor like pxr_homography's: at ratio 0.25 it
 *      would ask for log(0.001) / log(1 - 0.25^7) = 113173 samples, above max_num_trials.  No hypothesis at all: status 2.
 *   6. local optimisation: Levenberg-Marquardt on the inliers' signed Sampson residuals x2^t F x1 / sqrt(D) (D: the denominator of
 *      step 4) over an F that is rank 2 by construction, without an SVD: of the column pairs (0, 1), (0, 2), (1, 2) of F the one
 *      (i, k) whose cross product has the largest squared norm (the first of equals; none above zero: F stays as it is); the third
 *      column is alpha c_i + beta c_k with (alpha, beta) from the 2 x 2 normal equations by Cramer's rule, alpha = (r1 g22 - r2
 *      g12) / det, beta = (g11 r2 - g12 r1) / det, g = the Gram matrix of (c_i, c_k), r = their products with the third column (det
 *      not positive: F stays); the state is (c_i, c_k, alpha, beta), of whose first six entries the one of largest magnitude is
 *      held fixed (the first of equals) while the other five and alpha, beta move additively: seven parameters.  lambda schedule,
 *      step acceptance and termination are those of pxr_homography's step 6.  F is rebuilt from the state and scaled back to
 *      Frobenius norm 1, then all n are classified again; repeated until the set stands still or lo_rounds; a refined F with fewer
 *      inliers than the one before it is dropped.
 *   7. n_inliers < max(min_num_inliers, ceil(min_inlier_ratio n)): status 3.
 * Outputs: d_status[p] 0 = F (row-major, normalised planes, Frobenius norm 1, the entry of largest magnitude positive, the first of
 * equals) written to d_F[p], left untouched otherwise; d_n_inliers[p] (0 unless status is 0); d_n_trials[p] samples drawn; per
 * match d_inlier (0 unless status is 0) and d_err (sqrt(err) max_error / thr, i.e. the Sampson distance in pixels, of the usable
 * matches of a status-0 pair; NaN elsewhere).
 * PXR_EINVAL (nothing launched): offsets not starting at 0, not monotone or not ending at n_matches, a camera index out of
 * range, an option out of range.
 * Synchronises the context's stream (offsets and cameras are validated and the pairs ordered by size on the host). */
int pxr_fundamental(pxr_ctx* ctx, int32_t n_pairs, const int64_t* d_pair_offsets, int64_t n_matches, const double* d_xy1,
                    const double* d_xy2, const int32_t* d_pair_camera, int32_t n_cameras, const int32_t* d_cam_model,
                    const double* d_cam_params, const pxr_fundamental_options* options, double* d_F, int32_t* d_status,
                    int32_t* d_n_inliers, int32_t* d_n_trials, uint8_t* d_inlier, double* d_err);
/* The same, and the HIP-event times of its kernels in milliseconds: h_kernel_ms[4] = records, compaction, hypotheses, refinement. */
int pxr_fundamental_timed(pxr_ctx* ctx, int32_t n_pairs, const int64_t* d_pair_offsets, int64_t n_matches, const double* d_xy1,
                          const double* d_xy2, const int32_t* d_pair_camera, int32_t n_cameras, const int32_t* d_cam_model,
                          const double* d_cam_params, const pxr_fundamental_options* options, double* d_F, int32_t* d_status,
                          int32_t* d_n_inliers, int32_t* d_n_trials, uint8_t* d_inlier, double* d_err, double* h_kernel_ms);

/* ---- descriptor matching (descriptors of image pairs in, mutual nearest neighbours out) --------
 * What produces the match graph (and a query's 2D-3D pairs): hloc's match_features with the NearestNeighbor matcher, whose output
 * pixsfm/util/hloc.py:read_matches_hloc reads back.  hloc is not available where this library is built, so parity with it is
 * unpinned; the specification below is this library's own and reproduces bit for bit.
 * ratio_threshold <= 0 / distance_threshold <= 0 switch the test off.  hloc's confs: "NN-mutual" (0, 0, 1), "NN-ratio" (0.8, 0, 1),
 * "NN-superpoint" (0, 0.7, 1). */
#define PXR_MATCH_MAX_DIM 512
typedef struct {
  double ratio_threshold;      /* 0   Lowe's ratio on distances: d1 <= ratio^2 d2 (squared distances)      */
  double distance_threshold;   /* 0   d1 <= dist^2                                                         */
  int32_t do_mutual_check;     /* 1   keep i -> j only if j -> i                                           */
  int32_t reserved;            /* 0                                                                        */
} pxr_match_options;
/* Writes the defaults above ("NN-mutual"). */
void pxr_match_default_options(pxr_match_options* options);

/* A batch: n_images images, image m owning rows [d_image_offsets[m], d_image_offsets[m+1]) of d_desc (n_total x dim float32,
 * row-major), and n_pairs pairs of image indices d_pairs (n_pairs x 2 int32; a pair may name one image twice).  1 <= dim <=
 * PXR_MATCH_MAX_DIM.  Descriptors are expected to be finite and L2-normalised; nothing is normalised here.  All arrays are device
 * pointers.  For a pair (a, b) with na, nb descriptors A, B:
 *   similarity  sim[i][j] = the float32 value of  s = 0; for k = 0 .. dim-1: s = fmaf(A[i][k], B[j][k], s)  -- one rounding per
 *               product, ascending k, no wider accumulator, no split over k (what v_mfma_f32_32x32x2_f32 computes when the
 *               instructions of one output tile are issued in k order on one accumulator).  k is padded with zeros to a multiple
 *               of 16, which leaves every comparison below unchanged.  A NaN similarity never wins a comparison.
 *   forward     per row i: best = the j of the largest sim[i][j], ties to the lowest j; s1 that value; s2 the largest value over
 *               j != best.  In float32 d1 = 2 (1 - s1), d2 = 2 (1 - s2).  Ratio test: d1 <= r2 d2 with r2 = (float)(ratio ratio),
 *               skipped when ratio_threshold <= 0 and, for the whole pair, when na == 1 or nb == 1.  Distance test: d1 <= t2 with
 *               t2 = (float)(dist dist), skipped when distance_threshold <= 0.  m0[i] = best if both pass, else -1.
 *   backward    the same over the columns with the same thresholds: m1[j].
 *   mutual      (do_mutual_check != 0) m0[i] stays iff m1[m0[i]] == i.
 * Outputs of pair p at d_pair_offsets[p] of the flat arrays (d_pair_offsets: n_pairs + 1 entries, the prefix sum of na over the
 * pairs, computed by the caller and checked here): d_matches0 int32 of length na (-1: no match), d_scores0 float32 of length na
 * ((s1 + 1) / 2 where matches0 >= 0, else 0 -- also where the mutual check removed the match), d_n_matches[p] the count.
 * An empty image gives an empty result (first image) or all -1 (second image).  The similarity matrix is never stored.
 * PXR_EINVAL (nothing launched, outputs untouched): image offsets not starting at 0, not monotone or not ending at n_total, a pair
 * index out of range, d_pair_offsets not that prefix sum, dim outside [1, PXR_MATCH_MAX_DIM].  Synchronises the context's stream
 * (offsets and pairs are validated on a host copy). */
int pxr_match_descriptors(pxr_ctx* ctx, int32_t n_images, const int64_t* d_image_offsets, int64_t n_total, int32_t dim,
                          const float* d_desc, int32_t n_pairs, const int32_t* d_pairs, const int64_t* d_pair_offsets,
                          const pxr_match_options* options, int32_t* d_matches0, float* d_scores0, int32_t* d_n_matches);
/* The same, and the HIP-event times of its kernels in milliseconds: h_kernel_ms[3] = tiles, columns, mutual. */
int pxr_match_descriptors_timed(pxr_ctx* ctx, int32_t n_images, const int64_t* d_image_offsets, int64_t n_total, int32_t dim,
                                const float* d_desc, int32_t n_pairs, const int32_t* d_pairs, const int64_t* d_pair_offsets,
                                const pxr_match_options* options, int32_t* d_matches0, float* d_scores0, int32_t* d_n_matches,
                                double* h_kernel_ms);

/* ---- guided descriptor matching (nearest neighbours among the candidates that agree with a pair's two-view model) --------
 * COLMAP's guided matching: once a pair has a model, it is matched again and only candidates that agree with the model compete,
 * so a look-alike off the epipolar line no longer enters the ratio test.
 * The batch is pxr_match_descriptors' plus d_xy (n_total x 2 float64, row-aligned with d_desc: the keypoint of every descriptor in
 * the frame the models live in -- the normalised plane for the E, F and H of this library) and per pair a kind (int32), a model M
 * (9 float64, row-major) and a threshold thr (float64, in the units of d_xy).  The specification is exactly pxr_match_descriptors'
 * with one added rule: AN INADMISSIBLE (i, j) NEVER WINS A COMPARISON -- it is treated exactly as a NaN similarity, forward and
 * backward.  Admissibility is computed in float64, every operation rounded once in the order written (no contraction); a
 * comparison with a NaN is false.  With (x, y) = xy_a[i], (u, v) = xy_b[j]:
 *   PXR_GUIDE_EPIPOLAR    per row     l0 = (M00 x + M01 y) + M02,  l1 = (M10 x + M11 y) + M12,  l2 = (M20 x + M21 y) + M22,
 *                                     ra = l0 l0 + l1 l1
 *                         per column  m0 = (M00 u + M10 v) + M20,  m1 = (M01 u + M11 v) + M21,  cb = m0 m0 + m1 m1
 *                         per entry   t = (u l0 + v l1) + l2,  den = ra + cb;  admissible iff den > 0 and t t <= (thr thr) den.
 *                         This is the Sampson test of pxr_two_view_geometry step 4 without the division; it may differ from that
 *                         estimator's d_inlier for an error within an ulp of thr^2.
 *   PXR_GUIDE_HOMOGRAPHY  per row     X = (M00 x + M01 y) + M02, Y and Wd likewise from rows 1 and 2 of M;  px = X / Wd,
 *                                     py = Y / Wd;  the row is valid iff Wd > 0
 *                         per entry   dx = px - u,  dy = py - v;  admissible iff valid and dx dx + dy dy <= thr thr.
 *                         This is the forward transfer error in image 2, as pxr_homography scores it (the gate is one-sided).
 * Consequences: a row with no admissible column gets -1.  A row with exactly one admissible column has s2 = -inf, d2 = +inf and so
 * passes the ratio test.  The skip of the ratio test when na == 1 or nb == 1 is unchanged.  Records belong to the pair, not the
 * image: the same image pair may appear twice with different models.  thr = +inf is allowed and admits every entry with den > 0
 * (epipolar) or a valid row (homography).  A model with an entry that is not finite is not an error: nothing is admissible for it.
 * PXR_EINVAL (nothing launched, outputs untouched): everything pxr_match_descriptors rejects, a kind outside {0, 1}, a threshold
 * that is NaN or negative (kinds and thresholds are checked on a host copy). */
#define PXR_GUIDE_EPIPOLAR   0   /* x_b^t M x_a = 0 : E or F */
#define PXR_GUIDE_HOMOGRAPHY 1   /* x_b ~ M x_a          : H  */
int pxr_match_guided(pxr_ctx* ctx, int32_t n_images, const int64_t* d_image_offsets, int64_t n_total, int32_t dim,
                     const float* d_desc, const double* d_xy, int32_t n_pairs, const int32_t* d_pairs, const int64_t* d_pair_offsets,
                     const int32_t* d_pair_kind, const double* d_pair_model, const double* d_pair_thr,
                     const pxr_match_options* options, int32_t* d_matches0, float* d_scores0, int32_t* d_n_matches);
/* The same, and the HIP-event times of its kernels in milliseconds: h_kernel_ms[4] = records, tiles, columns, mutual. */
int pxr_match_guided_timed(pxr_ctx* ctx, int32_t n_images, const int64_t* d_image_offsets, int64_t n_total, int32_t dim,
                           const float* d_desc, const double* d_xy, int32_t n_pairs, const int32_t* d_pairs,
                           const int64_t* d_pair_offsets, const int32_t* d_pair_kind, const double* d_pair_model,
                           const double* d_pair_thr, const pxr_match_options* options, int32_t* d_matches0, float* d_scores0,
                           int32_t* d_n_matches, double* h_kernel_ms);

/* ---- image retrieval (local descriptors in, a VLAD global descriptor per image and the image pairs to match out) --------
 * What picks the image pairs: hloc's pairs_from_retrieval over global descriptors (examples/sfm+loc_aachen.py; pixsfm/localize.py
 * reads its output through parse_retrieval).  hloc's retrieval models need weights and stay out; this is the classical weight-free
 * one: VLAD (Jegou et al. 2010) with intra-normalisation (Arandjelovic & Zisserman 2013) over a vocabulary learned by spherical
 * k-means from the scene's own descriptors.  Parity with hloc and with COLMAP's vocabulary tree is unpinned; the specification
 * below is this library's own and reproduces bit for bit (csrc/pxr_retrieval.hip).
 *
 * d_desc is (n_total, dim) float32 row-major, image m owning rows [d_image_offsets[m], d_image_offsets[m+1]), as for
 * pxr_match_descriptors.  1 <= dim <= PXR_VLAD_MAX_DIM, 1 <= n_clusters K <= PXR_VLAD_MAX_CLUSTERS, K dim <=
 * PXR_VLAD_MAX_GLOBAL_DIM, n_total < 2^30.  Descriptors are expected to be L2-normalised.  A row is VALID iff every entry is finite
 * and |x| <= 1; an invalid row is assigned -1 and contributes to no sum.  All d_ arrays are device pointers.  Integer sums have no
 * order; every floating-point chain has the one order stated; nothing is contracted.
 *   1 similarity  sim(a, b) = the float32 value of  s = 0; for k ascending: s = fmaf(a[k], b[k], s)  (the chain of
 *                 pxr_match_descriptors; k is padded with zeros, which changes no value).  A NaN never wins a comparison.
 *   2 assignment  assign[i] = the c with the largest sim(x_i, C_c), ties to the lowest c; -1 for an invalid row or when every
 *                 similarity is NaN.  Centroids C: (K, dim) float32.
 *   3 sums        q(x) = llrint((double)x 2^32).  S[g][c][k] = sum of q(x_i[k]) over the valid rows i of group g with assign[i] = c,
 *                 as int64; cnt[g][c] the number of such rows.  A group is the training set (training) or an image (aggregation).
 *   4 vocabulary  (pxr_vocab_train) n_train = min(n_total, max_train); the training set is rows t_j = floor(j n_total / n_train),
 *                 j < n_train.  Initial centroid c = training row floor(c n_train / K), copied.  n_iterations times: assign the
 *                 training set (2), sum (3), then for every c with cnt[c] > 0: s_k = (double)S[c][k], n2 = sum_k s_k s_k in double
 *                 in ascending k, and if n2 > 0: C[c][k] = (float)(s_k / sqrt(n2)).  A cluster that is empty or has n2 = 0 keeps
 *                 its centroid.  Outputs: d_centroids (K, dim), d_counts (K) the cnt of the last iteration, *h_n_empty the number of
 *                 zeros among them (n_iterations = 0: the initial centroids, all counts 0, *h_n_empty = K).  No random state: a
 *                 function of the input alone.  Evenly spread initial rows can be duplicates; the later duplicate loses every tie
 *                 and stays empty.  Requires K <= n_train.
 *   5 VLAD        (pxr_vlad_aggregate) per image m and centroid c: v_k = (double)S[m][c][k] 2^-32 - (double)cnt[m][c] (double)C[c][k];
 *                 b2 = sum_k v_k v_k in double, ascending k.  A block with cnt = 0 or b2 = 0 is all zeros; nne[m] is the number of
 *                 other blocks; G[m][c dim + k] = (float)(v_k / (sqrt(b2) sqrt((double)nne[m]))): every non-empty block has norm
 *                 1 / sqrt(nne), the row has norm 1.  Outputs: d_global (n_images, K dim) float32; d_assign (n_total) int32 or NULL;
 *                 d_counts (n_images, K) int32 or NULL.  An image without valid descriptors gives a zero row.
 *   6 selection   (pxr_retrieval_topk) d_query (n_query, dim), d_db (n_db, dim) float32, 1 <= dim <= PXR_VLAD_MAX_GLOBAL_DIM;
 *                 d_query_self int32[n_query] or NULL: the database index that is the query itself, -1 for none; d_mask
 *                 uint8[n_query][n_db] or NULL, 0 = excluded; min_score applies iff it is finite.  Entry (i, j) is a CANDIDATE iff it
 *                 is not masked, j != self, sim is not NaN, and sim >= (float)min_score when that applies.  Row i of the outputs:
 *                 its candidates by (sim descending, j ascending), cut at num_matched: d_top_index int32[n_query][num_matched]
 *                 padded with -1, d_top_sim float32 padded with 0, d_n_found int32[n_query].  The n_query x n_db similarity matrix
 *                 is kept in the context's workspace.
 * PXR_EINVAL (nothing launched, outputs untouched): image offsets not starting at 0, not monotone or not ending at n_total; dim,
 * n_clusters, their product or n_total out of range; n_iterations < 0; max_train < 1; n_clusters > n_train; num_matched < 1; a NaN
 * min_score.  pxr_vocab_train and pxr_vlad_aggregate synchronise the context's stream (the offsets are validated on a host copy, the
 * counts are read back); pxr_retrieval_topk only queues its kernels. */
#define PXR_VLAD_MAX_DIM 512
#define PXR_VLAD_MAX_CLUSTERS 256
#define PXR_VLAD_MAX_GLOBAL_DIM 32768
int pxr_vocab_train(pxr_ctx* ctx, int64_t n_total, int32_t dim, const float* d_desc, int32_t n_clusters, int32_t n_iterations,
                    int64_t max_train, float* d_centroids, int32_t* d_counts, int32_t* h_n_empty);
/* The same, and the HIP-event times of its kernels in milliseconds, summed over the iterations: h_kernel_ms[4] = gather (with the
 * initial centroids), assign, accumulate, update. */
int pxr_vocab_train_timed(pxr_ctx* ctx, int64_t n_total, int32_t dim, const float* d_desc, int32_t n_clusters, int32_t n_iterations,
                          int64_t max_train, float* d_centroids, int32_t* d_counts, int32_t* h_n_empty, double* h_kernel_ms);
int pxr_vlad_aggregate(pxr_ctx* ctx, int32_t n_images, const int64_t* d_image_offsets, int64_t n_total, int32_t dim,
                       const float* d_desc, int32_t n_clusters, const float* d_centroids, float* d_global, int32_t* d_assign,
                       int32_t* d_counts);
/* h_kernel_ms[3] = assign, accumulate, finalise. */
int pxr_vlad_aggregate_timed(pxr_ctx* ctx, int32_t n_images, const int64_t* d_image_offsets, int64_t n_total, int32_t dim,
                             const float* d_desc, int32_t n_clusters, const float* d_centroids, float* d_global, int32_t* d_assign,
                             int32_t* d_counts, double* h_kernel_ms);
int pxr_retrieval_topk(pxr_ctx* ctx, int32_t n_query, int32_t n_db, int32_t dim, const float* d_query, const float* d_db,
                       const int32_t* d_query_self, const uint8_t* d_mask, int32_t num_matched, double min_score,
                       int32_t* d_top_index, float* d_top_sim, int32_t* d_n_found);
/* h_kernel_ms[2] = similarity, select. */
int pxr_retrieval_topk_timed(pxr_ctx* ctx, int32_t n_query, int32_t n_db, int32_t dim, const float* d_query, const float* d_db,
                             const int32_t* d_query_self, const uint8_t* d_mask, int32_t num_matched, double min_score,
                             int32_t* d_top_index, float* d_top_sim, int32_t* d_n_found, double* h_kernel_ms);

/* ---- reconstruction evaluation on point clouds (two clouds in, nearest neighbours and voxel-averaged fractions out) --------
 * What says how good a model is: the reference's pixsfm/eval/eth3d.  triangulation.py:19-52 hands the sparse cloud and a laser
 * scan to ETH3D's multi-view-evaluation program (Schoeps et al. 2017), which reports accuracy (model against scan) and
 * completeness (scan against model) at 1 / 2 / 5 cm; localization.py:113-157 computes pose errors and their AUC (host code here:
 * pixsfm_amd/api/evaluation.py).  Both directions of the cloud half are nearest-neighbour queries followed by an average over
 * occupied voxels, so that a densely sampled wall does not outvote a sparsely sampled one.  That program's occlusion and
 * free-space meshes are not modelled and parity with it is unpinned; the specification below is this library's own and
 * reproduces bit for bit (csrc/pxr_cloud.hip).
 *
 * Clouds are (n, 3) float64 row-major device pointers.  A point is VALID iff its three coordinates are finite.  Nothing is
 * contracted; integer sums have no order.
 *   1 nearest     (pxr_cloud_nearest) 0 <= n_ref < 2^31, 0 <= n_query < 2^31, max_dist finite and > 0.
 *                 d2(q, r) = ((dx dx + dy dy) + dz dz) in float64 with dx = q.x - r.x (and so on).  r is a CANDIDATE of q iff both
 *                 are valid and d2 <= max_dist max_dist (one float64 multiplication).  Per query: the candidate with the smallest
 *                 d2, ties to the lowest reference index, in d_nn_index int32[n_query] and d_nn_dist2 float64[n_query]; without a
 *                 candidate -1 and +inf.  A function of the two arrays alone: equal to the brute-force search bit for bit,
 *                 whatever the order the grid inside is built or walked in.
 *   2 voxels      (pxr_cloud_voxel_fractions) 0 <= n < 2^30, 1 <= n_tol <= PXR_CLOUD_MAX_TOLERANCES, tolerances finite and > 0,
 *                 voxel_size v finite and >= 0.  The valid point i lies in voxel (floor(x / v), floor(y / v), floor(z / v)), division
 *                 and floor in float64; within_t(i) iff d_dist2[i] <= t t (the +inf of a query without a candidate never is).  Per
 *                 occupied voxel: n_v points, w_v[t] of them within, q_v[t] = llrint(((double)w_v[t] / (double)n_v) 2^32).
 *                 h_fraction[t] = ((double)(sum over the voxels of q_v[t], as int64)) 2^-32 / (double)n_voxels; *h_n_voxels the
 *                 number of occupied voxels.  Without a valid point: NaN and 0.  v = 0: every valid point is its own voxel, the
 *                 result is exactly (double)W[t] / (double)n_valid.
 * PXR_EINVAL (nothing launched, outputs untouched): a size, max_dist, a tolerance, n_tol or voxel_size outside the limits above; a
 * NULL array of a non-empty cloud.  One check is made ON THE DEVICE and therefore AFTER the launch: every voxel component must
 * satisfy |floor(x / v)| < 2^20 (the key packs into 63 bits); otherwise pxr_cloud_voxel_fractions returns PXR_EINVAL with
 * h_fraction and h_n_voxels untouched.  Both calls take their scratch from the context's workspace and queue on its stream;
 * pxr_cloud_nearest only queues its kernels, pxr_cloud_voxel_fractions synchronises the stream to return its host values. */
#define PXR_CLOUD_MAX_TOLERANCES 8
int pxr_cloud_nearest(pxr_ctx* ctx, int64_t n_ref, const double* d_ref_xyz, int64_t n_query, const double* d_query_xyz,
                      double max_dist, int32_t* d_nn_index, double* d_nn_dist2);
/* The same, and the HIP-event times of its kernels in milliseconds: h_kernel_ms[2] = grid (count, scan, fill), query. */
int pxr_cloud_nearest_timed(pxr_ctx* ctx, int64_t n_ref, const double* d_ref_xyz, int64_t n_query, const double* d_query_xyz,
                            double max_dist, int32_t* d_nn_index, double* d_nn_dist2, double* h_kernel_ms);
int pxr_cloud_voxel_fractions(pxr_ctx* ctx, int64_t n, const double* d_xyz, const double* d_dist2, double voxel_size, int32_t n_tol,
                              const double* h_tolerances, double* h_fraction, int64_t* h_n_voxels);
/* h_kernel_ms[2] = insert, reduce. */
int pxr_cloud_voxel_fractions_timed(pxr_ctx* ctx, int64_t n, const double* d_xyz, const double* d_dist2, double voxel_size,
                                    int32_t n_tol, const double* h_tolerances, double* h_fraction, int64_t* h_n_voxels,
                                    double* h_kernel_ms);

/* ---- incremental mapping: visibility (triangulated tracks in, per-image scores and 2D-3D pairs out) ----
 * The stage of the reference's main entry point that produces poses: PixSfM.reconstruction (pixsfm/refine_hloc.py:133-146)
 * hands it to hloc.reconstruction.main, i.e. COLMAP's incremental mapper.  The arithmetic of a mapper is the stages above
 * (pxr_two_view_geometry, pxr_triangulate_tracks, pxr_absolute_pose, pxr_ba_solve_geometric); this is the device step between
 * triangulation and registration, for all candidate images at once: [upstream COLMAP 3.8] IncrementalMapper::FindNextImages
 * with VisibilityPyramid's score, and the 2D-3D gathering at the head of IncrementalMapper::RegisterNextImage -- as remembered,
 * parity unpinned.  All arrays are device pointers.
 *   view                 tracks in CSR form over the observations, images and cameras (qvec / tvec / cam_model / cam_params are not read)
 *   d_obs_track          [n_obs] the track of every observation
 *   d_image_obs_offsets  [n_images + 1], d_image_obs [n_obs]: the image-major transpose of the CSR -- image i owns the
 *                        observation indices d_image_obs[offsets[i] .. offsets[i+1]), ascending
 *   d_xyz, d_status      [n_tracks][3], [n_tracks] exactly as pxr_triangulate_tracks writes them
 *   d_image_mask         [n_images] non-zero = candidate
 *   d_cam_size           [n_cameras][2] width, height in pixels
 *   pyramid_levels       L, 1 <= L <= 6
 * Observation o of a candidate image is VISIBLE iff d_status[d_obs_track[o]] == 0, that track's xyz is finite and the
 * observation's xy is finite.  Its finest cell is cx = clamp((int)floor(x 2^L / width), 0, 2^L - 1), cy likewise with the
 * height; at level l = 1 .. L it occupies cell (cx >> (L - l), cy >> (L - l)).
 * Outputs: d_n_visible[i] the visible observations of image i; d_score[i] = sum over l of 4^l (distinct occupied cells at
 * level l); both 0 for an image that is masked out.  d_corr_offsets [n_images + 1] = the exclusive scan of d_n_visible;
 * d_corr_obs / d_corr_xy / d_corr_xyz (capacity n_obs rows) hold, for every image in turn, its visible observations in
 * ascending observation order: the observation index, its keypoint, the point of its track; *h_n_corr their number.
 * (n_images, d_corr_offsets, *h_n_corr, d_corr_xy, d_corr_xyz, view->d_image_camera) is an argument set of pxr_absolute_pose:
 * an image that is no candidate is a query without correspondences.
 * PXR_EINVAL (nothing launched on the outputs, which stay untouched): either offsets array not monotone or not ending at n_obs,
 * d_image_obs not that transpose, a track / image / camera index out of range, a camera size that is not positive,
 * pyramid_levels out of range.  Synchronises the context's stream. */
int pxr_mapper_visibility(pxr_ctx* ctx, const pxr_tri_view* view, const int64_t* d_obs_track, const int64_t* d_image_obs_offsets,
                          const int64_t* d_image_obs, const double* d_xyz, const int32_t* d_status, const uint8_t* d_image_mask,
                          const int32_t* d_cam_size, int32_t pyramid_levels, int32_t* d_n_visible, int64_t* d_score,
                          int64_t* d_corr_offsets, int64_t* d_corr_obs, double* d_corr_xy, double* d_corr_xyz, int64_t* h_n_corr);
/* The same, and the HIP-event times of its kernels in milliseconds: h_kernel_ms[4] = validation, count, scan, write. */
int pxr_mapper_visibility_timed(pxr_ctx* ctx, const pxr_tri_view* view, const int64_t* d_obs_track,
                                const int64_t* d_image_obs_offsets, const int64_t* d_image_obs, const double* d_xyz,
                                const int32_t* d_status, const uint8_t* d_image_mask, const int32_t* d_cam_size,
                                int32_t pyramid_levels, int32_t* d_n_visible, int64_t* d_score, int64_t* d_corr_offsets,
                                int64_t* d_corr_obs, double* d_corr_xy, double* d_corr_xyz, int64_t* h_n_corr,
                                double* h_kernel_ms);

/* ---- batched map localization: covisibility, clusters, 2D-3D pairs (a map and retrieved images in, pxr_absolute_pose's input out) ----
 * The glue of the reference's second entry point, pixsfm/localize.py:main, which takes it from hloc: pairs_from_covisibility (as
 * pixsfm/eval/eth3d/utils.py:73 calls it), localize_sfm.do_covisibility_clustering and the gathering of
 * localize_sfm.pose_from_cluster -- as remembered, parity unpinned; the definitions below are the
 * specification.  All arrays are device pointers unless named h_.  Every output is an integer or a copied double: two calls give
 * the same bits.  PXR_EINVAL always means: nothing was launched on the outputs, which stay untouched.  Every entry point
 * synchronises the context's stream (offsets are validated on host copies, index ranges by a kernel whose flag is read back). */
#define PXR_MAX_COVIS_IMAGES 8192 /* the count matrix is dense: 256 MB of int32 at this limit */
#define PXR_MAX_COVIS_MATCHED 256 /* partners per image */
#define PXR_MAX_LOC_ENTRIES 64    /* retrieved images of a query, entries of a problem: one wavefront, one 64-bit mask */

/* Covisibility counts of a map whose tracks are given as in pxr_tri_view (d_track_offsets [n_tracks + 1], d_obs_image [n_obs]);
 * d_track_mask [n_tracks] uint8 or NULL (= all tracks).
 *   d_count [n_images][n_images] int32, zeroed by the call: for every track whose mask is non-zero and every ORDERED pair (a, b)
 *   of its observations with image(a) != image(b), count[image(a)][image(b)] += 1.  The diagonal stays 0 and the matrix is
 *   symmetric.  This is hloc's count -- for every keypoint of image i that has a point, every element of that point's track in
 *   another image j adds one -- so an image that sees a track twice counts twice.
 *   d_topk_index, d_topk_count [n_images][num_matched] int32, d_n_topk [n_images] int32: row i holds the n = min(num_matched,
 *   number of j with count[i][j] > 0) images of largest count in the order (count descending, image index ascending) -- hloc
 *   leaves ties to argpartition, here they are defined -- with their counts; d_n_topk[i] = n; the entries from n on are -1
 *   (index) and 0 (count).  All three may be NULL: then only the counts are written and num_matched is ignored.
 * Limits: n_images <= PXR_MAX_COVIS_IMAGES, 1 <= num_matched <= PXR_MAX_COVIS_MATCHED, n_obs < 2^31.  A count is an int32 sum
 * that is not checked: an entry wraps around once two images share 2^31 ordered pairs, which takes e.g. one track that both
 * see 46341 times each -- far from any map, but tracks that long are the caller's to keep out (d_track_mask).
 * PXR_EINVAL: a limit exceeded; offsets not starting at 0, not monotone or not ending at n_obs; an image index out of range. */
int pxr_covisibility(pxr_ctx* ctx, int32_t n_images, int64_t n_tracks, const int64_t* d_track_offsets, int64_t n_obs,
                     const int32_t* d_obs_image, const uint8_t* d_track_mask, int32_t num_matched, int32_t* d_count,
                     int32_t* d_topk_index, int32_t* d_topk_count, int32_t* d_n_topk);
/* The same, and the HIP-event times of its kernels in milliseconds: h_kernel_ms[3] = validation, count, top-k. */
int pxr_covisibility_timed(pxr_ctx* ctx, int32_t n_images, int64_t n_tracks, const int64_t* d_track_offsets, int64_t n_obs,
                           const int32_t* d_obs_image, const uint8_t* d_track_mask, int32_t num_matched, int32_t* d_count,
                           int32_t* d_topk_index, int32_t* d_topk_count, int32_t* d_n_topk, double* h_kernel_ms);

/* Covisibility clusters of the retrieved images of a batch of queries.  d_count as pxr_covisibility writes it (symmetric; row
 * i of the entry's own image is what is read); query q owns the entries [d_ret_offsets[q], d_ret_offsets[q+1]) of d_ret [n_ret],
 * int32 map image indices in retrieval rank order (an image may appear twice).
 *   Two entries of one query are CONNECTED iff they name the same image or count[i][j] > 0; the clusters are the connected
 *   components of that relation restricted to the query's list -- hloc's breadth-first search, which only walks through frames
 *   of the list.  They are numbered by (size descending, rank of their first member ascending), size counting list entries:
 *   hloc's stable sorted(clusters, key=len, reverse=True) over discovery order.
 *   d_cluster [n_ret] int32 = the cluster number of every entry; d_n_clusters [n_queries] int32 (0 for a query without entries).
 * PXR_EINVAL: more than PXR_MAX_LOC_ENTRIES entries in a query; offsets not starting at 0, not monotone or not ending at n_ret;
 * an image index out of range; n_images > PXR_MAX_COVIS_IMAGES. */
int pxr_covisibility_clusters(pxr_ctx* ctx, int32_t n_images, const int32_t* d_count, int32_t n_queries, const int64_t* d_ret_offsets,
                              int64_t n_ret, const int32_t* d_ret, int32_t* d_cluster, int32_t* d_n_clusters);
/* The same, and the HIP-event times of its kernels in milliseconds: h_kernel_ms[2] = validation, clusters. */
int pxr_covisibility_clusters_timed(pxr_ctx* ctx, int32_t n_images, const int32_t* d_count, int32_t n_queries,
                                    const int64_t* d_ret_offsets, int64_t n_ret, const int32_t* d_ret, int32_t* d_cluster,
                                    int32_t* d_n_clusters, double* h_kernel_ms);

/* The 2D-3D pairs of a batch of localization problems, out of the matcher's device output: the device form of the gathering of
 * pose_from_cluster.  A PROBLEM is one (query, cluster), or one query with its whole list; problem p owns the entries
 * [d_problem_offsets[p], d_problem_offsets[p+1]) of d_problem_pair [n_entries], int32 indices into the matcher's pair list in
 * visiting (retrieval rank) order.
 *   from pxr_match_descriptors: n_pairs, d_pairs [n_pairs][2] (first image = the query, second = the database image, indices
 *   into the descriptor set), d_pair_offsets [n_pairs + 1], d_matches0 [n_rows] (per query keypoint the database keypoint or
 *   a negative value), n_set_images, d_image_offsets [n_set_images + 1] ending at n_total
 *   per keypoint of the set: d_kp_xy [n_total][2]; d_kp_point [n_total] int64, the row of d_xyz [n_points][3] (negative: no point)
 * Per problem and per query keypoint k, ascending, the entries j are visited in order: m = matches0[pair_offsets[pair_j] + k],
 * and for m >= 0, pid = kp_point[image_offsets[db_j] + m].  The pair (k, pid) is emitted iff pid >= 0, xyz[pid] and the keypoint
 * kp_xy[image_offsets[query] + k] are finite, and no earlier entry j' < j of the problem gave the same pid for k: within a
 * keypoint the order is first appearance.
 * Outputs: d_corr_offsets [n_problems + 1] int64; per emitted pair d_corr_kp int32 (k), d_corr_point int64 (pid), d_corr_xy
 * (the keypoint), d_corr_xyz (the point), each with room for the sum over the entries of their pair's rows; *h_n_corr their
 * number.  (n_problems, d_corr_offsets, *h_n_corr, d_corr_xy, d_corr_xyz) is an argument set of pxr_absolute_pose.
 * PXR_EINVAL: any offsets array not starting at 0, not monotone or not ending at its total; a pair, image, keypoint (a match
 * beyond the database image's keypoints) or point index out of range; entries of one problem that do not share their first
 * image; more than PXR_MAX_LOC_ENTRIES entries in a problem; a pair whose rows differ from its first image's keypoint count. */
int pxr_localization_pairs(pxr_ctx* ctx, int32_t n_problems, const int64_t* d_problem_offsets, int64_t n_entries,
                           const int32_t* d_problem_pair, int32_t n_pairs, const int32_t* d_pairs, const int64_t* d_pair_offsets,
                           int64_t n_rows, const int32_t* d_matches0, int32_t n_set_images, const int64_t* d_image_offsets,
                           int64_t n_total, const double* d_kp_xy, const int64_t* d_kp_point, int64_t n_points, const double* d_xyz,
                           int64_t* d_corr_offsets, int32_t* d_corr_kp, int64_t* d_corr_point, double* d_corr_xy, double* d_corr_xyz,
                           int64_t* h_n_corr);
/* The same, and the HIP-event times of its kernels in milliseconds: h_kernel_ms[3] = count (with the index checks), scan, write. */
int pxr_localization_pairs_timed(pxr_ctx* ctx, int32_t n_problems, const int64_t* d_problem_offsets, int64_t n_entries,
                                 const int32_t* d_problem_pair, int32_t n_pairs, const int32_t* d_pairs, const int64_t* d_pair_offsets,
                                 int64_t n_rows, const int32_t* d_matches0, int32_t n_set_images, const int64_t* d_image_offsets,
                                 int64_t n_total, const double* d_kp_xy, const int64_t* d_kp_point, int64_t n_points,
                                 const double* d_xyz, int64_t* d_corr_offsets, int32_t* d_corr_kp, int64_t* d_corr_point,
                                 double* d_corr_xy, double* d_corr_xyz, int64_t* h_n_corr, double* h_kernel_ms);

/* ---- batched query bundle adjustment (QBA: localization/src/single_query_bundle_optimizer.h:91-222, query_bundle_optimizer.h:
 * 114-151) -- the poses of a whole batch of queries refined in ONE launch, a workgroup per query, the trust-region loop inside
 * the kernel.  Per query it is the problem pxr_ba_solve solves for one image whose points are all constant
 * and whose intrinsics are constant: FeatureReferenceCostFunctor blocks, the pose on the quaternion manifold plus the
 * translation, six tangent unknowns.  All arrays are device pointers unless named h_.
 *   queries: n_queries, d_query_offsets [n_queries + 1] int64 into the residual-block arrays (a query may be empty)
 *   per residual block, n_obs in total: d_obs_patch int64 (arena index), d_xyz [n_obs][3] (the block's constant point),
 *     d_refs [n_obs][C] (its reference descriptor).  One row per (correspondence, reference descriptor): a correspondence with two
 *     references is two rows with the same patch and point.
 *   cameras: d_query_camera [n_queries] int32, n_cameras, d_cam_model [n_cameras], d_cam_params [n_cameras][PXR_KPAD]; constant
 *   poses: d_qvec [n_queries][4] (w first; normalised by the call), d_tvec [n_queries][3], refined IN PLACE
 * Cost per block: exactly pxr_ba_eval's -- the bicubic descriptor at WorldToPixel (use_float_simd as there), L2 normalisation
 * with its chain rule when cfg->l2_normalize, minus the reference; cfg->check_bounds as there, i.e. without effect, because every
 * block has a reference descriptor (see pxr_interp_cfg).
 * Loop: [upstream Ceres 2.1] trust-region Levenberg-Marquardt as pxr_ba_solve states it (oracle/pxo_solve.c with one image and
 * every point constant): Jacobi scaling from the initial linearisation when options->jacobi_scaling, the LM diagonal clamped to
 * [min_lm_diagonal, max_lm_diagonal], the robustifier's corrector, a 6 x 6 Cholesky step, acceptance by min_relative_decrease,
 * the radius update (initial_radius, min_radius, max_radius), max_consecutive_invalid_steps, the function / gradient / parameter
 * tolerances and max_iterations.  A trial pose whose cost is not finite is a rejected step.  IGNORED fields of pxr_lm_options:
 * use_inner_iterations, inner_iteration_tolerance (no point moves), linear_solver, max_linear_solver_iterations, eta,
 * linear_r_tolerance (the system is 6 x 6).  Iteration callbacks are NOT called: the loop runs inside the kernel, as in
 * pxr_ka_solve.
 * h_summaries [n_queries] (host): iterations, num_successful, termination, num_camera_unknowns = 6, num_point_unknowns = 0,
 * initial_cost, final_cost, final_radius, accumulation = 2 (ordered sums), total_ms = the HIP-event time of the solve kernel (the
 * same value for every query); the other fields are 0.
 *   an empty query keeps its pose: iterations = 0, PXR_TERM_CONVERGENCE, costs 0
 *   a query whose initial cost is not finite keeps its pose: iterations = 0, PXR_TERM_FAILURE
 * A query's outputs -- pose and summary except total_ms -- are a function of that query's own blocks, camera, pose and the options
 * alone: the same bits alone, in any batch, at any position of it and on every run (fixed-order sums; the lanes a block runs on
 * depend on nothing but its position in the query).
 * Storage and channels: fp16 / fp32 / fp64 arenas with C = 128 or 64 (what pxr_ba_eval dispatches beyond the cost maps); anything
 * else returns PXR_EUNSUPPORTED.
 * PXR_EINVAL (every output untouched, the summaries included): a NULL argument, offsets not starting at 0, not monotone or not
 * ending at n_obs, a camera index out of range (both checked on host copies), a patch index outside the arena (checked by a kernel
 * whose flag is read back before the solve starts), an arena with an upsampling factor, n_obs >= 2^31.
 * Synchronises the context's stream. */
int pxr_query_ba_solve(pxr_ctx* ctx, pxr_arena* arena, int32_t n_queries, const int64_t* d_query_offsets, int64_t n_obs,
                       const int64_t* d_obs_patch, const double* d_xyz, const double* d_refs, const int32_t* d_query_camera,
                       int32_t n_cameras, const int32_t* d_cam_model, const double* d_cam_params, double* d_qvec, double* d_tvec,
                       const pxr_interp_cfg* cfg, const pxr_loss* loss, const pxr_lm_options* options, pxr_lm_summary* h_summaries);
/* The same, and the HIP-event time of the solve kernel in milliseconds: h_kernel_ms[1]. */
int pxr_query_ba_solve_timed(pxr_ctx* ctx, pxr_arena* arena, int32_t n_queries, const int64_t* d_query_offsets, int64_t n_obs,
                             const int64_t* d_obs_patch, const double* d_xyz, const double* d_refs, const int32_t* d_query_camera,
                             int32_t n_cameras, const int32_t* d_cam_model, const double* d_cam_params, double* d_qvec, double* d_tvec,
                             const pxr_interp_cfg* cfg, const pxr_loss* loss, const pxr_lm_options* options,
                             pxr_lm_summary* h_summaries, double* h_kernel_ms);

/* ---- BA reference extraction -----------------------------------------------------------
 * Replaces ReferenceExtractor::Run (bundle_adjustment/src/reference_extractor.h:125-318) +
 * RobustMeanIRLS (base/src/irls_optim.h:24-71) for N_NODES = 1: per point, descriptors of all
 * its observations at the CURRENT projection (view->d_refs is ignored), IRLS robust mean with
 * `loss` (ReferenceConfig.loss, Cauchy(0.25)) and `iters` (100) iterations, reference = the
 * observation descriptor closest to the robust mean.  Outputs (device): d_refs_out
 * [n_points][C], d_ref_obs_out [n_points] (index of the chosen observation, -1 if the point has
 * none), optional d_robust_mean_out [n_points][C].  Channels: 128, 64, and 3 / 1 (image intensities; the registered
 * FeatureReferenceBundleOptimizer cases (128,1) (64,1) (3,1) (1,1), feature_reference_bundle_optimizer.h:13-16 -- below 8
 * channels the interpolation is the scalar Ceres bicubic the reference falls back to, interpolation.h:222-268). */
int pxr_ba_compute_references(pxr_ctx* ctx, pxr_arena* arena, const pxr_ba_view* view,
                              const pxr_interp_cfg* cfg, const pxr_loss* loss, int iters,
                              double* d_refs_out, int64_t* d_ref_obs_out, double* d_robust_mean_out,
                              double* d_obs_desc_out /* NULL, or [n_obs][C]: the per-observation descriptors
                                                        (ReferenceConfig::keep_observations, reference_extractor.h:60,259-265) */);

/* ---- cost maps (the reference's low-memory BA) -----------------------------
 * Replaces CostMapExtractor::RunSubset / FillPointCostmap (bundle_adjustment/src/costmap_extractor.h:177-358)
 * for CostMapConfig.upsampling_factor = 1, compute_cross_derivative = false on sparse patches: cost map
 * first_out + i of `costmaps` (C = 3 [cost, dcost/dr, dcost/dc] when as_gradientfield, else 1 [cost]; H, W as
 * the features; any dtype -- the reference's binding uses the features', bundle_adjustment/bindings.cc:21)
 * = featuremetric error of every texel of feature patch d_patch[i] against reference descriptor
 * d_refs[d_ref_index[i]] (the observation's 3D point), robustified with `loss` (CostMapConfig.loss), central
 * differences in the storage type, optional sqrt (CostMapConfig.apply_sqrt); corner and scale are copied from
 * the feature patch.  The cost-map BA (CostMapBundleOptimizer, costmap_bundle_optimizer.h) is then
 * pxr_ba_solve on the `costmaps` arena with view->d_refs = NULL and cfg->l2_normalize = 0
 * (bundle_adjustment/main.py:270): the residual block is the interpolated 3- (or 1-) channel texel. 
 * Feature channels: 128, 64, and 3 / 1 (image intensities; costmap_extractor.h:35-37 registers 128 and 3) -- one lane per
 * texel there.  pxr_costmap_extract_ex's interpolating branch (upsampling_factor != 1, cross derivative) takes 128 / 64 only. */
int pxr_costmap_extract(pxr_ctx* ctx, pxr_arena* features, pxr_arena* costmaps, int64_t first_out, int64_t n,
                        const int64_t* d_patch, const int32_t* d_ref_index, const double* d_refs,
                        const pxr_loss* loss, int as_gradientfield, int apply_sqrt);

/* The general form: CostMapConfig.upsampling_factor and compute_cross_derivative (costmap_extractor.h:42-45).  With
 * upsampling_factor = 1 and no cross derivative this IS pxr_costmap_extract.  Otherwise the reference interpolates
 * (FillPointCostmap :280-284, :341-345): output texel (y, x) = the features evaluated at the local patch coordinates
 * (x, y) / upsampling_factor by PatchInterpolator::EvaluateLocal under `cfg` (bicubic; L2 normalisation applies here),
 * 4 channels [cost, dcost/dr, dcost/dc, d2cost/drdc] with the cross derivative (:304-317).  The `costmaps` arena must be
 * int(H (f + 1e-6)) x int(W (f + 1e-6)) x {1, 3, 4} (CreateShallowCostmapFSet :385-390, GetEffectiveChannels :52-61) and
 * receives the upsampling factor (SetUpsamplingFactor :399; pxr_arena_set_upsampling), which the cost-map BA's coordinate
 * transform u = (x sx - 0.5 - x0) f then honours (featurepatch.h:250-255).  Note that the reference's own
 * CostMapBundleOptimizer takes 1 or 3 channels only (costmap_bundle_optimizer.h:9-14): 4-channel maps can be produced,
 * not optimised over -- here too (pxr_ba_eval rejects them). */
int pxr_costmap_extract_ex(pxr_ctx* ctx, pxr_arena* features, pxr_arena* costmaps, int64_t first_out, int64_t n,
                           const int64_t* d_patch, const int32_t* d_ref_index, const double* d_refs,
                           const pxr_loss* loss, int as_gradientfield, int apply_sqrt, const pxr_interp_cfg* cfg,
                           double upsampling_factor, int compute_cross_derivative);
/* FeaturePatch::SetUpsamplingFactor / UpsamplingFactor (features/src/featurepatch.h:208-216) for every patch of an arena;
 * 1 by default.  Only cost-map arenas (1 / 3 channels) may carry another value. */
int pxr_arena_set_upsampling(pxr_arena* a, double upsampling_factor);
double pxr_arena_upsampling(pxr_arena* a);

/* PatchInterpolator::Evaluate / InterpolateNodes, batched (A5, features/src/patch_interpolator.h:86-135;
 * `_features.PatchInterpolator(config).interpolate_nodes(fpatch, xy)`, features/bindings.cc): the normalised
 * bicubic descriptor of arena patch d_patch[i] at keypoint d_kp[i] (COLMAP image coordinates) into
 * d_desc [n][C], and optionally its Jacobian with respect to the keypoint, d_J [n][C][2] (d/dx, d/dy).
 * Channels 128, 64, 3, 1 (pxr_nearest_references below: the same). */
int pxr_interpolate(pxr_ctx* ctx, pxr_arena* arena, const pxr_interp_cfg* cfg, int64_t n, const double* d_kp,
                    const int64_t* d_patch, double* d_desc, double* d_J /* may be NULL */);

/* FindNearestReferences (localization/src/nearest_references.h:20-52): for each 2D-3D correspondence i the
 * query descriptor f(patch[d_patch[i]], d_kp[i]) is compared with its candidates -- rows
 * d_cand_index[d_cand_ptr[i] .. d_cand_ptr[i+1]) of d_cand_desc [*][C] (d_cand_index NULL: the rows
 * themselves), i.e. the observation descriptors of its 3D point (Reference::observations).  d_best[i] =
 * row of the nearest candidate (squared L2, first minimum wins; -1 without candidates), optional
 * d_best_dist[i], optional copy of the winner into d_out_desc [n][C]. */
int pxr_nearest_references(pxr_ctx* ctx, pxr_arena* arena, const pxr_interp_cfg* cfg, int64_t n,
                           const double* d_kp, const int64_t* d_patch, const int64_t* d_cand_ptr,
                           const int64_t* d_cand_index, const double* d_cand_desc, int64_t* d_best,
                           double* d_best_dist, double* d_out_desc);

/* ---- KA ---------------------------------------------------------------------------------
 * Batched replacement of FeatureMetricKeypointOptimizer::RunParallel / RunSubset
 * (keypoint_adjustment/src/featuremetric_keypoint_optimizer.h:69-137) for the flat edge list
 * the host builds from TopologicalKeypointOptimizer::SetUp + AddIntraResiduals
 * (topological_keypoint_optimizer.h:97-175, featuremetric_keypoint_optimizer.h:158-202):
 * one residual block per edge, r = f(patch[src], kp[src]) - f(patch[dst], kp[dst])
 * (FeatureMetric2DCostFunctor, residuals/src/featuremetric.h:44-63), ScaledLoss(loss, weight).
 * Sub-problems (ParallelOptimizer groups, base/src/parallel_optimizer.h:77-211) are given in
 * CSR form; each is solved by ONE workgroup that runs the whole bounded LM loop
 * (KeypointOptimizerBase::SolveProblem + ParameterizeKeypoints, keypoint_optimizer.h:77-157)
 * on the device.  All arrays are device pointers; d_kp is refined IN PLACE. */
typedef struct {
  int64_t n_nodes;
  double* d_kp;                   /* [n_nodes][2] keypoints in COLMAP image coordinates   */
  const int64_t* d_node_patch;    /* [n_nodes] patch index in the arena                   */
  const uint8_t* d_node_const;    /* [n_nodes] 1 = constant (roots, KeypointAdjustmentSetup); 2 = variable WITHOUT box
                                     bounds: a match destination outside RunSubset's nodes_in_problem, which
                                     ParameterizeKeypoints never visits (keypoint_optimizer.h:117); 0 = variable */
  int64_t n_edges;
  const int32_t* d_edge_src;      /* [n_edges]                                            */
  const int32_t* d_edge_dst;
  const double* d_edge_w;         /* ScaledLoss weight (similarity if weight_by_sim, else 1) */
  int32_t n_problems;
  const int64_t* d_prob_node_ptr; /* [n_problems + 1] into d_prob_nodes (ascending node ids) */
  const int32_t* d_prob_nodes;
  const int64_t* d_prob_edge_ptr; /* [n_problems + 1] into d_prob_edges                    */
  const int32_t* d_prob_edges;
  /* Unary reference terms (localization QKA, A8): one FeatureReference2DCostFunctor block
   * r = f(patch[node], kp[node]) - ref per entry (residuals/src/feature_reference.h:20-60,
   * localization/src/query_keypoint_optimizer.h:122-139); several entries may name the same
   * node (stacked correspondences, single_query_keypoint_optimizer.h:124-170).  n_unary = 0
   * (and NULL pointers) for plain KA. */
  int64_t n_unary;
  const int32_t* d_unary_node;    /* [n_unary]                                            */
  const double* d_unary_ref;      /* [n_unary][C] reference descriptors                   */
  const double* d_unary_w;        /* [n_unary] ScaledLoss weight; NULL = 1                */
  const int64_t* d_prob_unary_ptr;/* [n_problems + 1] into d_prob_unary                   */
  const int32_t* d_prob_unary;
  /* Optional (NULL: every sub-problem is a Ceres problem of its own, as above).  d_prob_group[i] = id of the label group --
   * the ceres::Problem of the reference, ONE trust region / line search / termination (keypoint_optimizer.h:77-104) -- that
   * sub-problem i is a CHUNK of.  The chunks of a group are consecutive sub-problems and share no variable (whole tracks
   * each); every chunk still gets its own workgroup, and the group's scalars -- cost, model cost change, probe costs, step
   * norms -- are summed over its workgroups, so that a group of 1000 keypoints (configs/low_memory.yaml:
   * max_kps_per_problem 1000) runs on 20 workgroups instead of one with the decisions of ONE problem.  Per-chunk summaries
   * then carry the group's iteration counts and the chunk's part of the costs.  A group may have at most as many chunks as
   * the launch keeps resident (~448 on an MI355X; larger groups: PXR_EUNSUPPORTED). */
  const int32_t* d_prob_group;    /* [n_problems] non-decreasing group ids, or NULL          */
} pxr_ka_view;

/* Per-edge evaluation for parity checks: d_cost [n_edges] = 0.5 w rho(|r|^2); optional
 * d_r [n_edges][C], d_J1 / d_J2 [n_edges][C][2] (dr/dkp_src, dr/dkp_dst, row-major). */
int pxr_ka_eval(pxr_ctx* ctx, pxr_arena* arena, const pxr_ka_view* view, const pxr_interp_cfg* cfg,
                const pxr_loss* loss, double* d_cost, double* d_r, double* d_J1, double* d_J2);

/* Solve every sub-problem.  bound: KeypointOptimizerOptions::bound (4.0,
 * keypoint_adjustment/main.py:78).  h_summaries: NULL or [n_problems] per-problem summaries;
 * *total accumulates them like AccumulateSummaries (util/src/statistics.h:131-160). */
int pxr_ka_solve(pxr_ctx* ctx, pxr_arena* arena, const pxr_ka_view* view, const pxr_interp_cfg* cfg,
                 const pxr_loss* loss, double bound, const pxr_lm_options* options,
                 pxr_lm_summary* h_summaries, pxr_lm_summary* total);

/* ---- match-graph labelling (host code) ----------------------------------
 * ComputeTrackLabels / ComputeScoreLabels / ComputeRootLabels (base/src/graph.cc:126-256), the
 * pre-processing KeypointAdjuster.refine runs before the optimisers (keypoint_adjustment/main.py:111-118),
 * over flat HOST arrays: node_image [n_nodes] (FeatureNode::image_id), edges in Graph order (for node in
 * nodes: for match in node.out_matches) as edge_src / edge_dst / edge_sim.  Sequential by construction
 * (every union depends on the earlier ones), native so that it does not become the bottleneck. */
int pxr_graph_track_labels(int64_t n_nodes, const int32_t* node_image, int64_t n_edges,
                           const int64_t* edge_src, const int64_t* edge_dst, const double* edge_sim,
                           int64_t* track_labels /* [n_nodes] */, int64_t* n_tracks_out /* may be NULL */);
int pxr_graph_score_labels(int64_t n_nodes, int64_t n_edges, const int64_t* edge_src,
                           const int64_t* edge_dst, const double* edge_sim, const int64_t* track_labels,
                           double* scores /* [n_nodes] */);
int pxr_graph_root_labels(int64_t n_nodes, const int64_t* track_labels, const double* scores,
                          uint8_t* is_root /* [n_nodes] */);
/* The same three labellings ON THE DEVICE for a flat graph that already lives in HBM (csrc/pxr_graph_gpu.hip): connected
 * components by label hooking, one wavefront per component replaying the reference's ordered, image-constrained
 * union-find, scores summed in the reference's order (bit-identical), roots by per-track maximum.  All arrays are device
 * pointers; matches in Graph order (ascending source node); d_scores / d_is_root may be NULL (roots need scores). */
int pxr_graph_labels_device(pxr_ctx* ctx, int64_t n_nodes, const int32_t* d_node_image, int64_t n_edges,
                            const int64_t* d_edge_src, const int64_t* d_edge_dst, const double* d_edge_sim,
                            int64_t* d_track_labels, double* d_scores, uint8_t* d_is_root, int64_t* h_n_tracks);
/* ---- BA problem construction (host code; A16, A17) ----------------------------------------------------------
 * BundleOptimizer::SetUp on a flat scene (bundle_adjustment/src/bundle_optimizer.h:139-165): AddImageToProblem for the
 * images of the setup (:247-275, incl. the min_track_length filter), AddPointToProblem for the extra variable /
 * constant points (:279-317: their observations in images OUTSIDE the setup, whose cameras become constant unless
 * residuals of setup images use them), FeatureReferenceBundleOptimizer::AddResiduals
 * (feature_reference_bundle_optimizer.h:90-149), then ParameterizePoints / Images / Cameras (:335-453).
 * Scene (HOST arrays, what a binding reads off colmap::Reconstruction): images 0 .. n_images-1 with their camera and
 * their points2D (rows p2d_ptr[i] .. p2d_ptr[i+1] of p2d_point3D; -1 = no 3D point), cameras (COLMAP model id), points
 * 0 .. n_points-1 with their tracks in Track().Elements() order (track_ptr / track_image / track_p2d);
 * has_patch [n_p2d] (NULL: every observation has a feature patch; a missing one is an error unless
 * skip_missing_patches -- the extractors' GetVisibleObservations, reference_extractor.h:171-213).
 * Setup (BundleAdjustmentSetup, bundle_adjustment_options.h:28-42): in_setup / const_pose / tvec_mask (bit a = tvec[a]
 * constant) per image, variable_point / constant_point per point, constant_camera per camera; the four refine_* flags
 * and min_track_length of BundleOptimizerOptions (:66-90).
 * Outputs: the residual blocks (capacity n_p2d) as (image, point2D index, point3D), ordered by point and inside a point
 * like its track; per image whether it takes part, whether its pose is constant, its constant translation components;
 * per camera -1 (not in the problem) or the bit mask of constant parameters (all bits: the block is constant); per
 * point -1 (no residual block), 0 variable, 1 constant.  With inner iterations every variable point is in group 0
 * (:350-355).  The linear solver follows the number of images IN THE SETUP (:180-191), see pxr_lm_options. */
int pxr_ba_build_problem(int32_t n_images, const int32_t* image_camera, const int64_t* p2d_ptr, const int64_t* p2d_point3D,
                         int32_t n_cameras, const int32_t* cam_model, int64_t n_points, const int64_t* track_ptr,
                         const int32_t* track_image, const int32_t* track_p2d, const uint8_t* has_patch,
                         const uint8_t* in_setup, const uint8_t* const_pose, const uint8_t* tvec_mask,
                         const uint8_t* variable_point, const uint8_t* constant_point, const uint8_t* constant_camera,
                         int refine_focal_length, int refine_principal_point, int refine_extra_params, int refine_extrinsics,
                         int min_track_length, int skip_missing_patches, int64_t* n_obs, int32_t* obs_image, int32_t* obs_p2d,
                         int64_t* obs_point, uint8_t* image_in_problem, uint8_t* pose_is_const, uint8_t* tvec_mask_out,
                         int32_t* camera_mask, int8_t* point_role);

/* ---- global mapping: rotation averaging and global positioning --------------------
 * All rotations and centres at once from the verified pairs, instead of growing a model from an initial pair.  Conventions: a
 * pair p = (i, j) carries the pose of camera j relative to camera i, x_j = R_p x_i + t_p; with image poses x_i = R_i X + t_i and
 * centres c_i = -R_i^t t_i this is R_p = R_j R_i^t, and the baseline direction in the world b_p = -R_j^t t_p / |t_p| is parallel
 * to c_j - c_i.  All d_ arrays are device pointers, h_ arguments host pointers.
 *
 * pxr_rotation_averaging.  d_pair_image [n_pairs][2] int32, d_pair_qvec [n_pairs][4] (normalised on the way in), d_pair_weight
 * [n_pairs] >= 0 (for instance the pair's inlier count).  Outputs: d_qvec [n_images][4] (unit, w >= 0), *h_root, *h_iterations,
 * d_pair_angle [n_pairs] = the residual angle (radians) of every pair under the final rotations.
 *   1. Root: the image with the largest sum of weights over its pairs (summed in pair order), the first of equals.  R_root = I.
 *   2. Initial rotations by spanning tree (host): Prim from the root over the pairs of POSITIVE weight, always the heaviest pair
 *      that leaves the tree (ties: the lower pair index); R_j = R_p R_i or R_i = R_p^t R_j along it.  An image that is not
 *      reached makes the call fail with PXR_EINVAL.
 *   3. Iteration it = 0, 1, ...:  e_p = Log(R_j^t R_p R_i), theta_p = |e_p|;  rho_p = w_p / max(theta_p, min_angle) while
 *      it < l1_iterations (L1 by reweighting), after that rho_p = w_p / (1 + (theta_p / sigma)^2);  solve L w = b, L the graph
 *      Laplacian of the rho_p with the root's row and column removed, b_j += rho_p e_p, b_i -= rho_p e_p (the three coordinates
 *      decouple: one (n - 1)^2 matrix, three right-hand sides);  R_k <- R_k Exp(w_k).  Stop once it >= l1_iterations and
 *      max_k |w_k| < tolerance, or after max_iterations.
 * Device: a lane per pair for Log and the weights; L and b assembled owner-computes per image row from an image -> pairs list
 * (no atomics, the same bits every run); the solve is the library's dense fp64 Cholesky, three factor + solve calls per iteration.
 * PXR_EINVAL, outputs untouched: n_images < 1, n_images - 1 > PXR_MAX_IMAGES_DIRECT, a pair index out of range, a pair with
 * i == j, a weight negative or not finite, a qvec zero or not finite, an option out of range, images not connected to the root.
 * PXR_ENUMERIC: a Laplacian that is not positive definite in floating point.  Synchronises the context's stream every iteration. */
typedef struct {
  int32_t l1_iterations;    /* 20 */
  int32_t max_iterations;   /* 40 */
  double min_angle;         /* 1e-3 radians: the floor of theta in the L1 weights */
  double sigma;             /* 5.0 degrees: the Cauchy scale after the L1 phase */
  double tolerance;         /* 1e-10 radians */
} pxr_rotavg_options;
void pxr_rotavg_default_options(pxr_rotavg_options* options);
int pxr_rotation_averaging(pxr_ctx* ctx, int32_t n_images, int32_t n_pairs, const int32_t* d_pair_image, const double* d_pair_qvec,
                           const double* d_pair_weight, const pxr_rotavg_options* options, double* d_qvec, int32_t* h_root,
                           int32_t* h_iterations, double* d_pair_angle);
/* The same, and HIP-event times summed over the iterations: h_kernel_ms[3] = residuals, first assembly, solves (with the two other
 * assemblies and the update). */
int pxr_rotation_averaging_timed(pxr_ctx* ctx, int32_t n_images, int32_t n_pairs, const int32_t* d_pair_image, const double* d_pair_qvec,
                                 const double* d_pair_weight, const pxr_rotavg_options* options, double* d_qvec, int32_t* h_root,
                                 int32_t* h_iterations, double* d_pair_angle, double* h_kernel_ms);

/* pxr_global_positioning.  view: tracks, observations and cameras as for pxr_triangulate_tracks (offsets start at 0); its d_qvec
 * holds the averaged rotations, d_tvec is ignored.  Pairs: d_pair_image [n_pairs][2], d_pair_dir [n_pairs][3] = the unit b_p above,
 * d_pair_weight [n_pairs] >= 0; root: the image whose centre is the origin.  Outputs: d_centre [n_images][3], d_xyz [n_tracks][3]
 * (written where the status is 0), d_track_status (0 = point written, 1 = fewer than two usable rays or near-singular A_k in the last
 * round), d_obs_weight [n_obs] and d_pair_weight_out [n_pairs] (the final robust weights, 0 = rejected), *h_status (0 = ok,
 * 1 = degenerate: the outputs are then unspecified and the return value is still 0), *h_rounds (rounds completed).
 *   Every observation becomes a world-frame unit ray d = R_i^t (u, v, 1) / |.| with (u, v) its undistorted point; one that cannot
 *   be undistorted has weight 0 throughout.  P = I - d d^t.  Pairs: P_p = I - b_p b_p^t, w_p = d_pair_weight[p] / max weight times
 *   a robust factor that starts at 1.  Observation weights start at 1.  Each of `iterations` rounds:
 *   1. per track A_k = sum w P; the track is valid iff det A_k > min_det; A_k^-1 in closed form (adjugate);
 *   2. the reduced system over the centres, dense 3n x 3n, upper triangle: S_ii += w P for the observations of valid tracks,
 *      S_ij -= (w_a P_a) A_k^-1 (w_b P_b) for every ordered pair (a, b) of observations of a valid track (images i, j, a = b
 *      included), and w_p P_p added to (i, i) and (j, j), subtracted from (i, j) and (j, i);
 *   3. gauge: c_root = 0 (its rows and columns removed); scale and sign by g^t c = h with g_j += w_p b_p, g_i -= w_p b_p,
 *      h = sum w_p (the weighted mean baseline length along the pairs' own directions is 1).  The cost is homogeneous, so the
 *      constrained minimum is y = S^-1 g, c = h y / (g^t y): one Cholesky solve.  A non-positive pivot or g^t y <= 0: degenerate;
 *   4. X_k = A_k^-1 sum w P c_i;
 *   5. with v = X_k - c_i, s = |P v| / |v|: w = 1 / (1 + (s / sigma_obs)^2), 0 for an invalid track or v = 0, and from round
 *      cheirality_from on (counting from 0) 0 where d^t v <= 0; the pairs' robust factors likewise with v = c_j - c_i, sigma_pair.
 * Device: a track per 16 lanes; everything between two rounds stays on the device, the host reads one word per round.  S is summed
 * in 64-bit fixed point with integer atomics (every addend is at most 1 in magnitude, the scale comes from the largest number of
 * addends an entry can receive): the same bits every run.
 * PXR_EINVAL, outputs untouched: offsets not starting at 0, not monotone or not ending at n_obs; an image, camera, pair or root
 * index out of range; a pair with i == j; a direction that is not a finite unit vector (to 1e-9); a weight negative or not finite;
 * n_images - 1 > PXR_MAX_IMAGES_DIRECT (the Cholesky's 3 (n - 1) columns); an option out of range. */
typedef struct {
  int32_t iterations;       /* 8 */
  int32_t cheirality_from;  /* 2: the first round (from 0) whose reweighting rejects what lies behind its camera */
  double sigma_obs;         /* 1.0 degree */
  double sigma_pair;        /* 3.0 degrees */
  double min_det;           /* 1e-12 */
} pxr_globalpos_options;
void pxr_globalpos_default_options(pxr_globalpos_options* options);
int pxr_global_positioning(pxr_ctx* ctx, const pxr_tri_view* view, int32_t n_pairs, const int32_t* d_pair_image, const double* d_pair_dir,
                           const double* d_pair_weight, int32_t root, const pxr_globalpos_options* options, double* d_centre,
                           double* d_xyz, int32_t* d_track_status, double* d_obs_weight, double* d_pair_weight_out, int32_t* h_status,
                           int32_t* h_rounds);
/* The same, and HIP-event times summed over the rounds: h_kernel_ms[5] = tracks (A_k), contraction (with the pair terms), gauge and
 * packing, Cholesky, scale and reweighting. */
int pxr_global_positioning_timed(pxr_ctx* ctx, const pxr_tri_view* view, int32_t n_pairs, const int32_t* d_pair_image,
                                 const double* d_pair_dir, const double* d_pair_weight, int32_t root,
                                 const pxr_globalpos_options* options, double* d_centre, double* d_xyz, int32_t* d_track_status,
                                 double* d_obs_weight, double* d_pair_weight_out, int32_t* h_status, int32_t* h_rounds, double* h_kernel_ms);

/* Residual-block selection of TopologicalKeypointOptimizer::SetUp + AddIntraResiduals (A12,
 * topological_keypoint_optimizer.h:97-175, featuremetric_keypoint_optimizer.h:158-202): intra-track matches,
 * minus keypoint aliases, optionally root edges only, plus root-regularisation blocks; weights = similarity
 * (weight_by_sim) or 1 / root_regularize_weight.  HOST arrays; node_feature [n_nodes] = FeatureNode::feature_idx;
 * edges grouped by ascending source node (Graph order); nodes_in_problem NULL = every node;
 * out_src / out_dst / out_w have capacity 3 * n_edges, *n_out receives the number of blocks.  The output is what
 * pxr_ka_view's d_edge_src / d_edge_dst / d_edge_w take. */
int pxr_ka_build_edges(int64_t n_nodes, const int32_t* node_image, const int32_t* node_feature,
                       int64_t n_edges, const int64_t* edge_src, const int64_t* edge_dst, const double* edge_sim,
                       const int64_t* track_labels, const uint8_t* root_labels, const int64_t* nodes_in_problem,
                       int64_t n_in_problem, int weight_by_sim, int root_edges_only,
                       double root_regularize_weight, int64_t* out_src, int64_t* out_dst, double* out_w,
                       int64_t* n_out);

/* Dense SPD solve used for the reduced camera system (what Ceres' DENSE_SCHUR / SPARSE_SCHUR
 * Cholesky does on the CPU, bundle_optimizer.h:181-191): blocked right-looking Cholesky +
 * substitution in hand-written HIP.  d_a: n x n row-major, UPPER triangle filled (overwritten
 * by the factor); d_b: right-hand side -> solution.  *h_info = 0 or the 1-based index of the
 * first non-positive pivot. */
int pxr_dense_spd_solve(pxr_ctx* ctx, double* d_a, int n, double* d_b, int* h_info);

/* Dense SPD inverse (the covariance of a reduced camera system, what ceres::Covariance's dense path
 * computes): the Cholesky factorisation of pxr_dense_spd_solve, then T = inv(L) by block columns and
 * inv(A) = T^T T in 64 x 64 fp64 MFMA tiles; no atomics, the same bits every run.
 * d_a: n x n row-major, UPPER triangle filled (the strictly lower part is ignored).  On return the FULL
 * symmetric inverse (symmetric bit for bit).
 * *h_info: 0, or the 1-based index of the first non-positive pivot.  In that case d_a is unspecified and
 * the return value is 0.  n may not exceed 18 * PXR_MAX_IMAGES_DIRECT (PXR_EINVAL). */
int pxr_dense_spd_inverse(pxr_ctx* ctx, double* d_a, int n, int* h_info);

#ifdef __cplusplus
}
#endif
#endif /* PIXSFM_HIP_H_ */
