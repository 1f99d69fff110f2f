// csrc/pxr_sift.hip as host code over the stand-in runtime (on_host.h, hip/hip_runtime.h).
// With -DSIFT_ON_HOST_MAIN: a stand-alone program (for -fsanitize=address,undefined builds) that runs pyramid, detect and describe
// on a synthetic h x w image (command line: h w first_octave capacity) with every array allocated at its exact size -- the
// pyramid at pxr_sift_pyramid_bytes, the outputs at `capacity` rows, below the number found when capacity is small -- and prints
// the counts.  The keypoints given to describe include one that is not finite, one with a negative sigma, one far outside the
// image and one whose window is larger than its octave.
#include "on_host.h"
#include "pxr_sift.hip"

#ifdef SIFT_ON_HOST_MAIN
#include <limits>
int main(int argc, char** argv) {
  if (argc < 5) return 2;
  const int h = atoi(argv[1]), w = atoi(argv[2]), first = atoi(argv[3]);
  const int64_t capacity = atoll(argv[4]);
  std::vector<uint8_t> image((size_t)h * w);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {                     // blobs on a 12-pixel grid, alternating sign, over a ramp
      const double dx = (x % 12) - 5.3, dy = (y % 12) - 5.6, sign = ((x / 12 + y / 12) & 1) ? -1.0 : 1.0;
      image[(size_t)y * w + x] = (uint8_t)std::lrint(128.0 + 0.2 * x + 100.0 * sign * std::exp(-(dx * dx + dy * dy) / (2.0 * 2.2 * 2.2)));
    }
  pxr_sift_options opt;
  pxr_sift_default_options(&opt);
  opt.first_octave = first;
  int64_t bytes = -1;
  pxr_ctx* ctx = emu_ctx();
  int rc = pxr_sift_pyramid_bytes(h, w, &opt, &bytes);
  if (rc) { printf("error %d: %s\n", rc, g_err); return 1; }
  std::vector<float> pyramid((size_t)bytes / 4);
  rc = pxr_sift_pyramid(ctx, image.data(), PXR_U8, h, w, &opt, pyramid.data());
  if (rc) { printf("error %d: %s\n", rc, g_err); return 1; }
  std::vector<double> kp((size_t)capacity * 4);
  std::vector<int32_t> rec((size_t)capacity * 4);
  std::vector<float> resp((size_t)capacity);
  int64_t found = -1;
  rc = pxr_sift_detect(ctx, pyramid.data(), h, w, &opt, capacity, kp.data(), rec.data(), resp.data(), &found);
  if (rc) { printf("error %d: %s\n", rc, g_err); return 1; }
  const int64_t n = std::min(found, capacity);
  std::vector<double> q(kp.begin(), kp.begin() + 4 * n);
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  int32_t n_oct = 0, sizes[16];
  int64_t offsets[8];
  rc = pxr_sift_pyramid_layout(h, w, &opt, &n_oct, sizes, offsets);
  if (rc) { printf("error %d: %s\n", rc, g_err); return 1; }
  const double coarse = opt.sigma0 * std::exp2(first + n_oct - 1 + 0.8);     // in the last octave, its window larger than that octave
  const double extra[5][4] = {{nan, 3.0, 2.0, 0.0}, {5.0, 5.0, -1.0, 0.0}, {1e300, -1e300, 2.0, 1.0}, {w / 2.0, h / 2.0, coarse, 0.5},
                              {3.0, inf, 2.0, 0.0}};
  for (auto& e : extra) q.insert(q.end(), e, e + 4);
  const int64_t nq = n + 5;
  std::vector<float> desc((size_t)nq * 128);
  std::vector<uint8_t> valid((size_t)nq);
  rc = pxr_sift_describe(ctx, pyramid.data(), h, w, &opt, nq, q.data(), desc.data(), valid.data());
  if (rc) { printf("error %d: %s\n", rc, g_err); return 1; }
  int64_t n_valid = 0;
  for (int64_t i = 0; i < n; ++i) n_valid += valid[i];
  printf("found %lld written %lld valid %lld extra %d %d %d %d %d\n", (long long)found, (long long)n, (long long)n_valid, valid[n], valid[n + 1],
         valid[n + 2], valid[n + 3], valid[n + 4]);
  emu_ctx_free(ctx);
  return 0;
}
#endif
