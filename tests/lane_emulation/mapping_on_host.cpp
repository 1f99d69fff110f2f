// csrc/pxr_mapper.hip as host code over the stand-in runtime (on_host.h, hip/hip_runtime.h).
// With -DMAPPING_ON_HOST_MAIN: a stand-alone program (for -fsanitize=address,undefined builds) that runs one scene whose images
// have the observation counts given on the command line -- every third observation on a track without a point, every seventh
// with a keypoint that is not finite, the second image masked out -- with every array allocated at its exact size, and prints
// per image the visible count, the score and the offset.
#include "on_host.h"
#include "pxr_mapper.hip"

#ifdef MAPPING_ON_HOST_MAIN
#include <limits>
#include <random>
int main(int argc, char** argv) {
  std::vector<int64_t> image_off(1, 0);
  for (int i = 1; i < argc; ++i) image_off.push_back(image_off.back() + atoll(argv[i]));
  const int32_t n_images = (int32_t)image_off.size() - 1;
  const int64_t n_obs = image_off.back(), n_tracks = std::max<int64_t>(n_obs / 2, 1);
  std::mt19937_64 rng(5);
  std::uniform_real_distribution<double> px(-100.0, 900.0);
  // observation k of image i is observation number (k * n_images + i) mod-ordered into tracks: built image-major, then sorted by track
  std::vector<int64_t> track_of(n_obs), image_of(n_obs);
  for (int32_t i = 0; i < n_images; ++i)
    for (int64_t k = image_off[i]; k < image_off[i + 1]; ++k) { track_of[k] = (int64_t)(rng() % (uint64_t)n_tracks); image_of[k] = i; }
  std::vector<int64_t> perm(n_obs);
  for (int64_t o = 0; o < n_obs; ++o) perm[o] = o;
  std::stable_sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) { return track_of[a] < track_of[b]; });
  std::vector<int64_t> track_off(n_tracks + 1, 0), obs_track(n_obs), image_obs(n_obs);
  std::vector<int32_t> obs_image(n_obs);
  std::vector<double> obs_xy(2 * n_obs);
  for (int64_t o = 0; o < n_obs; ++o) {
    obs_track[o] = track_of[perm[o]]; obs_image[o] = (int32_t)image_of[perm[o]]; ++track_off[obs_track[o] + 1];
    obs_xy[2 * o] = o % 7 == 3 ? std::numeric_limits<double>::quiet_NaN() : px(rng); obs_xy[2 * o + 1] = px(rng);
  }
  for (int64_t t = 0; t < n_tracks; ++t) track_off[t + 1] += track_off[t];
  std::vector<int64_t> fill(image_off.begin(), image_off.end() - 1);
  for (int64_t o = 0; o < n_obs; ++o) image_obs[fill[obs_image[o]]++] = o;               // ascending inside an image
  std::vector<double> xyz(3 * n_tracks, 1.0);
  std::vector<int32_t> status(n_tracks), image_camera(n_images), cam_size = {800, 600, 640, 480};
  for (int64_t t = 0; t < n_tracks; ++t) status[t] = t % 3 == 1 ? 2 : 0;
  std::vector<uint8_t> mask(n_images, 1);
  for (int32_t i = 0; i < n_images; ++i) image_camera[i] = i % 2;
  if (n_images > 1) mask[1] = 0;
  pxr_tri_view v = {};
  v.n_tracks = n_tracks; v.d_track_offsets = track_off.data(); v.n_obs = n_obs; v.d_obs_image = obs_image.data();
  v.d_obs_xy = obs_xy.data(); v.n_images = n_images; v.d_image_camera = image_camera.data(); v.n_cameras = 2;
  std::vector<int32_t> n_visible(n_images);
  std::vector<int64_t> score(n_images), corr_off(n_images + 1), corr_obs(n_obs);
  std::vector<double> corr_xy(2 * n_obs), corr_xyz(3 * n_obs);
  int64_t n_corr = -1;
  pxr_ctx* ctx = emu_ctx();
  for (int levels : {1, 6}) {
    const int rc = pxr_mapper_visibility(ctx, &v, obs_track.data(), image_off.data(), image_obs.data(), xyz.data(), status.data(),
                                         mask.data(), cam_size.data(), levels, n_visible.data(), score.data(), corr_off.data(),
                                         corr_obs.data(), corr_xy.data(), corr_xyz.data(), &n_corr);
    if (rc) { printf("error %d: %s\n", rc, g_err); return 1; }
    for (int32_t i = 0; i < n_images; ++i)
      printf("L %d image %d observations %lld visible %d score %lld offset %lld\n", levels, i, (long long)(image_off[i + 1] - image_off[i]),
             n_visible[i], (long long)score[i], (long long)corr_off[i]);
    printf("L %d total %lld\n", levels, (long long)n_corr);
  }
  emu_ctx_free(ctx);
  return 0;
}
#endif
