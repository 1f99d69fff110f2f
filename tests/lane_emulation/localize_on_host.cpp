// csrc/pxr_localize.hip as host code over the stand-in runtime (on_host.h, hip/hip_runtime.h).
// With -DLOCALIZE_ON_HOST_MAIN: a stand-alone program (for -fsanitize=address,undefined builds) that runs the three entry points
// once with every array allocated at its exact size -- a map of argv[1] images whose tracks have the lengths argv[2..] (the second
// one masked out), both numbers of partners, retrieval lists of 0, 1, 63 and 64 entries, and a batch of 2D-3D problems (a query
// without keypoints, a database image without keypoints, an empty problem, one of 64 entries, points without coordinates) -- and
// prints what it counted.
#include "on_host.h"
#include "pxr_localize.hip"

#ifdef LOCALIZE_ON_HOST_MAIN
#include <limits>
#include <random>
int main(int argc, char** argv) {
  const int32_t n_images = argc > 1 ? atoi(argv[1]) : 65;
  std::vector<int64_t> track_off(1, 0);
  for (int i = 2; i < argc; ++i) track_off.push_back(track_off.back() + atoll(argv[i]));
  const int64_t n_tracks = (int64_t)track_off.size() - 1, n_obs = track_off.back();
  std::mt19937_64 rng(7);
  std::vector<int32_t> obs_image(n_obs);
  for (auto& i : obs_image) i = (int32_t)(rng() % (uint64_t)n_images);
  std::vector<uint8_t> mask(n_tracks, 1);
  if (n_tracks > 1) mask[1] = 0;
  pxr_ctx* ctx = emu_ctx();
  std::vector<int32_t> count((size_t)n_images * n_images);
  for (int32_t K : {1, 100}) {
    std::vector<int32_t> topk_index((size_t)n_images * K), topk_count((size_t)n_images * K), n_topk(n_images);
    const int rc = pxr_covisibility(ctx, n_images, n_tracks, track_off.data(), n_obs, obs_image.data(), mask.data(), K, count.data(),
                                    topk_index.data(), topk_count.data(), n_topk.data());
    if (rc) { printf("error %d: %s\n", rc, g_err); return 1; }
    long long sum = 0, asym = 0, diag = 0, partners = 0, best = 0;
    for (int32_t i = 0; i < n_images; ++i) {
      diag += count[(size_t)i * n_images + i]; partners += n_topk[i];
      if (n_topk[i] > 0) best += topk_count[(size_t)i * K];
      for (int32_t j = 0; j < n_images; ++j) { sum += count[(size_t)i * n_images + j]; asym += count[(size_t)i * n_images + j] != count[(size_t)j * n_images + i]; }
    }
    printf("covisibility K %d sum %lld asymmetric %lld diagonal %lld partners %lld best %lld\n", (int)K, sum, asym, diag, partners, best);
  }
  if (int rc = pxr_covisibility(ctx, n_images, n_tracks, track_off.data(), n_obs, obs_image.data(), nullptr, 0, count.data(), nullptr, nullptr, nullptr)) {
    printf("error %d: %s\n", rc, g_err); return 1;
  }

  {
    const std::vector<int64_t> ret_off = {0, 0, 1, 64, 128};
    std::vector<int32_t> ret(128), cluster(128), n_clusters(4);
    for (auto& i : ret) i = (int32_t)(rng() % (uint64_t)n_images);
    const int rc = pxr_covisibility_clusters(ctx, n_images, count.data(), 4, ret_off.data(), 128, ret.data(), cluster.data(), n_clusters.data());
    if (rc) { printf("error %d: %s\n", rc, g_err); return 1; }
    printf("clusters %d %d %d %d\n", n_clusters[0], n_clusters[1], n_clusters[2], n_clusters[3]);
    for (int q = 0; q < 4; ++q)
      for (int64_t r = ret_off[q]; r < ret_off[q + 1]; ++r)
        if (cluster[r] < 0 || cluster[r] >= n_clusters[q]) { printf("cluster number out of range\n"); return 1; }
  }

  {
    const std::vector<int64_t> img_off = {0, 70, 70, 110, 110, 135};                 // queries 0, 1; database images 2, 3, 4
    const std::vector<int32_t> pairs = {0, 2, 0, 3, 0, 4, 1, 2, 1, 3, 1, 4};
    const std::vector<int64_t> pair_off = {0, 70, 140, 210, 210, 210, 210};
    const int64_t n_points = 30, n_total = img_off.back(), n_rows = pair_off.back();
    std::vector<int32_t> matches0(n_rows);
    for (int p = 0; p < 3; ++p) {
      const int64_t nb = img_off[pairs[2 * p + 1] + 1] - img_off[pairs[2 * p + 1]];
      for (int64_t k = 0; k < 70; ++k) matches0[pair_off[p] + k] = nb == 0 || rng() % 3 == 0 ? -1 : (int32_t)(rng() % (uint64_t)nb);
    }
    std::vector<double> kp_xy(2 * n_total), xyz(3 * n_points);
    for (auto& v : kp_xy) v = (double)(rng() % 640);
    for (auto& v : xyz) v = (double)(rng() % 100) / 10.0;
    kp_xy[2 * 8] = std::numeric_limits<double>::quiet_NaN();
    xyz[3 * 11 + 1] = std::numeric_limits<double>::quiet_NaN();
    xyz[3 * 12 + 2] = std::numeric_limits<double>::infinity();
    std::vector<int64_t> kp_point(n_total);
    for (auto& v : kp_point) v = (int64_t)(rng() % (uint64_t)(n_points + 8)) - 8;
    std::vector<int64_t> prob_off = {0, 3, 3, 6};
    std::vector<int32_t> prob_pair = {2, 0, 1, 3, 4, 5};
    for (int e = 0; e < 64; ++e) prob_pair.push_back((int32_t)(rng() % 3));
    prob_off.push_back((int64_t)prob_pair.size());
    int64_t cap = 0;
    for (int32_t pr : prob_pair) cap += pair_off[pr + 1] - pair_off[pr];
    std::vector<int64_t> corr_off(prob_off.size()), corr_point(cap);
    std::vector<int32_t> corr_kp(cap);
    std::vector<double> corr_xy(2 * cap), corr_xyz(3 * cap);
    int64_t n_corr = -1;
    const int rc = pxr_localization_pairs(ctx, (int32_t)prob_off.size() - 1, prob_off.data(), (int64_t)prob_pair.size(), prob_pair.data(), 6, pairs.data(),
                                          pair_off.data(), n_rows, matches0.data(), 5, img_off.data(), n_total, kp_xy.data(), kp_point.data(), n_points,
                                          xyz.data(), corr_off.data(), corr_kp.data(), corr_point.data(), corr_xy.data(), corr_xyz.data(), &n_corr);
    if (rc) { printf("error %d: %s\n", rc, g_err); return 1; }
    printf("pairs capacity %lld total %lld offsets", (long long)cap, (long long)n_corr);
    for (int64_t o : corr_off) printf(" %lld", (long long)o);
    printf("\n");
  }
  emu_ctx_free(ctx);
  return 0;
}
#endif
