// csrc/pxr_cloud.hip as host code over the stand-in runtime (on_host.h, hip/hip_runtime.h).
// With -DCLOUD_ON_HOST_MAIN: a stand-alone program (for -fsanitize=address,undefined builds) that runs both entry points on
// synthetic clouds (command line: n_ref n_query max_dist voxel_size) with every array allocated at its exact size -- rows that are
// not valid in both clouds, points on cell faces, duplicates -- checks the result against the brute-force search and prints counts.
#include "on_host.h"
#include "pxr_cloud.hip"

#ifdef CLOUD_ON_HOST_MAIN
int main(int argc, char** argv) {
  if (argc < 5) return 2;
  const int64_t n_ref = atoll(argv[1]), n_query = atoll(argv[2]);
  const double max_dist = atof(argv[3]), voxel = atof(argv[4]);
  uint32_t state = 2024u;
  auto fill = [&](std::vector<double>& c, int64_t n) {
    c.resize((size_t)n * 3);
    for (int64_t i = 0; i < n * 3; ++i) {
      state = state * 1664525u + 1013904223u;
      const int k = (int)((state >> 8) % 41) - 20;                       // multiples of max_dist / 2: cell faces, duplicates, exact ties
      c[(size_t)i] = 0.5 * max_dist * k;
    }
    if (n > 2) c[3 * 2 + 1] = std::numeric_limits<double>::quiet_NaN();
    if (n > 5) c[3 * 5] = -std::numeric_limits<double>::infinity();
  };
  std::vector<double> ref, query;
  fill(ref, n_ref);
  fill(query, n_query);
  pxr_ctx* ctx = emu_ctx();
  std::vector<int32_t> idx((size_t)n_query);
  std::vector<double> d2((size_t)n_query);
  int rc = pxr_cloud_nearest(ctx, n_ref, ref.data(), n_query, query.data(), max_dist, idx.data(), d2.data());
  if (rc) { printf("error %d: %s\n", rc, g_err); return 1; }
  int64_t found = 0, wrong = 0;
  const double m2 = max_dist * max_dist;
  for (int64_t i = 0; i < n_query; ++i) {
    int32_t best = -1;
    double bd = std::numeric_limits<double>::infinity();
    const double* q = &query[(size_t)i * 3];
    if (std::isfinite(q[0]) && std::isfinite(q[1]) && std::isfinite(q[2]))
      for (int64_t r = 0; r < n_ref; ++r) {
        const double* p = &ref[(size_t)r * 3];
        if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]))) continue;
        const double dx = q[0] - p[0], dy = q[1] - p[1], dz = q[2] - p[2];
        const double d = (dx * dx + dy * dy) + dz * dz;
        if (d <= m2 && (best < 0 || d < bd)) { bd = d; best = (int32_t)r; }
      }
    found += idx[(size_t)i] >= 0;
    wrong += idx[(size_t)i] != best || d2[(size_t)i] != bd;
  }
  const double tol[3] = {0.5 * max_dist, max_dist, 2.0 * max_dist};
  double frac[3] = {-7.0, -7.0, -7.0};
  int64_t n_vox = -7;
  rc = pxr_cloud_voxel_fractions(ctx, n_query, query.data(), d2.data(), voxel, 3, tol, frac, &n_vox);
  if (rc) { printf("error %d: %s\n", rc, g_err); return 1; }
  printf("queries %lld found %lld wrong %lld voxels %lld fraction %.17g\n", (long long)n_query, (long long)found, (long long)wrong,
         (long long)n_vox, frac[2]);
  emu_ctx_free(ctx);
  return 0;
}
#endif
