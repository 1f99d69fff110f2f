// csrc/pxr_match.hip as host code over the stand-in runtime (on_host.h, hip/hip_runtime.h), for pxr_match_guided
// (tests/test_guided_matching_lanes_cpu.py): the translation unit of match_on_host.cpp, which exports every entry point of the file.
// With -DGUIDED_ON_HOST_MAIN: a stand-alone program (for -fsanitize=address,undefined builds) that runs pxr_match_guided on one
// pair of (1, 1, 1), one of (129, 65, 128) and a batch over images of 0, 1, 33, 129 and 200 descriptors with the empty image on
// either side, both kinds under "NN-ratio" (ratio test and mutual check), every array allocated at its exact size, and prints the
// match counts.
#include "match_on_host.cpp"

#ifdef GUIDED_ON_HOST_MAIN
#include <random>
namespace {
struct Batch {
  std::vector<int64_t> off{0};
  std::vector<float> desc;
  std::vector<double> xy;
  int dim;
};

Batch make_batch(const std::vector<int>& sizes, int dim, std::mt19937_64& rng) {
  Batch b;
  b.dim = dim;
  std::normal_distribution<float> g(0.f, 1.f);
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  for (int n : sizes) {
    b.off.push_back(b.off.back() + n);
    for (int i = 0; i < n; ++i) {
      std::vector<float> v(dim);
      float s = 0.f;
      for (float& x : v) { x = g(rng); s += x * x; }
      for (float x : v) b.desc.push_back(x / std::sqrt(s));
      b.xy.push_back(u(rng)); b.xy.push_back(u(rng));
    }
  }
  return b;
}

int run(pxr_ctx* ctx, const Batch& b, const std::vector<int32_t>& pairs, const char* what) {
  const int32_t n_pairs = (int32_t)pairs.size() / 2;
  std::vector<int64_t> pair_off(1, 0);
  for (int32_t p = 0; p < n_pairs; ++p) pair_off.push_back(pair_off.back() + b.off[pairs[2 * p] + 1] - b.off[pairs[2 * p]]);
  std::vector<int32_t> kind((size_t)n_pairs), m0((size_t)pair_off.back()), n_m((size_t)n_pairs);
  std::vector<double> model((size_t)n_pairs * 9), thr((size_t)n_pairs);
  std::vector<float> s0((size_t)pair_off.back());
  const double E[9] = {0.0, -0.1, 0.2, 0.1, 0.0, -1.0, -0.2, 1.0, 0.0}, H[9] = {1.0, 0.05, 0.0, -0.05, 1.0, 0.1, 0.1, 0.0, 1.0};
  for (int32_t p = 0; p < n_pairs; ++p) {
    kind[p] = p & 1;
    thr[p] = kind[p] ? 0.6 : 0.15;
    for (int k = 0; k < 9; ++k) model[9 * (size_t)p + k] = kind[p] ? H[k] : E[k];
  }
  const pxr_match_options o = {0.8, 0.0, 1, 0};
  const int rc = pxr_match_guided(ctx, (int32_t)b.off.size() - 1, b.off.data(), b.off.back(), b.dim, b.desc.data(), b.xy.data(), n_pairs,
                                  pairs.data(), pair_off.data(), kind.data(), model.data(), thr.data(), &o, m0.data(), s0.data(), n_m.data());
  if (rc) { printf("%s: error %d: %s\n", what, rc, g_err); return 1; }
  printf("%s:", what);
  for (int32_t p = 0; p < n_pairs; ++p) printf(" %d", n_m[p]);
  printf("\n");
  return 0;
}
}  // namespace

int main() {
  std::mt19937_64 rng(5);
  pxr_ctx* ctx = emu_ctx();
  int bad = 0;
  bad |= run(ctx, make_batch({1, 1}, 1, rng), {0, 1, 1, 0}, "1x1x1");
  bad |= run(ctx, make_batch({129, 65}, 128, rng), {0, 1, 0, 1}, "129x65x128");
  bad |= run(ctx, make_batch({0, 1, 33, 129, 200}, 128, rng), {4, 4, 3, 4, 3, 4, 4, 3, 0, 2, 2, 0, 1, 3}, "batch");
  emu_ctx_free(ctx);
  return bad;
}
#endif
