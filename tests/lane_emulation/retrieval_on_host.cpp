// csrc/pxr_retrieval.hip as host code over the stand-in runtime (on_host.h, hip/hip_runtime.h).
// With -DRETRIEVAL_ON_HOST_MAIN: a stand-alone program (for -fsanitize=address,undefined builds) that trains a vocabulary, aggregates
// and selects on synthetic descriptors (command line: n_images rows_per_image dim n_clusters num_matched) with every array allocated
// at its exact size -- images of different sizes, one of them empty, one row that is not valid -- and prints the counts.
#include "on_host.h"
#include "pxr_retrieval.hip"

#ifdef RETRIEVAL_ON_HOST_MAIN
#include <limits>
int main(int argc, char** argv) {
  if (argc < 6) return 2;
  const int n_images = atoi(argv[1]), per = atoi(argv[2]), dim = atoi(argv[3]), K = atoi(argv[4]), num_matched = atoi(argv[5]);
  std::vector<int64_t> off((size_t)n_images + 1, 0);
  for (int m = 0; m < n_images; ++m) off[(size_t)m + 1] = off[(size_t)m] + (m == 1 ? 0 : per + 7 * m);   // image 1 is empty
  const int64_t n_total = off[(size_t)n_images];
  std::vector<float> desc((size_t)n_total * dim);
  uint32_t state = 12345u;
  for (int64_t i = 0; i < n_total; ++i) {
    double n2 = 0.0;
    for (int k = 0; k < dim; ++k) {
      state = state * 1664525u + 1013904223u;
      const float v = (float)((state >> 8) & 0xffff) / 65536.0f - 0.5f;
      desc[(size_t)i * dim + k] = v;
      n2 += (double)v * v;
    }
    for (int k = 0; k < dim; ++k) desc[(size_t)i * dim + k] = (float)(desc[(size_t)i * dim + k] / std::sqrt(n2 > 0 ? n2 : 1.0));
  }
  if (n_total > 3) desc[(size_t)3 * dim] = std::numeric_limits<float>::quiet_NaN();
  pxr_ctx* ctx = emu_ctx();
  std::vector<float> C((size_t)K * dim), G((size_t)n_images * K * dim);
  std::vector<int32_t> cnt((size_t)K), assign((size_t)n_total), counts((size_t)n_images * K);
  int32_t n_empty = -1;
  int rc = pxr_vocab_train(ctx, n_total, dim, desc.data(), K, 2, n_total - 5, C.data(), cnt.data(), &n_empty);
  if (rc) { printf("error %d: %s\n", rc, g_err); return 1; }
  rc = pxr_vlad_aggregate(ctx, n_images, off.data(), n_total, dim, desc.data(), K, C.data(), G.data(), assign.data(), counts.data());
  if (rc) { printf("error %d: %s\n", rc, g_err); return 1; }
  std::vector<int32_t> self((size_t)n_images), top((size_t)n_images * num_matched), found((size_t)n_images);
  std::vector<float> top_sim((size_t)n_images * num_matched);
  for (int m = 0; m < n_images; ++m) self[(size_t)m] = m;
  rc = pxr_retrieval_topk(ctx, n_images, n_images, K * dim, G.data(), G.data(), self.data(), nullptr, num_matched,
                          std::numeric_limits<double>::infinity(), top.data(), top_sim.data(), found.data());
  if (rc) { printf("error %d: %s\n", rc, g_err); return 1; }
  int64_t n_assigned = 0, n_counted = 0, n_found = 0;
  for (int32_t a : assign) n_assigned += a >= 0;
  for (int32_t c : counts) n_counted += c;
  for (int32_t f : found) n_found += f;
  printf("rows %lld assigned %lld counted %lld empty %d found %lld\n", (long long)n_total, (long long)n_assigned, (long long)n_counted,
         (int)n_empty, (long long)n_found);
  emu_ctx_free(ctx);
  return 0;
}
#endif
