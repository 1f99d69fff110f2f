// csrc/pxr_homography.hip as host code over the stand-in runtime (on_host.h, hip/hip_runtime.h).
// With -DHOMOGRAPHY_ON_HOST_MAIN: a stand-alone program (for -fsanitize=address,undefined builds) that runs synthetic pairs of
// the match counts given on the command line -- 0 is an empty pair -- alternately rotation-only and in front of a plane, and
// prints every pair's status, inliers, rotation inliers and trials.
#include "on_host.h"
#include "pxr_homography.hip"

#ifdef HOMOGRAPHY_ON_HOST_MAIN
#include <random>
int main(int argc, char** argv) {
  std::vector<int64_t> off(1, 0);
  for (int i = 1; i < argc; ++i) off.push_back(off.back() + atoll(argv[i]));
  const int32_t T = (int32_t)off.size() - 1;
  const int64_t N = off.back();
  std::mt19937_64 rng(7);
  std::uniform_real_distribution<double> uni(0.0, 1.0);
  // pinhole cameras (f 1200, c 500 / 480); camera 2 = a rotation of 0.1 rad about y, and for odd pairs a baseline along x in
  // front of the plane Z = 6; every fourth match an outlier
  const double f = 1200.0, cx = 500.0, cy = 480.0, cs = cos(0.1), sn = sin(0.1);
  std::vector<double> xy1((size_t)N * 2 + 2), xy2((size_t)N * 2 + 2);
  for (int32_t p = 0; p < T; ++p)
    for (int64_t i = off[p]; i < off[p + 1]; ++i) {
      const double u = uni(rng) * 0.7 - 0.35, v = uni(rng) * 0.7 - 0.35, d = (p & 1) ? 6.0 : 2.0 + 18.0 * uni(rng);
      const double X = u * d, Y = v * d, Z = d;
      const double X2 = cs * X + sn * Z + ((p & 1) ? 1.0 : 0.0), Y2 = Y, Z2 = -sn * X + cs * Z;
      xy1[2 * i] = f * u + cx; xy1[2 * i + 1] = f * v + cy;
      xy2[2 * i] = f * X2 / Z2 + cx + uni(rng) - 0.5; xy2[2 * i + 1] = f * Y2 / Z2 + cy + uni(rng) - 0.5;
      if (i % 4 == 3) { xy2[2 * i] = 1000.0 * uni(rng); xy2[2 * i + 1] = 960.0 * uni(rng); }
    }
  std::vector<int32_t> pcam((size_t)T * 2 + 2, 0), model(1, 1), st((size_t)T + 1), ni((size_t)T + 1), nr((size_t)T + 1), nt((size_t)T + 1);
  std::vector<double> params(PXR_KPAD, 0.0), H((size_t)T * 9 + 9), q((size_t)T * 4 + 4), err((size_t)N + 1);
  std::vector<uint8_t> inl((size_t)N + 1);
  params[0] = params[1] = f; params[2] = cx; params[3] = cy;
  pxr_homography_options o;
  pxr_homography_default_options(&o);
  pxr_ctx* ctx = emu_ctx();
  const int rc = pxr_homography(ctx, T, off.data(), N, xy1.data(), xy2.data(), pcam.data(), 1, model.data(), params.data(), &o, H.data(),
                                q.data(), st.data(), ni.data(), nr.data(), nt.data(), inl.data(), err.data());
  if (rc) { printf("error %d: %s\n", rc, emu_last_error()); return 1; }
  for (int32_t p = 0; p < T; ++p)
    printf("pair %d: %lld matches, status %d, %d inliers, %d rotation inliers, %d trials\n", p, (long long)(off[p + 1] - off[p]), st[p],
           ni[p], nr[p], nt[p]);
  emu_ctx_free(ctx);
  return 0;
}
#endif

// the four-point solver alone (tests/test_minimal_solvers_cpu.py): n samples of four records (x1, y1, x2, y2) -> H, valid[s] = 0
// where there is none
extern "C" void emu_four_point(int n, const double* rec, double* H, uint8_t* valid) {
  for (int s = 0; s < n; ++s) {
    const double* r[4];
    for (int m = 0; m < 4; ++m) r[m] = rec + ((size_t)s * 4 + m) * 4;
    valid[s] = pxr::hg_four_point(r, H + (size_t)s * 9) ? 1 : 0;
  }
}
