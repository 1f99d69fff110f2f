// csrc/pxr_fundamental.hip as host code over the stand-in runtime (on_host.h, hip/hip_runtime.h).
// With -DFUNDAMENTAL_ON_HOST_MAIN: a stand-alone program (for -fsanitize=address,undefined builds) that runs synthetic pairs of
// the match counts given on the command line -- 0 is an empty pair -- through a focal length stated 0.7 times too long on odd
// pairs, and prints every pair's status, inliers and trials.
#include "on_host.h"
#include "pxr_fundamental.hip"

#ifdef FUNDAMENTAL_ON_HOST_MAIN
#include <random>
int main(int argc, char** argv) {
  std::vector<int64_t> off(1, 0);
  for (int i = 1; i < argc; ++i) off.push_back(off.back() + atoll(argv[i]));
  const int32_t T = (int32_t)off.size() - 1;
  const int64_t N = off.back();
  std::mt19937_64 rng(7);
  std::uniform_real_distribution<double> uni(0.0, 1.0);
  // the scene is seen through pinhole cameras (f 1200, c 500 / 480); camera 2 = a rotation of 0.1 rad about y and a baseline
  // along x, depths 2-20; every fourth match an outlier.  Camera 0 is the true one, camera 1 states f x 0.7 (odd pairs use it)
  const double f = 1200.0, cx = 500.0, cy = 480.0, cs = cos(0.1), sn = sin(0.1);
  std::vector<double> xy1((size_t)N * 2 + 2), xy2((size_t)N * 2 + 2);
  for (int32_t p = 0; p < T; ++p)
    for (int64_t i = off[p]; i < off[p + 1]; ++i) {
      const double u = uni(rng) * 0.7 - 0.35, v = uni(rng) * 0.7 - 0.35, d = 2.0 + 18.0 * uni(rng);
      const double X = u * d, Y = v * d, Z = d;
      const double X2 = cs * X + sn * Z + 1.0, Y2 = Y, Z2 = -sn * X + cs * Z;
      xy1[2 * i] = f * u + cx; xy1[2 * i + 1] = f * v + cy;
      xy2[2 * i] = f * X2 / Z2 + cx + uni(rng) - 0.5; xy2[2 * i + 1] = f * Y2 / Z2 + cy + uni(rng) - 0.5;
      if (i % 4 == 3) { xy2[2 * i] = 1000.0 * uni(rng); xy2[2 * i + 1] = 960.0 * uni(rng); }
    }
  std::vector<int32_t> pcam((size_t)T * 2 + 2, 0), model(2, 1), st((size_t)T + 1), ni((size_t)T + 1), nt((size_t)T + 1);
  for (int32_t p = 0; p < T; ++p) pcam[2 * p] = pcam[2 * p + 1] = p & 1;
  std::vector<double> params(2 * PXR_KPAD, 0.0), F((size_t)T * 9 + 9), err((size_t)N + 1);
  std::vector<uint8_t> inl((size_t)N + 1);
  for (int c = 0; c < 2; ++c) {
    double* k = params.data() + c * PXR_KPAD;
    k[0] = k[1] = c ? 0.7 * f : f; k[2] = cx; k[3] = cy;
  }
  pxr_fundamental_options o;
  pxr_fundamental_default_options(&o);
  pxr_ctx* ctx = emu_ctx();
  const int rc = pxr_fundamental(ctx, T, off.data(), N, xy1.data(), xy2.data(), pcam.data(), 2, model.data(), params.data(), &o, F.data(),
                                 st.data(), ni.data(), nt.data(), inl.data(), err.data());
  if (rc) { printf("error %d: %s\n", rc, emu_last_error()); return 1; }
  for (int32_t p = 0; p < T; ++p)
    printf("pair %d: %lld matches, status %d, %d inliers, %d trials\n", p, (long long)(off[p + 1] - off[p]), st[p], ni[p], nt[p]);
  emu_ctx_free(ctx);
  return 0;
}
#endif

// the seven-point solver alone (tests/test_minimal_solvers_cpu.py): n samples of seven records (x1, y1, x2, y2) -> F of each real
// root in ascending order, valid[3 s + k] = 0 where there is none
extern "C" void emu_seven_point(int n, const double* rec, double* F, uint8_t* valid) {
  for (int s = 0; s < n; ++s) {
    const double* r[7];
    for (int m = 0; m < 7; ++m) r[m] = rec + ((size_t)s * 7 + m) * 4;
    pxr::FmSolver sol;
    const bool ok = pxr::fm_solver_setup(r, sol);
    for (int k = 0; k < 3; ++k)
      valid[3 * s + k] = ok && k < sol.n_roots && pxr::fm_fundamental(sol, pxr::fm_root(sol, k), F + (size_t)(3 * s + k) * 9) ? 1 : 0;
  }
}

// the root stage alone: the scaled cubic (4 ascending coefficients), its count of real roots and the roots as fm_root returns
// them, n_roots[s] = -1 where the sample gives no cubic
extern "C" void emu_seven_point_roots(int n, const double* rec, double* c, int32_t* n_roots, double* roots) {
  for (int s = 0; s < n; ++s) {
    const double* r[7];
    for (int m = 0; m < 7; ++m) r[m] = rec + ((size_t)s * 7 + m) * 4;
    pxr::FmSolver sol;
    n_roots[s] = -1;
    if (!pxr::fm_solver_setup(r, sol)) continue;
    n_roots[s] = sol.n_roots;
    for (int k = 0; k <= pxr::FM_DEG; ++k) c[(size_t)s * 4 + k] = sol.c[k];
    for (int k = 0; k < sol.n_roots; ++k) roots[(size_t)s * 3 + k] = pxr::fm_root(sol, k);
  }
}
