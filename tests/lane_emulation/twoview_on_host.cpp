// csrc/pxr_twoview.hip as host code over the stand-in runtime (on_host.h, hip/hip_runtime.h).
// With -DTWOVIEW_ON_HOST_MAIN: a stand-alone program (for -fsanitize=address,undefined builds) that runs synthetic pairs of the
// match counts given on the command line -- 0 is an empty pair -- and prints every pair's status, inliers and trials.
#include "on_host.h"
#include "pxr_twoview.hip"

#ifdef TWOVIEW_ON_HOST_MAIN
#include <random>
int main(int argc, char** argv) {
  std::vector<int64_t> off(1, 0);
  for (int i = 1; i < argc; ++i) off.push_back(off.back() + atoll(argv[i]));
  const int32_t T = (int32_t)off.size() - 1;
  const int64_t N = off.back();
  std::mt19937_64 rng(7);
  std::uniform_real_distribution<double> uni(0.0, 1.0);
  // pinhole cameras (f 1200, c 500 / 480); camera 2 = a rotation of 0.1 rad about y and a baseline along x; every fourth match an outlier
  const double f = 1200.0, cx = 500.0, cy = 480.0, cs = cos(0.1), sn = sin(0.1);
  std::vector<double> xy1((size_t)N * 2 + 2), xy2((size_t)N * 2 + 2);
  for (int64_t i = 0; i < N; ++i) {
    const double u = uni(rng) * 0.7 - 0.35, v = uni(rng) * 0.7 - 0.35, d = 2.0 + 18.0 * uni(rng);
    const double X = u * d, Y = v * d, Z = d;
    const double X2 = cs * X + sn * Z + 1.0, Y2 = Y, Z2 = -sn * X + cs * Z;
    xy1[2 * i] = f * u + cx; xy1[2 * i + 1] = f * v + cy;
    xy2[2 * i] = f * X2 / Z2 + cx + uni(rng) - 0.5; xy2[2 * i + 1] = f * Y2 / Z2 + cy + uni(rng) - 0.5;
    if (i % 4 == 3) { xy2[2 * i] = 1000.0 * uni(rng); xy2[2 * i + 1] = 960.0 * uni(rng); }
  }
  std::vector<int32_t> pcam((size_t)T * 2 + 2, 0), model(1, 1), st((size_t)T + 1), ni((size_t)T + 1), nt((size_t)T + 1);
  std::vector<double> params(PXR_KPAD, 0.0), q((size_t)T * 4 + 4), t((size_t)T * 3 + 3), E((size_t)T * 9 + 9), err((size_t)N + 1);
  std::vector<uint8_t> inl((size_t)N + 1);
  params[0] = params[1] = f; params[2] = cx; params[3] = cy;
  pxr_two_view_options o;
  pxr_two_view_default_options(&o);
  pxr_ctx* ctx = emu_ctx();
  int rc = pxr_two_view_geometry(ctx, T, off.data(), N, xy1.data(), xy2.data(), pcam.data(), 1, model.data(), params.data(), nullptr, nullptr,
                                 &o, q.data(), t.data(), E.data(), st.data(), ni.data(), nt.data(), inl.data(), err.data());
  if (rc) { printf("error %d: %s\n", rc, emu_last_error()); return 1; }
  for (int32_t p = 0; p < T; ++p)
    printf("pair %d: %lld matches, status %d, %d inliers, %d trials\n", p, (long long)(off[p + 1] - off[p]), st[p], ni[p], nt[p]);
  // the same pairs under the pose they were made with
  std::vector<double> pq((size_t)T * 4 + 4), pt((size_t)T * 3 + 3);
  for (int32_t p = 0; p < T; ++p) { pq[4 * p] = cos(0.05); pq[4 * p + 1] = 0.0; pq[4 * p + 2] = sin(0.05); pq[4 * p + 3] = 0.0; pt[3 * p] = 1.0; pt[3 * p + 1] = pt[3 * p + 2] = 0.0; }
  rc = pxr_two_view_geometry(ctx, T, off.data(), N, xy1.data(), xy2.data(), pcam.data(), 1, model.data(), params.data(), pq.data(), pt.data(),
                             &o, q.data(), t.data(), E.data(), st.data(), ni.data(), nt.data(), inl.data(), err.data());
  if (rc) { printf("error %d: %s\n", rc, emu_last_error()); return 1; }
  for (int32_t p = 0; p < T; ++p) printf("pair %d with its pose given: status %d, %d inliers, %d trials\n", p, st[p], ni[p], nt[p]);
  emu_ctx_free(ctx);
  return 0;
}
#endif

// the five-point solver alone (tests/test_minimal_solvers_cpu.py): n samples of five records (x1, y1, x2, y2) -> E of each real
// root in ascending order, valid[10 s + k] = 0 where there is none
extern "C" void emu_five_point(int n, const double* rec, double* E, uint8_t* valid) {
  for (int s = 0; s < n; ++s) {
    const double* r[5];
    for (int m = 0; m < 5; ++m) r[m] = rec + ((size_t)s * 5 + m) * 4;
    pxr::TvSolver sol;
    const bool ok = pxr::tv_solver_setup(r, sol);
    for (int k = 0; k < 10; ++k)
      valid[10 * s + k] = ok && k < sol.n_roots && pxr::tv_essential(sol, pxr::tv_root(sol, k), E + (size_t)(10 * s + k) * 9) ? 1 : 0;
  }
}

// the root stage alone: the scaled polynomial det B(z) (11 ascending coefficients), its count of real roots and the roots as
// tv_root returns them (before any polish), n_roots[s] = -1 where the sample gives no polynomial
extern "C" void emu_five_point_roots(int n, const double* rec, double* c, int32_t* n_roots, double* roots) {
  for (int s = 0; s < n; ++s) {
    const double* r[5];
    for (int m = 0; m < 5; ++m) r[m] = rec + ((size_t)s * 5 + m) * 4;
    pxr::TvSolver sol;
    n_roots[s] = -1;
    if (!pxr::tv_solver_setup(r, sol)) continue;
    n_roots[s] = sol.n_roots;
    for (int k = 0; k <= pxr::TV_DEG; ++k) c[(size_t)s * 11 + k] = sol.c[k];
    for (int k = 0; k < sol.n_roots; ++k) roots[(size_t)s * 10 + k] = pxr::tv_root(sol, k);
  }
}
