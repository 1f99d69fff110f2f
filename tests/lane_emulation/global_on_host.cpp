// csrc/pxr_global.hip as host code over the stand-in runtime (on_host.h, hip/hip_runtime.h), with a plain host Cholesky in place of
// pxr_chol.hip's chol_factor_solve (same layout: (n + 1) x (n + 1) row-major, the upper triangle of the matrix in rows and columns
// 0 .. n - 1, the right-hand side in column n; *d_info = the 1-based column of the first non-positive pivot).
// With -DGLOBAL_ON_HOST_MAIN: a stand-alone program (for -fsanitize=address,undefined builds) that runs both entry points on a ring
// of `argv[1]` images with tracks of the lengths given after it, every array allocated at its exact size, and prints the statuses.
#include "on_host.h"
#include "pxr_global.hip"

namespace pxr {
size_t chol_workspace_doubles(int) { return 1; }
int chol_factor_solve(hipStream_t, double* a, int n, int* d_info, double*, double* x_out, bool zero_info) {
  const size_t ld = (size_t)n + 1;
  if (zero_info) *d_info = 0;
  std::vector<double> u((size_t)n * n, 0.0), z((size_t)n);
  for (int k = 0; k < n; ++k) {                                   // A = U^t U, row k of U
    double d = a[k * ld + k];
    for (int s = 0; s < k; ++s) d -= u[(size_t)s * n + k] * u[(size_t)s * n + k];
    if (!(d > 0.0)) { if (*d_info == 0) *d_info = k + 1; return PXR_OK; }
    const double r = std::sqrt(d);
    u[(size_t)k * n + k] = r;
    for (int c = k + 1; c < n; ++c) {
      double v = a[k * ld + c];
      for (int s = 0; s < k; ++s) v -= u[(size_t)s * n + k] * u[(size_t)s * n + c];
      u[(size_t)k * n + c] = v / r;
    }
  }
  for (int k = 0; k < n; ++k) {                                   // U^t z = b
    double v = a[k * ld + n];
    for (int s = 0; s < k; ++s) v -= u[(size_t)s * n + k] * z[s];
    z[k] = v / u[(size_t)k * n + k];
  }
  for (int k = n - 1; k >= 0; --k) {                              // U x = z
    double v = z[k];
    for (int c = k + 1; c < n; ++c) v -= u[(size_t)k * n + c] * x_out[c];
    x_out[k] = v / u[(size_t)k * n + k];
  }
  return PXR_OK;
}
}  // namespace pxr

#ifdef GLOBAL_ON_HOST_MAIN
#include <random>
int main(int argc, char** argv) {
  if (argc < 3) { printf("usage: n_images track_length...\n"); return 2; }
  const int n = atoi(argv[1]);
  std::mt19937_64 rng(7);
  std::normal_distribution<double> gauss(0.0, 1.0);
  std::uniform_real_distribution<double> cube(-2.0, 2.0);
  const double f = 1200.0, cx = 800.0, cy = 600.0, radius = 10.0;
  // ring cameras looking at the origin: rotation about y by the ring angle, as quaternions; c = -R^t t
  std::vector<double> q(4 * (size_t)n), c(3 * (size_t)n);
  for (int k = 0; k < n; ++k) {
    const double ang = 2.0 * 3.14159265358979323846 * k / n;
    c[3 * k] = radius * std::cos(ang); c[3 * k + 1] = 0.0; c[3 * k + 2] = radius * std::sin(ang);
    // the camera's z axis points at the origin: yaw = atan2(-cx, -cz) about y
    const double yaw = std::atan2(-c[3 * k], -c[3 * k + 2]);
    const double om[3] = {0.02 * gauss(rng), -yaw + 0.02 * gauss(rng), 0.02 * gauss(rng)};
    pxr::quat_exp(om, &q[4 * k]);
    pxr::quat_canonical(&q[4 * k]);
  }
  auto rotate = [&](int k, const double* X, double* out) {        // R_k X
    double R[9];
    pxr::quat_to_rotation(&q[4 * k], R);
    for (int r = 0; r < 3; ++r) out[r] = R[3 * r] * X[0] + R[3 * r + 1] * X[1] + R[3 * r + 2] * X[2];
  };
  // tracks: the last image observes nothing; one keypoint in seven is not finite
  std::vector<int64_t> off(1, 0);
  std::vector<int32_t> obs_image;
  std::vector<double> obs_xy;
  for (int a = 2; a < argc; ++a) {
    const int L = atoi(argv[a]);
    const double X[3] = {cube(rng), cube(rng), cube(rng)};
    for (int k = 0; k < L; ++k) {
      const int img = (int)((a * 5 + k) % (n - 1));
      double d[3] = {X[0] - c[3 * img], X[1] - c[3 * img + 1], X[2] - c[3 * img + 2]}, x[3];
      rotate(img, d, x);
      obs_image.push_back(img);
      const bool nan = obs_image.size() % 7 == 3;
      obs_xy.push_back(nan ? std::nan("") : f * x[0] / x[2] + cx + 0.5 * gauss(rng));
      obs_xy.push_back(f * x[1] / x[2] + cy + 0.5 * gauss(rng));
    }
    off.push_back((int64_t)obs_image.size());
  }
  const int64_t T = (int64_t)off.size() - 1, N = (int64_t)obs_image.size();
  // pairs one and two apart, exact relative rotations and baselines with a little noise; every fifth weight zero among the second kind
  std::vector<int32_t> pim;
  std::vector<double> pq, pdir, pw;
  for (int step = 1; step <= 2; ++step)
    for (int i = 0; i < n; ++i) {
      const int j = (i + step) % n;
      double ci[4], rel[4];
      pxr::quat_conj(&q[4 * i], ci);
      pxr::quat_mul(&q[4 * j], ci, rel);
      double b[3] = {c[3 * j] - c[3 * i] + 0.05 * gauss(rng), c[3 * j + 1] - c[3 * i + 1] + 0.05 * gauss(rng), c[3 * j + 2] - c[3 * i + 2] + 0.05 * gauss(rng)};
      const double nb = std::sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
      pim.push_back(i); pim.push_back(j);
      for (int k = 0; k < 4; ++k) pq.push_back(rel[k] + 1e-3 * gauss(rng));
      for (int k = 0; k < 3; ++k) pdir.push_back(b[k] / nb);
      pw.push_back(step == 2 && i % 5 == 0 ? 0.0 : 50.0 + (i * 37) % 150);
    }
  const int P = (int)pw.size();
  std::vector<int32_t> image_camera((size_t)n, 0), cam_model(1, PXR_SIMPLE_PINHOLE);
  std::vector<double> cam_params(PXR_KPAD, 0.0);
  cam_params[0] = f; cam_params[1] = cx; cam_params[2] = cy;

  pxr_ctx* ctx = emu_ctx();
  pxr_rotavg_options ro;
  pxr_rotavg_default_options(&ro);
  std::vector<double> qvec(4 * (size_t)n), angle((size_t)P);
  int32_t root = -1, iterations = -1;
  int rc = pxr_rotation_averaging(ctx, n, P, pim.data(), pq.data(), pw.data(), &ro, qvec.data(), &root, &iterations, angle.data());
  if (rc) { printf("error %d: %s\n", rc, g_err); return 1; }
  double worst = 0.0;
  for (int p = 0; p < P; ++p) worst = std::max(worst, angle[p]);
  printf("rotation averaging: root %d iterations %d largest residual %.3e rad\n", root, iterations, worst);

  // the baselines above are in the ground-truth world frame; the averaged rotations live in the root's camera frame: b -> R_root b
  for (int p = 0; p < P; ++p) {
    double out[3];
    rotate(root, &pdir[3 * p], out);
    const double nb = std::sqrt(out[0] * out[0] + out[1] * out[1] + out[2] * out[2]);
    for (int k = 0; k < 3; ++k) pdir[3 * p + k] = out[k] / nb;
  }
  pxr_tri_view v = {};
  v.n_tracks = T; v.d_track_offsets = off.data(); v.n_obs = N; v.d_obs_image = obs_image.data(); v.d_obs_xy = obs_xy.data();
  v.n_images = n; v.d_image_camera = image_camera.data(); v.d_qvec = qvec.data(); v.n_cameras = 1; v.d_cam_model = cam_model.data();
  v.d_cam_params = cam_params.data();
  pxr_globalpos_options go;
  pxr_globalpos_default_options(&go);
  std::vector<double> centre(3 * (size_t)n), xyz(3 * (size_t)T), obs_w((size_t)N), pair_w((size_t)P);
  std::vector<int32_t> status((size_t)T);
  int32_t h_status = -1, rounds = -1;
  rc = pxr_global_positioning(ctx, &v, P, pim.data(), pdir.data(), pw.data(), root, &go, centre.data(), xyz.data(), status.data(),
                              obs_w.data(), pair_w.data(), &h_status, &rounds);
  if (rc) { printf("error %d: %s\n", rc, g_err); return 1; }
  int64_t points = 0, rejected = 0;
  for (int64_t t = 0; t < T; ++t) points += status[t] == 0;
  for (int64_t o = 0; o < N; ++o) rejected += obs_w[o] == 0.0;
  double span = 0.0;
  for (int k = 0; k < n; ++k) span = std::max(span, std::sqrt(centre[3 * k] * centre[3 * k] + centre[3 * k + 1] * centre[3 * k + 1] + centre[3 * k + 2] * centre[3 * k + 2]));
  printf("global positioning: status %d rounds %d tracks %lld points %lld rejected %lld of %lld span %.3f\n", h_status, rounds, (long long)T,
         (long long)points, (long long)rejected, (long long)N, span);
  emu_ctx_free(ctx);
  return 0;
}
#endif
