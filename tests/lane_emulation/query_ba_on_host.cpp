// csrc/pxr_query_ba.hip as host code over the stand-in runtime (on_host.h, hip/hip_runtime.h).  The stand-in has no uint4, which
// the texel loads of pxr_interp.h use: it is defined here.  emu_arena / emu_arena_free make the pxr_arena an entry point reads
// (host pointers stand for device pointers).
// With -DQUERY_BA_ON_HOST_MAIN: a stand-alone program (for -fsanitize=address,undefined builds) that runs pxr_query_ba_solve once
// on a batch whose queries have the block counts argv[1..] (default 0 1 16 17), every array allocated at its exact size, and
// prints every query's summary.
#include "on_host.h"
struct uint4 { unsigned x, y, z, w; };
inline uint4 make_uint4(unsigned x, unsigned y, unsigned z, unsigned w) { return {x, y, z, w}; }
#include "pxr_query_ba.hip"

extern "C" pxr_arena* emu_arena(int dtype, int C, int H, int W, int64_t n, void* data, int32_t* corners, double* scales) {
  pxr_arena* a = new pxr_arena();
  a->dtype = dtype; a->C = C; a->H = H; a->W = W; a->n = n; a->d_data = data; a->d_corners = corners; a->d_scales = scales;
  return a;
}
extern "C" void emu_arena_free(pxr_arena* a) { delete a; }
extern "C" void emu_arena_set_upsampling(pxr_arena* a, double up) { a->up = up; }

#ifdef QUERY_BA_ON_HOST_MAIN
#include <random>
int main(int argc, char** argv) {
  std::vector<int64_t> off(1, 0);
  if (argc > 1) for (int i = 1; i < argc; ++i) off.push_back(off.back() + atoll(argv[i]));
  else for (int64_t n : {0, 1, 16, 17}) off.push_back(off.back() + n);
  const int32_t T = (int32_t)off.size() - 1;
  const int64_t N = off.back();
  const int C = 128, H = 16, W = 16;
  std::mt19937_64 rng(11);
  std::uniform_real_distribution<double> uni(0.0, 1.0);
  // one SIMPLE_RADIAL camera looking down the z axis; every block's point projects into the middle of its own patch
  std::vector<int32_t> cam_model = {PXR_SIMPLE_RADIAL}, query_camera(T, 0);
  std::vector<double> cam_params(PXR_KPAD, 0.0);
  cam_params[0] = 600.0; cam_params[1] = 500.0; cam_params[2] = 500.0; cam_params[3] = 0.01;
  std::vector<_Float16> patches((size_t)N * H * W * C);
  for (auto& v : patches) v = (_Float16)uni(rng);
  std::vector<int32_t> corners(2 * N);
  std::vector<double> scales(2 * N, 1.0), xyz(3 * N), refs((size_t)N * C);
  std::vector<int64_t> obs_patch(N);
  for (int64_t i = 0; i < N; ++i) {
    const double X = uni(rng) - 0.5, Y = uni(rng) - 0.5, Z = 4.0 + uni(rng);
    xyz[3 * i] = X; xyz[3 * i + 1] = Y; xyz[3 * i + 2] = Z;
    corners[2 * i] = (int32_t)floor(600.0 * X / Z + 500.0 - W / 2.0);
    corners[2 * i + 1] = (int32_t)floor(600.0 * Y / Z + 500.0 - H / 2.0);
    obs_patch[i] = N - 1 - i;
  }
  {                                                       // a patch belongs to the block that names it
    std::vector<int32_t> c2(2 * N);
    for (int64_t i = 0; i < N; ++i) { c2[2 * obs_patch[i]] = corners[2 * i]; c2[2 * obs_patch[i] + 1] = corners[2 * i + 1]; }
    corners = c2;
  }
  for (auto& v : refs) v = uni(rng) * 0.12;
  std::vector<double> qvec(4 * (size_t)T), tvec(3 * (size_t)T);
  for (int32_t q = 0; q < T; ++q) {
    qvec[4 * q] = 1.0; qvec[4 * q + 1] = 1e-3; qvec[4 * q + 2] = -2e-3; qvec[4 * q + 3] = 5e-4;
    tvec[3 * q] = 0.01; tvec[3 * q + 1] = -0.01; tvec[3 * q + 2] = 0.02;
  }
  pxr_ctx* ctx = emu_ctx();
  pxr_arena* arena = emu_arena(PXR_F16, C, H, W, N, patches.data(), corners.data(), scales.data());
  pxr_interp_cfg cfg = {1, 0, 0};
  pxr_loss loss = {PXR_LOSS_CAUCHY, 0.25};
  pxr_lm_options opt = {};
  opt.max_iterations = 4; opt.initial_radius = 1e4; opt.max_radius = 1e16; opt.min_radius = 1e-32; opt.min_relative_decrease = 1e-3;
  opt.min_lm_diagonal = 1e-6; opt.max_lm_diagonal = 1e32; opt.max_consecutive_invalid_steps = 10; opt.jacobi_scaling = 1;
  std::vector<pxr_lm_summary> sum(T);
  const int rc = pxr_query_ba_solve(ctx, arena, T, off.data(), N, obs_patch.data(), xyz.data(), refs.data(), query_camera.data(), 1,
                                    cam_model.data(), cam_params.data(), qvec.data(), tvec.data(), &cfg, &loss, &opt, sum.data());
  if (rc) { printf("error %d: %s\n", rc, g_err); return 1; }
  for (int32_t q = 0; q < T; ++q)
    printf("query %d blocks %lld iterations %d successful %d termination %d cost %.17g -> %.17g\n", (int)q, (long long)(off[q + 1] - off[q]),
           sum[q].iterations, sum[q].num_successful, sum[q].termination, sum[q].initial_cost, sum[q].final_cost);
  emu_arena_free(arena);
  emu_ctx_free(ctx);
  return 0;
}
#endif
