// csrc/pxr_abspose.hip as host code over the stand-in runtime (on_host.h, hip/hip_runtime.h).
#include "on_host.h"
#include "pxr_abspose.hip"

// the P3P solver alone (tests/test_minimal_solvers_cpu.py): n samples of three records (u, v, X, Y, Z) -> the pose of each of the
// four roots, valid[4 s + root] = 0 where the root gives none
extern "C" void emu_p3p(int n, const double* rec, double* R, double* t, uint8_t* valid) {
  for (int s = 0; s < n; ++s) {
    const double* r = rec + (size_t)s * 3 * pxr::ABS_REC;
    pxr::P3P p3;
    const bool ok = pxr::p3p_setup(r, r + pxr::ABS_REC, r + 2 * pxr::ABS_REC, p3);
    for (int root = 0; root < 4; ++root)
      valid[4 * s + root] = ok && pxr::p3p_pose(p3, root, R + (size_t)(4 * s + root) * 9, t + (size_t)(4 * s + root) * 3) ? 1 : 0;
  }
}
