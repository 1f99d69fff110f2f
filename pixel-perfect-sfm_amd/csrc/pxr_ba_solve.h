// pxr_ba_solve.h -- device-side structures shared by the BA solver's translation units (pxr_ba_lists.hip: block layout and
// observation lists; pxr_ba_solve.hip: linearisation, direct Schur + Cholesky path, LM loop; pxr_ba_pcg.hip: the iterative
// Schur path), and the layout of the scalar block.  The host side of the driver is in pxr_ba_driver.h.  Not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <functional>

#include "pixsfm_hip.h"
#include "pxr_ba_structure.h"
#include "pxr_device.h"
#include "pxr_internal.h"

namespace pxr {

static_assert(sizeof(IntPair) == sizeof(int2) && alignof(IntPair) == alignof(int2), "IntPair tables are read as int2 by the kernels");
inline const int2* as_int2(const IntPair* p) { return reinterpret_cast<const int2*>(p); }

// ---- the scalar block of an LM attempt: kScalSlots doubles, their integer limbs (deterministic mode), the factorisation's info
// word, the diagonal statistics of the newest linearisation.  One memset / k_pinv's side job clears everything but the statistics,
// one copy brings the whole block to the host (read_scalars).  Slots below kScalRep are summed over the ranks (point side),
// the others are replicated (camera side: every rank computes them from identical inputs).
constexpr int kScalSlots = 16, kScalRep = 8;
enum ScalSlot : int {
  SCAL_COST = 0,                  // cost of the evaluated point
  SCAL_MODEL_PT = 1,              // model cost change delta.(D^2 delta - g), point part ...
  SCAL_STEP2_PT = 2,              // |step|^2
  SCAL_X2_PT = 3,                 // |x|^2
  SCAL_COST_BEFORE_INNER = 4,     // cost at the candidate before the inner iterations
  SCAL_GRAD_COUNT_PT = 5,         // gradient entries above the tolerance
  SCAL_MODEL_CAM = kScalRep + 0,  // ... and the camera parts
  SCAL_STEP2_CAM = kScalRep + 1,
  SCAL_X2_CAM = kScalRep + 2,
  SCAL_GRAD_COUNT_CAM = kScalRep + 4,
};
constexpr int kScalLimbs = kScalSlots;                               // [kScalSlots][PXR_LIMBS] long long
constexpr int kScalInfo = kScalLimbs + kScalSlots * PXR_LIMBS;       // one slot whose first 4 bytes are the info word
constexpr int kScalZeroed = kScalInfo + 1;                           // what an attempt clears
constexpr int kScalStats = kScalZeroed;                              // {max, sum, min of diag(U), trace}
constexpr int kScalAll = kScalStats + 4;
static_assert(kScalAll == 16 + 16 * PXR_LIMBS + 1 + 4, "scalar block layout");

struct SolveDev {          // device-side problem description shared by the kernels
  pxr_ba_view v;           // parameters being linearised (current or candidate)
  const int* pose_off; const int* pose_dim; const int* tmask;   // per image
  const int* intr_off; const int* intr_dim; const int* cmask;   // per camera
  const int* pt_var;                                             // per point
  const double* scale_c;   // [n_c]   Jacobi scaling, camera side
  const double* scale_p;   // [n_points][3]
  int n_c; int DC; int LS; // reduced system size, max camera-side columns, Lrec stride
  int ldS;                 // leading dimension of the reduced system buffer: n_c + 1 (rhs = last column)
};

// global column index of camera-side column `a` of an observation in image img / camera cam
__device__ __forceinline__ int col_index(const SolveDev& d, int img, int cam, int a) {
  return column_of(d.pose_off, d.pose_dim, d.intr_off, img, cam, a);
}

// Y_i = W_i T_p is formed on the fly where it is consumed (row a of observation i)
__device__ __forceinline__ void y_row(const double* __restrict__ W, const double* __restrict__ T, int64_t i, int a, int DC,
                                      int64_t pt, double& y0, double& y1, double& y2) {
  const double* Wi = W + ((size_t)i * DC + a) * 3;
  const double* Tp = T + 6 * (size_t)pt;
  const double w0 = Wi[0], w1 = Wi[1], w2 = Wi[2];
  y0 = w0 * Tp[0] + w1 * Tp[1] + w2 * Tp[2];
  y1 = w0 * Tp[1] + w1 * Tp[3] + w2 * Tp[4];
  y2 = w0 * Tp[2] + w1 * Tp[4] + w2 * Tp[5];
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

}  // namespace pxr
