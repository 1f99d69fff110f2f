// pxr_ba_cov.h -- what the covariance estimation (pxr_ba_cov.hip) takes from the BA solver (pxr_ba_solve.hip) and from the dense
// inverse (pxr_spd_inverse.hip).  Not part of the C-ABI.
#pragma once
#include <functional>

#include "pxr_ba_solve.h"

namespace pxr {

// The undamped linearisation at the caller's records with the point blocks eliminated and S factored: device pointers into the
// solver's work buffers, valid inside the callback of ba_cov_system only.
struct CovSystem {
  SolveDev dv;                  // block layout, constancy tables, scale_c: the power of two of every camera-side column
  int n_c = 0, DC = 1;
  double* aug = nullptr;        // [S | rhs] after chol_factor_solve: L below the diagonal tiles (column-major, ld = n_c + 1)
  double* linv = nullptr;       // the factorisation's workspace: inverses and factors of the diagonal tiles
  double* xsol = nullptr;       // n_c doubles
  int* d_info = nullptr;        // the factorisation's info word
  double* scratch = nullptr;    // n_c x n_c doubles, free
  const double* W = nullptr;    // [n_obs][DC][3]  B^T M~ E of the SCALED camera-side columns
  const double* T = nullptr;    // [n_points][6]   inv(V_p), zero for constant and singular points
  const int64_t* pt_ptr = nullptr;
  const int64_t* pt_obs = nullptr;
  bool deterministic = false;
};

// pxr_ba_solve.hip: structure, buffers and linearisation of a solve at the records d_rec, then `then` while they are alive.
// d_singular: [n_points] flags, d_n_singular: their count (both filled by k_pinv_checked)
int ba_cov_system(pxr_ctx* ctx, const pxr_ba_view* view, const double* d_rec, const pxr_loss* loss, const uint8_t* h_pose_const,
                  const uint8_t* h_tvec_const_mask, const uint16_t* h_cam_const_mask, const uint8_t* h_point_const, int* d_singular,
                  unsigned long long* d_n_singular, const std::function<int(const CovSystem&)>& then);

// pxr_spd_inverse.hip: inv(A) = inv(L)^T inv(L) into out (n x n row-major, symmetric bit for bit) from what chol_factor_solve left
// in aug and linv_ws; aug is overwritten.  No host synchronisation.
int spd_inverse_from_factor(hipStream_t st, double* aug, int n, double* out, const double* linv_ws);
size_t spd_inverse_max_n();

}  // namespace pxr
