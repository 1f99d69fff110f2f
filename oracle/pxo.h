/*
 * pxo.h -- CPU ORACLE for the featuremetric KA/BA hot path of cvg/pixel-perfect-sfm.
 *
 * THIS IS TEST INFRASTRUCTURE, NOT PRODUCT CODE.  Only tests/, __graft_entry__.smoke()
 * and bench.py's cpu_baseline leg may load liboracle.so.  The product path
 * (pixel-perfect-sfm_amd/) never links, imports or calls anything in this directory.
 *
 * It is a plain-C restatement (no Eigen / Ceres / COLMAP) of the reference's arithmetic.
 * Every function cites the reference file:line (relative to /root/reference) it follows;
 * [upstream] marks formulas that live in un-vendored third-party code (Ceres >= 2.1,
 * COLMAP 3.8) and are restated from their published algorithms.
 *
 * PARITY STATUS (round 6).  The reference's C++ path CANNOT BE BUILT in this image: every header on
 * it includes Eigen, Ceres, COLMAP, HighFive or Boost, none of which is installed, and no
 * stand-in headers are written for them (rounds 1-5 compiled the reference's files over builder-written
 * stand-ins and called the result "the reference"; that build and every vector made with it were
 * removed in round 6).  What pins this restatement:
 *   - the KNOWN-ANSWER cases of the reference's own tests, restated in tests/test_oracle_interp.py and
 *     tests/test_oracle_geometry.py: bicubic value + derivatives of biquadratics (interpolation_test.cc:21-185,
 *     1e-8), unit norm after L2 (:187-207, 1e-10), the Jet chain rule (:272-311), the SIMD path against
 *     Ceres' bicubic (:327-364, 1e-5; Ceres' published formula restated), projection round trips
 *     (projection_test.cc, 1e-6);
 *   - the reference's vendored third-party/half.hpp compiled from its own source (oracle/ref_half_shim.cc
 *     -> oracle/_ref/libpxo_ref_half.so): the fp16 rounding rules;
 *   - the reference's Python run here: find_problem_labels (tests/golden/packing_ref.npz), extract_patches
 *     (tests/golden/extract_ref.npz);
 *   - third-party code: scipy.optimize.least_squares (the OPTIMUM of the trust-region solves and the
 *     robust losses, tests/test_third_party_solver.py), scipy.spatial.transform (the rotation), numpy fp16.
 * PARITY UNPINNED (restated from the source, validated by finite differences / closed forms only): the
 * split of the bicubic's arithmetic into an fp32 horizontal and an fp64 vertical pass; the featuremetric
 * residual / Jacobian VALUES (A7-A10); KA / BA problem construction (A12-A17); reference extraction and
 * the IRLS loop (A19); cost maps; match-graph labelling; the query refinements; the COLMAP camera models
 * (A6); the loss functions and corrector (A20); the trust-region TRAJECTORY of Ceres (A14, A18).
 */
#ifndef PXO_H_
#define PXO_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { PXO_F16 = 0, PXO_F32 = 1, PXO_F64 = 2 };

/* COLMAP 3.8 camera model ids [upstream colmap/base/camera_models.h] */
enum {
  PXO_SIMPLE_PINHOLE = 0,
  PXO_PINHOLE = 1,
  PXO_SIMPLE_RADIAL = 2,
  PXO_RADIAL = 3,
  PXO_OPENCV = 4,
  PXO_OPENCV_FISHEYE = 5,
  PXO_FULL_OPENCV = 6,
  PXO_FOV = 7,
  PXO_SIMPLE_RADIAL_FISHEYE = 8,
  PXO_RADIAL_FISHEYE = 9,
  PXO_THIN_PRISM_FISHEYE = 10
};

/* Ceres loss functions [upstream ceres/loss_function.h] */
enum { PXO_LOSS_TRIVIAL = 0, PXO_LOSS_CAUCHY = 1, PXO_LOSS_HUBER = 2, PXO_LOSS_SOFTL1 = 3 };

/* FeaturePatch descriptor: features/src/featurepatch.h:40-156 (HWC, channel fastest). */
typedef struct {
  const void* data; /* H*W*C elements of dtype                                 */
  int32_t dtype;    /* PXO_F16 / PXO_F32 / PXO_F64                             */
  int32_t H, W, C;
  int32_t x0, y0;   /* corner_                                                 */
  double sx, sy;    /* scale_                                                  */
  double up;        /* upsampling_factor_ (1.0 for feature patches)            */
} pxo_patch;

/* InterpolationConfig (base/src/interpolation.h:39-51); BICUBIC, N_NODES=1 only. */
typedef struct {
  int32_t l2_normalize;
  int32_t use_float_simd;
  int32_t check_bounds;
} pxo_interp_cfg;

typedef struct {
  int32_t type;  /* PXO_LOSS_*                  */
  double a;      /* scale parameter             */
} pxo_loss;

/* ---- fp16 helpers -------------------------------------------------------------- */
float pxo_half_to_float(uint16_t h);
uint16_t pxo_float_to_half(float f);
void pxo_halfs_to_floats(const uint16_t* h, float* f, int64_t n);
void pxo_floats_to_halfs(const float* f, uint16_t* h, int64_t n);

/* ---- A2: Catmull-Rom spline + bicubic ------------------------------------------- */
/* cubic_hermite_spline_simd.h:123-192 (IN_T = half/float): fp32 math for channels
 * [0, C - C%8), scalar fp64 tail beyond; results widened to double. */
void pxo_spline_lowp(const void* p0, const void* p1, const void* p2, const void* p3,
                     int dtype, int C, double x, int round_out_to_float, double* f,
                     double* dfdx);
/* cubic_hermite_spline_simd.h:56-121 (double input). */
void pxo_spline_f64(const double* p0, const double* p1, const double* p2, const double* p3,
                    int C, double x, double* f, double* dfdx);
/* ceres::CubicHermiteSpline [upstream ceres/cubic_interpolation.h], all-fp64 Horner. */
void pxo_spline_ceres(const double* p0, const double* p1, const double* p2, const double* p3,
                      int C, double x, double* f, double* dfdx);
/* BiCubicInterpolator::Evaluate (interpolation.h:177-274): AVX2 path semantics for
 * C >= 8, scalar Ceres path for C < 8. (r,c) in patch texel coordinates. */
void pxo_bicubic(const pxo_patch* p, double r, double c, int use_float_simd, double* f,
                 double* dfdr, double* dfdc);
/* ceres::BiCubicInterpolator [upstream] on a border-clamped grid: all-fp64. */
void pxo_bicubic_ceres(const pxo_patch* p, double r, double c, double* f, double* dfdr,
                       double* dfdc);

/* ---- A3: PixelInterpolator::Evaluate (interpolation.h:642-677) -------------------- */
void pxo_pixel_interp_cross(const pxo_patch* p, double r, double c, const pxo_interp_cfg* cfg,
                            double* f, double* dfdr, double* dfdc, double* dfdrc);
void pxo_pixel_interp(const pxo_patch* p, double r, double c, const pxo_interp_cfg* cfg,
                      double* f, double* dfdr, double* dfdc);

/* ---- A1/A5: PatchInterpolator::Evaluate (patch_interpolator.h:125-135) ------------
 * xy in COLMAP image coordinates; returns is_inside (always 1 unless check_bounds).
 * dfdx/dfdy are derivatives w.r.t. the image coordinates (Jet bridge A4 applied to
 * featurepatch.h:250-255). Either may be NULL. */
int pxo_patch_eval(const pxo_patch* p, const double xy[2], const pxo_interp_cfg* cfg,
                   double* f, double* dfdx, double* dfdy);

/* ---- A6: projection ------------------------------------------------------------- */
int pxo_camera_num_params(int model);
/* CameraModel::WorldToImage [upstream COLMAP]; J_uv 2x2 row-major, J_k 2xK row-major. */
int pxo_world_to_image(int model, const double* params, double u, double v, double* x,
                       double* y, double* J_uv, double* J_k);
/* WorldToPixel (base/src/projection.h:60-75). Jacobians row-major 2x4, 2x3, 2x3, 2xK;
 * J_q is the ambient derivative (includes the normalisation inside
 * ceres::QuaternionRotatePoint). Any Jacobian pointer may be NULL. */
int pxo_world_to_pixel(int model, const double* params, const double q[4], const double t[3],
                       const double X[3], double xy[2], double* J_q, double* J_t, double* J_X,
                       double* J_k);

/* ---- A7-A10: residual functors ---------------------------------------------------- */
/* FeatureReferenceCostFunctor (residuals/src/feature_reference.h:98-137).
 * r[C]; Jacobians row-major C x {4,3,3,K} as ceres::AutoDiffCostFunction emits. */
int pxo_ba_residual(const pxo_patch* p, const pxo_interp_cfg* cfg, int model,
                    const double q[4], const double t[3], const double X[3],
                    const double* params, const double* ref, double* r, double* Jq,
                    double* Jt, double* JX, double* Jk);
/* FeatureMetric2DCostFunctor (residuals/src/featuremetric.h:44-63). J1,J2: C x 2. */
int pxo_ka_residual(const pxo_patch* p1, const pxo_patch* p2, const pxo_interp_cfg* cfg,
                    const double kp1[2], const double kp2[2], double* r, double* J1,
                    double* J2);
/* FeatureReference2DCostFunctor (residuals/src/feature_reference.h:44-60). */
int pxo_ref2d_residual(const pxo_patch* p, const pxo_interp_cfg* cfg, const double kp[2],
                       const double* ref, double* r, double* J);

/* ---- A20: robustifier [upstream ceres/loss_function.cc, corrector.cc] ------------- */
/* rho[0..2] = weight * (rho, rho', rho'') at s. */
void pxo_loss_eval(const pxo_loss* loss, double weight, double s, double rho[3]);
/* Corrector: in-place r~ = scale*r, J~ = sqrt(rho')(J - alpha/s r r^T J); J row-major C x n
 * (may be NULL). */
void pxo_corrector(double s, const double rho[3], int C, int n, double* r, double* J);

/* ---- A19: reference extraction ---------------------------------------------------- */
/* RobustMeanIRLS (base/src/irls_optim.h:24-71), N_NODES = 1. descs: n x C row-major.
 * Returns the index of an observation if the early-return branch (rho <= 0) is taken
 * (mean then holds that descriptor), else -1. */
int pxo_robust_mean_irls(const double* descs, int n, int C, const pxo_loss* loss, int iters,
                         int l2_normalize, double* mean);
/* ComputeReference (bundle_adjustment/src/reference_extractor.h:238-272): returns the
 * index of the observation closest to the robust mean; ref_out = that descriptor
 * (closest_to_robust_mean = true) . */
int pxo_compute_reference(const double* descs, int n, int C, const pxo_loss* loss, int iters,
                          int l2_normalize, double* ref_out, double* robust_mean_out);

/* ---- batch helpers (CPU baseline timing + test convenience) ----------------------- */
typedef struct {
  int64_t n_obs;
  const int32_t* obs_image;   /* [n_obs] */
  const int32_t* obs_point;   /* [n_obs] */
  const int64_t* obs_patch;   /* [n_obs] index into patches */
  const int32_t* image_camera;/* [n_images] */
  const double* qvec;         /* [n_images][4] */
  const double* tvec;         /* [n_images][3] */
  const int32_t* cam_model;   /* [n_cams] */
  const double* cam_params;   /* [n_cams][12] (padded) */
  const double* xyz;          /* [n_points][3] */
  const double* refs;         /* [n_points][C]; NULL = no reference is subtracted (costmap BA,
                               * bundle_adjustment/src/costmap_bundle_optimizer.h:104-119 passes nullptr) */
  /* uniform patch arena */
  const void* arena; int32_t dtype, H, W, C;
  const int32_t* corners;     /* [n_patches][2] */
  const double* scales;       /* [n_patches][2] */
  double upsampling;          /* FeaturePatch::upsampling_factor_ of every patch (1 for features; cost maps extracted
                               * with CostMapConfig.upsampling_factor carry it, costmap_extractor.h:399); 0 reads as 1 */
} pxo_ba_batch;

/* Evaluate residual + materialised 128 x n Jacobian blocks for obs [first, first+count),
 * the way ceres::AutoDiffCostFunction hands them to Ceres; returns sum of 0.5*rho(s).
 * Optional outputs (may be NULL): r_out [count][C], J_out [count][C][10+Kmax] with
 * column layout q(4) t(3) X(3) k(Kpad=12).  n_threads <= 1 -> serial. */
double pxo_ba_eval_batch(const pxo_ba_batch* b, const pxo_interp_cfg* cfg, const pxo_loss* loss,
                         int64_t first, int64_t count, int n_threads, double* r_out,
                         double* J_out);


/* ---- LM solvers [upstream Ceres 2.1 trust_region_minimizer.cc restated] -------------- */
enum { PXO_TERM_CONVERGENCE = 0, PXO_TERM_NO_CONVERGENCE = 1, PXO_TERM_FAILURE = 2 };

typedef struct {
  int32_t max_iterations;              /* 100 (base/main.py:9-22)                           */
  double function_tolerance;           /* 0                                                 */
  double gradient_tolerance;           /* 0                                                 */
  double parameter_tolerance;          /* 0 for BA, 1e-5 for KA (keypoint_adjustment/main.py:74) */
  double initial_radius;               /* 1e4  [upstream default]                           */
  double max_radius;                   /* 1e16                                              */
  double min_radius;                   /* 1e-32                                             */
  double min_relative_decrease;        /* 1e-3                                              */
  double min_lm_diagonal;              /* 1e-6                                              */
  double max_lm_diagonal;              /* 1e32                                              */
  int32_t max_consecutive_invalid_steps; /* 10 (bundle_adjustment_options.h:56)             */
  int32_t jacobi_scaling;              /* 1                                                 */
  int32_t use_inner_iterations;        /* BA only: True by default (bundle_adjustment/main.py:43) */
  double inner_iteration_tolerance;    /* 1e-3 [upstream]                                   */
} pxo_lm_options;

typedef struct {
  int32_t iterations;       /* LM iterations attempted (successful + rejected + invalid)   */
  int32_t num_successful;
  int32_t termination;      /* PXO_TERM_*                                                  */
  int32_t num_unknowns;
  double initial_cost, final_cost, final_radius;
} pxo_lm_summary;

/* Featuremetric BA on the flat problem (parameters are updated IN PLACE inside b, like the
 * reference does in the colmap::Reconstruction, feature_reference_bundle_optimizer.h:111-114).
 *   pose_const[img]        1 = SetParameterBlockConstant(qvec, tvec)   (bundle_optimizer.h:391-394)
 *   tvec_const_mask[img]   bit a = tvec[a] held by a SubsetManifold     (:385-390)
 *   cam_const_mask[cam]    bit a = camera param a constant              (:400-442)
 *   point_const[pt]        1 = constant point                           (:342-363)          */
int pxo_ba_solve(pxo_ba_batch* b, int n_images, int n_cams, int64_t n_points,
                 const pxo_interp_cfg* cfg, const pxo_loss* loss, const uint8_t* pose_const,
                 const uint8_t* tvec_const_mask, const uint16_t* cam_const_mask,
                 const uint8_t* point_const, const pxo_lm_options* opt, pxo_lm_summary* sum);

/* The same LM loop with the ITERATIVE reduced step the project specifies for scenes above 1000 images (include/pixsfm_hip.h:
 * pxr_lm_options; the header comment of csrc/pxr_ba_pcg.hip), on the dense scaled system: the 3 x 3 point blocks eliminated
 * (damped by diag / radius), preconditioned conjugate gradients on S x = b from x = 0 with Q = -(x.b + x.r) / 2 from the
 * recurrence residual, the points back-substituted exactly for that x, the model cost change from the full step
 * (-d.g - d.H.d / 2: never from the solver's residual).  The stops, in the order they are tested in iteration i:
 * rho = r.z zero or not finite (iteration not counted); p.Sp <= 0 (not counted, the last x kept); i (Q_i - Q_{i-1}) / Q_i < eta;
 * |r| <= r_tolerance |b| (r_tolerance > 0 only); i = max_linear_solver_iterations.  No counted iteration = invalid step.
 * Preconditioner: per pose block of an image / intrinsics block of a camera (joint where the camera has a single image)
 * A[g, g] - sum_i W_i[g] T_p W_i[g]^T -- the block diagonal of S without the cross terms of two observations of one point. */
typedef struct {
  int32_t max_linear_solver_iterations;  /* 200 (bundle_adjustment_options.h:55)   */
  double eta;                            /* 0.1 [upstream Solver::Options::eta]    */
  double r_tolerance;                    /* <= 0: off                              */
} pxo_linear_options;

enum { PXO_CG_STOP_MAX_ITERATIONS = 0, PXO_CG_STOP_Q = 1, PXO_CG_STOP_R_TOLERANCE = 2, PXO_CG_STOP_RHO = 3, PXO_CG_STOP_INDEFINITE = 4,
       PXO_CG_STOP_PRECONDITIONER = 5 /* a block (or a point block) is not positive definite */, PXO_CG_STOP_ZERO_RHS = 6 };

typedef struct {
  int32_t cg_iterations;       /* counted conjugate-gradient iterations of this LM iteration            */
  int32_t cg_stop;             /* PXO_CG_STOP_*                                                         */
  int32_t step_is_valid, step_is_successful;
  double relative_decrease;    /* cost change / model cost change (0 for an invalid step)               */
  double radius;               /* the radius AFTER this iteration                                       */
  /* |zeta - eta| / eta, zeta = i (Q_i - Q_{i-1}) / Q_i: at the last counted iteration, at the one before it, and the smallest
   * over the iterations of this solve; -1 where there is none (eta = 0, fewer iterations)             */
  double margin_last, margin_prev, margin_min;
} pxo_lm_trace_entry;

typedef struct {
  int32_t capacity;            /* entries the caller allocated                                          */
  int32_t count;               /* LM iterations that ended in a decision (may exceed capacity)          */
  pxo_lm_trace_entry* entries;
} pxo_lm_trace;

int pxo_ba_solve_iterative(pxo_ba_batch* b, int n_images, int n_cams, int64_t n_points,
                           const pxo_interp_cfg* cfg, const pxo_loss* loss, const uint8_t* pose_const,
                           const uint8_t* tvec_const_mask, const uint16_t* cam_const_mask,
                           const uint8_t* point_const, const pxo_lm_options* opt, const pxo_linear_options* lin,
                           pxo_lm_summary* sum, pxo_lm_trace* trace /* or NULL */);

/* The reduced system of the first LM iteration (radius = opt->initial_radius) at the batch's parameters; see pxo_solve.c. */
int pxo_ba_reduced_system(pxo_ba_batch* b, int n_images, int n_cams, int64_t n_points,
                          const pxo_interp_cfg* cfg, const pxo_loss* loss, const uint8_t* pose_const,
                          const uint8_t* tvec_const_mask, const uint16_t* cam_const_mask,
                          const uint8_t* point_const, const pxo_lm_options* opt, const pxo_linear_options* lin,
                          double* S_out, double* rhs_out, double* M_out, double* x_out, int32_t* col_group_out,
                          int32_t* cg_iterations);


/* ONE LM iteration with Schur elimination, staged and timed the way the reference's CPU path spends it
 * (pxo_lm_bench.c; OpenMP over observations / points): bench.py's cpu_baseline_lm and an independent check of a
 * first LM step.  times_ms [6]: Jacobian evaluation, Schur elimination, Cholesky + camera step, back-substitution,
 * residual-only evaluation, total.  delta_c_out [n_c] / delta_p_out [n_points][3] (tangent, unscaled) may be NULL. */
int pxo_ba_lm_iteration_schur(const pxo_ba_batch* b, int n_images, int n_cams, int64_t n_points,
                              const pxo_interp_cfg* cfg, const pxo_loss* loss, const uint8_t* pose_const,
                              const uint8_t* tvec_const_mask, const uint16_t* cam_const_mask,
                              const uint8_t* point_const, double radius, double min_diag, double max_diag,
                              int n_threads, int* n_c_out, double* delta_c_out, double* delta_p_out,
                              double* times_ms, double* cost_out);

/* ---- KA --------------------------------------------------------------------------------- */
typedef struct {
  int64_t n_nodes;
  double* kp;                 /* [n_nodes][2] keypoints, COLMAP coords, refined IN PLACE          */
  const int64_t* node_patch;  /* [n_nodes] patch of each node in the arena                        */
  const uint8_t* node_const;  /* [n_nodes] 1 = constant (track roots, KeypointAdjustmentSetup)    */
  int64_t n_edges;
  const int32_t* edge_src;    /* residual blocks: FeatureMetric2DCostFunctor(patch[src], patch[dst]) */
  const int32_t* edge_dst;
  const double* edge_w;       /* ScaledLoss weight (match similarity or 1)                        */
  const void* arena; int32_t dtype, H, W, C;
  const int32_t* corners; const double* scales;
  /* unary reference terms (localization QKA): FeatureReference2DCostFunctor(patch[node], ref)
   * (residuals/src/feature_reference.h:20-60, localization/src/query_keypoint_optimizer.h:122-139);
   * several entries may name the same node (stacked correspondences). n_unary may be 0. */
  int64_t n_unary;
  const int32_t* unary_node;  /* [n_unary]                                                        */
  const double* unary_ref;    /* [n_unary][C] reference descriptors                               */
  const double* unary_w;      /* [n_unary] ScaledLoss weight, NULL = 1                            */
} pxo_ka_batch;

/* One independent sub-problem (one ceres::Problem of RunSubset,
 * featuremetric_keypoint_optimizer.h:118-137): nodes[nn] / edges[m] index into the batch.
 * Ceres TR-LM with box bounds: ParameterBlock::Plus projects onto the bounds; projected Armijo
 * line search along the LM step (DoLineSearch) [upstream Ceres 2.1]. */
int pxo_ka_solve_problem(pxo_ka_batch* b, const int32_t* nodes, int nn, const int32_t* edges, int m,
                         const pxo_interp_cfg* cfg, const pxo_loss* loss, double bound,
                         const pxo_lm_options* opt, pxo_lm_summary* sum);
/* Same with this problem's unary reference terms unary[nu] (indices into the batch's unary arrays):
 * SingleQueryKeypointOptimizer::RunQuery builds ONE problem over all keypoints of a query
 * (localization/src/single_query_keypoint_optimizer.h:86-122). */
int pxo_ka_solve_problem_u(pxo_ka_batch* b, const int32_t* nodes, int nn, const int32_t* edges, int m,
                           const int32_t* unary, int nu, const pxo_interp_cfg* cfg, const pxo_loss* loss,
                           double bound, const pxo_lm_options* opt, pxo_lm_summary* sum);

/* The box bounds of one node: lower / upper (x, y) as KeypointOptimizerBase::ParameterizeKeypoints sets them
 * (keypoint_adjustment/src/keypoint_optimizer.h:124-152). */
void pxo_ka_node_bounds(const pxo_ka_batch* b, int64_t node, double bound, double lo[2], double hi[2]);

#ifdef __cplusplus
}
#endif
#endif /* PXO_H_ */
