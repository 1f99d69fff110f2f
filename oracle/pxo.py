"""ctypes binding of the CPU oracle (oracle/liboracle.so; oracle/_ref/libpxo_ref_half.so).

TEST INFRASTRUCTURE ONLY: imported by tests/, __graft_entry__.smoke() and the
cpu_baseline leg of bench.py.  The product package never imports this module.

PINNING STATUS (round 6).  The reference's C++ path cannot be built in this image (every header on it includes Eigen /
Ceres / COLMAP / HighFive, none of which is installed) and no stand-in headers are written for them.  The oracle is
therefore pinned ONLY by
  * the known-answer cases of the reference's own tests (base/src/interpolation_test.cc, irls_optim_test.cc,
    projection_test.cc), restated in tests/test_oracle_interp.py / test_oracle_geometry.py / test_irls.py;
  * the reference's vendored half.hpp compiled from its own source (oracle/ref_half_shim.cc): fp16 rounding rules;
  * the reference's Python functions run here (find_problem_labels, extract_patches; tests/golden/make_golden_*.py);
  * third-party code the builder did not write: scipy.optimize.least_squares (optimum of the trust-region solves and the
    robust losses), torch.autograd (the analytic Jacobians against automatic differentiation, what the reference itself uses),
    scipy.spatial.transform (rotation), numpy float16 (tests/test_third_party_*.py).
Everything else -- featuremetric residual / Jacobian values (A7-A10), problem construction (A12-A17), reference extraction
(A19), cost maps, the COLMAP camera models (A6), the trust-region TRAJECTORY (A14, A18) -- is a restatement read from the
reference's source (each function cites file:line) and validated by finite differences / closed forms: PARITY UNPINNED.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
F16, F32, F64 = 0, 1, 2
KPAD = 12
CAMERA_MODELS = {"SIMPLE_PINHOLE": 0, "PINHOLE": 1, "SIMPLE_RADIAL": 2, "RADIAL": 3, "OPENCV": 4, "OPENCV_FISHEYE": 5,
                 "FULL_OPENCV": 6, "FOV": 7, "SIMPLE_RADIAL_FISHEYE": 8, "RADIAL_FISHEYE": 9, "THIN_PRISM_FISHEYE": 10}
LOSSES = {"trivial": 0, "cauchy": 1, "huber": 2, "soft_l1": 3}
_NP2DT = {np.dtype(np.float16): F16, np.dtype(np.float32): F32, np.dtype(np.float64): F64}

c_double_p = C.POINTER(C.c_double)


class Patch(C.Structure):
    _fields_ = [("data", C.c_void_p), ("dtype", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("C", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("sx", C.c_double),
                ("sy", C.c_double), ("up", C.c_double)]


class InterpCfg(C.Structure):
    _fields_ = [("l2_normalize", C.c_int32), ("use_float_simd", C.c_int32),
                ("check_bounds", C.c_int32)]


class Loss(C.Structure):
    _fields_ = [("type", C.c_int32), ("a", C.c_double)]


class BaBatch(C.Structure):
    _fields_ = [("n_obs", C.c_int64), ("obs_image", C.c_void_p), ("obs_point", C.c_void_p),
                ("obs_patch", C.c_void_p), ("image_camera", C.c_void_p), ("qvec", C.c_void_p),
                ("tvec", C.c_void_p), ("cam_model", C.c_void_p), ("cam_params", C.c_void_p),
                ("xyz", C.c_void_p), ("refs", C.c_void_p), ("arena", C.c_void_p),
                ("dtype", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32),
                ("corners", C.c_void_p), ("scales", C.c_void_p), ("upsampling", C.c_double)]


def _newest(paths):
    return max((os.path.getmtime(p) for p in paths), default=0.0)


def build(force=False):
    """Compile liboracle.so and, when /root/reference is present, oracle/_ref/libpxo_ref_half.so (oracle/Makefile)."""
    so = os.path.join(HERE, "liboracle.so")
    srcs = [os.path.join(HERE, f) for f in os.listdir(HERE) if f.endswith((".c", ".h"))]
    if force or not os.path.exists(so) or _newest(srcs) > os.path.getmtime(so):
        subprocess.check_call(["make", "-C", HERE, "-s", "liboracle.so"], stdout=subprocess.DEVNULL)
    half = os.path.join(HERE, "_ref", "libpxo_ref_half.so")
    shim = os.path.join(HERE, "ref_half_shim.cc")
    if os.path.isfile("/root/reference/third-party/half.hpp") and (
            force or not os.path.exists(half) or os.path.getmtime(shim) > os.path.getmtime(half)):
        subprocess.check_call(["make", "-C", HERE, "-s", "ref"], stdout=subprocess.DEVNULL)
    return so


_lib = None
_ref = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.pxo_half_to_float.restype = C.c_float
        _lib.pxo_half_to_float.argtypes = [C.c_uint16]
        _lib.pxo_float_to_half.restype = C.c_uint16
        _lib.pxo_float_to_half.argtypes = [C.c_float]
        _lib.pxo_ba_eval_batch.restype = C.c_double
        _lib.pxo_ba_eval_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                           C.c_int, C.c_void_p, C.c_void_p]
    return _lib


def ref():
    """The reference's vendored third-party/half.hpp compiled from its own source (None if not built)."""
    global _ref
    if _ref is None:
        path = os.path.join(HERE, "_ref", "libpxo_ref_half.so")
        if not os.path.exists(path):
            return None
        _ref = C.CDLL(path)
    return _ref


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def make_patch(data, corner=(0, 0), scale=(1.0, 1.0), up=1.0):
    """data: HxWxC numpy array (f16/f32/f64), C-contiguous. Keeps a reference alive."""
    assert data.ndim == 3 and data.flags["C_CONTIGUOUS"]
    p = Patch(data.ctypes.data, _NP2DT[data.dtype], data.shape[0], data.shape[1], data.shape[2],
              int(corner[0]), int(corner[1]), float(scale[0]), float(scale[1]), float(up))
    p._keep = data
    return p


def cfg(l2_normalize=True, use_float_simd=False, check_bounds=False):
    return InterpCfg(int(l2_normalize), int(use_float_simd), int(check_bounds))


def loss(name="cauchy", a=0.25):
    return Loss(LOSSES[name], float(a))


def bicubic(patch, r, c, use_float_simd=False):
    n = patch.C
    f, dr, dc = (np.empty(n) for _ in range(3))
    lib().pxo_bicubic(C.byref(patch), C.c_double(r), C.c_double(c), int(use_float_simd), _p(f), _p(dr), _p(dc))
    return f, dr, dc


def bicubic_ceres(patch, r, c):
    n = patch.C
    f, dr, dc = (np.empty(n) for _ in range(3))
    lib().pxo_bicubic_ceres(C.byref(patch), C.c_double(r), C.c_double(c), _p(f), _p(dr), _p(dc))
    return f, dr, dc


def pixel_interp(patch, r, c, config):
    n = patch.C
    f, dr, dc = (np.empty(n) for _ in range(3))
    lib().pxo_pixel_interp(C.byref(patch), C.c_double(r), C.c_double(c), C.byref(config), _p(f), _p(dr), _p(dc))
    return f, dr, dc


def pixel_interp_cross(patch, r, c, config):
    """PixelInterpolator::Evaluate with the cross derivative (interpolation.h:642-677): f, df/dr, df/dc, d2f/drdc."""
    n = patch.C
    f, dr, dc, drc = (np.empty(n) for _ in range(4))
    lib().pxo_pixel_interp_cross(C.byref(patch), C.c_double(r), C.c_double(c), C.byref(config), _p(f), _p(dr), _p(dc), _p(drc))
    return f, dr, dc, drc


def patch_eval(patch, xy, config, want_grad=True):
    n = patch.C
    xy = np.ascontiguousarray(xy, dtype=np.float64)
    f = np.empty(n)
    gx, gy = (np.empty(n), np.empty(n)) if want_grad else (None, None)
    inside = lib().pxo_patch_eval(C.byref(patch), _p(xy), C.byref(config), _p(f), _p(gx), _p(gy))
    return f, gx, gy, inside


def world_to_image(model, params, u, v):
    K = lib().pxo_camera_num_params(model)
    params = np.ascontiguousarray(params, dtype=np.float64)
    x, y = C.c_double(), C.c_double()
    Juv, Jk = np.empty((2, 2)), np.empty((2, K))
    rc = lib().pxo_world_to_image(model, _p(params), C.c_double(u), C.c_double(v), C.byref(x), C.byref(y), _p(Juv), _p(Jk))
    assert rc == 0
    return np.array([x.value, y.value]), Juv, Jk


def world_to_pixel(model, params, q, t, X, jac=True):
    K = lib().pxo_camera_num_params(model)
    params, q, t, X = (np.ascontiguousarray(a, dtype=np.float64) for a in (params, q, t, X))
    xy = np.empty(2)
    if jac:
        Jq, Jt, JX, Jk = np.empty((2, 4)), np.empty((2, 3)), np.empty((2, 3)), np.empty((2, K))
    else:
        Jq = Jt = JX = Jk = None
    rc = lib().pxo_world_to_pixel(model, _p(params), _p(q), _p(t), _p(X), _p(xy), _p(Jq), _p(Jt), _p(JX), _p(Jk))
    assert rc == 0
    return xy, Jq, Jt, JX, Jk


def ba_residual(patch, config, model, q, t, X, params, ref_desc, jac=True):
    n = patch.C
    K = lib().pxo_camera_num_params(model)
    params, q, t, X = (np.ascontiguousarray(a, dtype=np.float64) for a in (params, q, t, X))
    ref_desc = None if ref_desc is None else np.ascontiguousarray(ref_desc, dtype=np.float64)
    r = np.empty(n)
    if jac:
        Jq, Jt, JX, Jk = np.empty((n, 4)), np.empty((n, 3)), np.empty((n, 3)), np.empty((n, K))
    else:
        Jq = Jt = JX = Jk = None
    rc = lib().pxo_ba_residual(C.byref(patch), C.byref(config), model, _p(q), _p(t), _p(X), _p(params),
                               _p(ref_desc), _p(r), _p(Jq), _p(Jt), _p(JX), _p(Jk))
    assert rc >= 0
    return r, Jq, Jt, JX, Jk


def ka_residual(p1, p2, config, kp1, kp2, jac=True):
    n = p1.C
    kp1, kp2 = (np.ascontiguousarray(a, dtype=np.float64) for a in (kp1, kp2))
    r = np.empty(n)
    J1, J2 = (np.empty((n, 2)), np.empty((n, 2))) if jac else (None, None)
    rc = lib().pxo_ka_residual(C.byref(p1), C.byref(p2), C.byref(config), _p(kp1), _p(kp2), _p(r), _p(J1), _p(J2))
    assert rc >= 0
    return r, J1, J2


def ref2d_residual(p, config, kp, ref_desc, jac=True):
    n = p.C
    kp = np.ascontiguousarray(kp, dtype=np.float64)
    ref_desc = np.ascontiguousarray(ref_desc, dtype=np.float64)
    r = np.empty(n)
    J = np.empty((n, 2)) if jac else None
    lib().pxo_ref2d_residual(C.byref(p), C.byref(config), _p(kp), _p(ref_desc), _p(r), _p(J))
    return r, J


def loss_eval(ls, s, weight=1.0):
    rho = np.empty(3)
    lib().pxo_loss_eval(C.byref(ls), C.c_double(weight), C.c_double(s), _p(rho))
    return rho


def corrector(s, rho, r, J=None):
    r = np.array(r, dtype=np.float64)
    rho = np.ascontiguousarray(rho, dtype=np.float64)
    n = 0
    if J is not None:
        J = np.array(J, dtype=np.float64, order="C")
        n = J.shape[1]
    lib().pxo_corrector(C.c_double(s), _p(rho), r.shape[0], n, _p(r), _p(J))
    return r, J


def robust_mean_irls(descs, ls, iters=100, l2_normalize=True):
    descs = np.ascontiguousarray(descs, dtype=np.float64)
    n, ch = descs.shape
    mean = np.empty(ch)
    early = lib().pxo_robust_mean_irls(_p(descs), n, ch, C.byref(ls), iters, int(l2_normalize), _p(mean))
    return mean, early


def compute_reference(descs, ls, iters=100, l2_normalize=True):
    descs = np.ascontiguousarray(descs, dtype=np.float64)
    n, ch = descs.shape
    ref_out, mean = np.empty(ch), np.empty(ch)
    idx = lib().pxo_compute_reference(_p(descs), n, ch, C.byref(ls), iters, int(l2_normalize), _p(ref_out), _p(mean))
    return idx, ref_out, mean


def ba_batch(problem):
    """problem: dict of numpy arrays (see tests/synth.py). Returns (BaBatch, keepalive)."""
    keep = {}

    def arr(name, dt):
        a = np.ascontiguousarray(problem[name], dtype=dt)
        keep[name] = a
        return a.ctypes.data

    arena = np.ascontiguousarray(problem["patches"])
    keep["patches"] = arena
    n_p, H, W, ch = arena.shape
    b = BaBatch(len(problem["obs_image"]), arr("obs_image", np.int32), arr("obs_point", np.int32),
                arr("obs_patch", np.int64), arr("image_camera", np.int32), arr("qvec", np.float64),
                arr("tvec", np.float64), arr("cam_model", np.int32), arr("cam_params", np.float64),
                arr("xyz", np.float64), arr("refs", np.float64) if problem.get("refs") is not None else None, arena.ctypes.data,
                _NP2DT[arena.dtype], H, W, ch, arr("corners", np.int32), arr("scales", np.float64),
                float(problem.get("upsampling", 1.0)))
    return b, keep


def ba_eval_batch(problem, config, ls, first=0, count=None, n_threads=1, want_r=False, want_J=False):
    b, keep = ba_batch(problem)
    n = b.n_obs if count is None else count
    ch = b.C
    r = np.empty((n, ch)) if want_r else None
    J = np.empty((n, ch, 10 + KPAD)) if want_J else None
    cost = lib().pxo_ba_eval_batch(C.byref(b), C.byref(config), C.byref(ls), first, n, n_threads, _p(r), _p(J))
    return cost, r, J


class LMOptions(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("function_tolerance", C.c_double),
                ("gradient_tolerance", C.c_double), ("parameter_tolerance", C.c_double),
                ("initial_radius", C.c_double), ("max_radius", C.c_double), ("min_radius", C.c_double),
                ("min_relative_decrease", C.c_double), ("min_lm_diagonal", C.c_double),
                ("max_lm_diagonal", C.c_double), ("max_consecutive_invalid_steps", C.c_int32),
                ("jacobi_scaling", C.c_int32), ("use_inner_iterations", C.c_int32),
                ("inner_iteration_tolerance", C.c_double)]


class LMSummary(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("num_successful", C.c_int32), ("termination", C.c_int32),
                ("num_unknowns", C.c_int32), ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("final_radius", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def lm_options(max_iterations=100, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0,
               initial_radius=1e4, max_radius=1e16, min_radius=1e-32, min_relative_decrease=1e-3,
               min_lm_diagonal=1e-6, max_lm_diagonal=1e32, max_consecutive_invalid_steps=10, jacobi_scaling=1,
               use_inner_iterations=0, inner_iteration_tolerance=1e-3):
    return LMOptions(max_iterations, function_tolerance, gradient_tolerance, parameter_tolerance,
                     initial_radius, max_radius, min_radius, min_relative_decrease, min_lm_diagonal,
                     max_lm_diagonal, max_consecutive_invalid_steps, jacobi_scaling, int(use_inner_iterations),
                     inner_iteration_tolerance)


def ba_solve(problem, config, ls, pose_const, tvec_const_mask, cam_const_mask, point_const, opts=None):
    """Runs the oracle LM; returns (summary dict, refined copies of qvec, tvec, cam_params, xyz)."""
    prob = dict(problem)
    for k in ("qvec", "tvec", "cam_params", "xyz"):
        prob[k] = np.array(problem[k], dtype=np.float64, order="C", copy=True)
    b, keep = ba_batch(prob)
    # ba_batch made contiguous copies only if needed; make sure we mutate the arrays we return
    for k in ("qvec", "tvec", "cam_params", "xyz"):
        assert keep[k] is prob[k] or keep[k].ctypes.data == prob[k].ctypes.data
    opts = opts or lm_options()
    s = LMSummary()
    pc = np.ascontiguousarray(pose_const, dtype=np.uint8)
    tm = np.ascontiguousarray(tvec_const_mask, dtype=np.uint8)
    cm = np.ascontiguousarray(cam_const_mask, dtype=np.uint16)
    ptc = np.ascontiguousarray(point_const, dtype=np.uint8)
    rc = lib().pxo_ba_solve(C.byref(b), len(prob["image_camera"]), len(prob["cam_model"]),
                            C.c_int64(len(prob["xyz"])), C.byref(config), C.byref(ls), _p(pc), _p(tm), _p(cm),
                            _p(ptc), C.byref(opts), C.byref(s))
    assert rc == 0
    return s.as_dict(), prob["qvec"], prob["tvec"], prob["cam_params"], prob["xyz"]


class LinearOptions(C.Structure):
    _fields_ = [("max_linear_solver_iterations", C.c_int32), ("eta", C.c_double), ("r_tolerance", C.c_double)]


CG_STOPS = ("max_iterations", "q", "r_tolerance", "rho", "indefinite", "preconditioner", "zero_rhs")


class LMTraceEntry(C.Structure):
    _fields_ = [("cg_iterations", C.c_int32), ("cg_stop", C.c_int32), ("step_is_valid", C.c_int32),
                ("step_is_successful", C.c_int32), ("relative_decrease", C.c_double), ("radius", C.c_double),
                ("margin_last", C.c_double), ("margin_prev", C.c_double), ("margin_min", C.c_double)]


class LMTrace(C.Structure):
    _fields_ = [("capacity", C.c_int32), ("count", C.c_int32), ("entries", C.POINTER(LMTraceEntry))]


def linear_options(max_linear_solver_iterations=200, eta=0.1, r_tolerance=-1.0):
    return LinearOptions(int(max_linear_solver_iterations), float(eta), float(r_tolerance))


def _gauge_arrays(pose_const, tvec_const_mask, cam_const_mask, point_const):
    return (np.ascontiguousarray(pose_const, dtype=np.uint8), np.ascontiguousarray(tvec_const_mask, dtype=np.uint8),
            np.ascontiguousarray(cam_const_mask, dtype=np.uint16), np.ascontiguousarray(point_const, dtype=np.uint8))


def ba_solve_iterative(problem, config, ls, pose_const, tvec_const_mask, cam_const_mask, point_const, opts=None, lin=None):
    """pxo_ba_solve_iterative: the oracle's LM loop with the iterative reduced step.  Returns (summary dict, trace, refined copies
    of qvec, tvec, cam_params, xyz); trace: one dict per LM iteration (cg_iterations, cg_stop as a name of CG_STOPS,
    step_is_valid, step_is_successful, relative_decrease, radius, margin_last, margin_prev, margin_min); the summary gains
    linear_iterations, their sum."""
    prob = dict(problem)
    for k in ("qvec", "tvec", "cam_params", "xyz"):
        prob[k] = np.array(problem[k], dtype=np.float64, order="C", copy=True)
    b, keep = ba_batch(prob)
    for k in ("qvec", "tvec", "cam_params", "xyz"):
        assert keep[k] is prob[k] or keep[k].ctypes.data == prob[k].ctypes.data
    opts = opts or lm_options()
    lin = lin or linear_options()
    s = LMSummary()
    cap = max(1, int(opts.max_iterations))
    entries = (LMTraceEntry * cap)()
    tr = LMTrace(cap, 0, C.cast(entries, C.POINTER(LMTraceEntry)))
    pc, tm, cm, ptc = _gauge_arrays(pose_const, tvec_const_mask, cam_const_mask, point_const)
    fn = lib().pxo_ba_solve_iterative
    fn.restype = C.c_int
    rc = fn(C.byref(b), len(prob["image_camera"]), len(prob["cam_model"]), C.c_int64(len(prob["xyz"])), C.byref(config),
            C.byref(ls), _p(pc), _p(tm), _p(cm), _p(ptc), C.byref(opts), C.byref(lin), C.byref(s), C.byref(tr))
    assert rc == 0 and tr.count <= cap
    trace = []
    for e in entries[:tr.count]:
        d = {k: getattr(e, k) for k, _ in LMTraceEntry._fields_}
        d["cg_stop"] = CG_STOPS[d["cg_stop"]]
        trace.append(d)
    out = s.as_dict()
    out["linear_iterations"] = sum(e["cg_iterations"] for e in trace)
    return out, trace, prob["qvec"], prob["tvec"], prob["cam_params"], prob["xyz"]


def ba_reduced_system(problem, config, ls, pose_const, tvec_const_mask, cam_const_mask, point_const, opts=None, lin=None):
    """pxo_ba_reduced_system: dict with S (n_c x n_c), rhs, M (the specified preconditioner blocks, damped, not inverted, zero
    outside them), x (the conjugate-gradient iterate `lin` stops at), col_group, cg_iterations -- of the first LM iteration
    (radius = opts.initial_radius) at the problem's parameters."""
    b, keep = ba_batch(problem)
    opts = opts or lm_options()
    lin = lin or linear_options()
    n_img, n_cam = len(problem["image_camera"]), len(problem["cam_model"])
    cap = 6 * n_img + KPAD * n_cam
    S, M = np.zeros(cap * cap), np.zeros(cap * cap)
    rhs, x = np.zeros(cap), np.zeros(cap)
    grp = np.zeros(cap, np.int32)
    its = C.c_int32(0)
    pc, tm, cm, ptc = _gauge_arrays(pose_const, tvec_const_mask, cam_const_mask, point_const)
    fn = lib().pxo_ba_reduced_system
    fn.restype = C.c_int
    n_c = fn(C.byref(b), n_img, n_cam, C.c_int64(len(problem["xyz"])), C.byref(config), C.byref(ls), _p(pc), _p(tm), _p(cm),
             _p(ptc), C.byref(opts), C.byref(lin), _p(S), _p(rhs), _p(M), _p(x), _p(grp), C.byref(its))
    assert n_c >= 0
    return dict(n_c=n_c, S=S[:n_c * n_c].reshape(n_c, n_c).copy(), rhs=rhs[:n_c].copy(), M=M[:n_c * n_c].reshape(n_c, n_c).copy(),
                x=x[:n_c].copy(), col_group=grp[:n_c].copy(), cg_iterations=its.value)


def ba_lm_iteration_schur(problem, config, ls, pose_const, tvec_const_mask, cam_const_mask, point_const, radius=1e4,
                          n_threads=0, want_step=True):
    """One Schur-complement LM iteration on the host cores (pxo_lm_bench.c).  Returns a dict with the stage times
    (ms), the costs, the size of the reduced system and -- want_step -- the tangent step (delta_c, delta_p)."""
    b, keep = ba_batch(problem)
    n_img, n_cam, n_pts = len(problem["image_camera"]), len(problem["cam_model"]), len(problem["xyz"])
    pc = np.ascontiguousarray(pose_const, dtype=np.uint8)
    tm = np.ascontiguousarray(tvec_const_mask, dtype=np.uint8)
    cm = np.ascontiguousarray(cam_const_mask, dtype=np.uint16)
    ptc = np.ascontiguousarray(point_const, dtype=np.uint8)
    n_c = C.c_int()
    times, cost = np.zeros(6), np.zeros(2)
    dc = np.zeros(n_img * 6 + n_cam * KPAD) if want_step else None
    dp = np.zeros((n_pts, 3)) if want_step else None
    fn = lib().pxo_ba_lm_iteration_schur
    fn.restype = C.c_int
    rc = fn(C.byref(b), n_img, n_cam, C.c_int64(n_pts), C.byref(config), C.byref(ls), _p(pc), _p(tm), _p(cm), _p(ptc),
            C.c_double(radius), C.c_double(1e-6), C.c_double(1e32), int(n_threads), C.byref(n_c), _p(dc), _p(dp),
            _p(times), _p(cost))
    names = ("jacobian_eval_ms", "schur_ms", "cholesky_ms", "backsub_ms", "cost_eval_ms", "total_ms")
    out = dict(zip(names, times.tolist()))
    out.update(rc=rc, n_c=n_c.value, cost=float(cost[0]), cost_check=float(cost[1]))
    if want_step:
        out["delta_c"], out["delta_p"] = dc[:n_c.value], dp
    return out


def nearest_reference(patch, config, kp, candidates):
    """FindNearestReferences for one correspondence (localization/src/nearest_references.h:36-49):
    index of the candidate descriptor with the smallest squared distance to the query descriptor
    (first minimum wins) and that distance."""
    q, _ = ref2d_residual(patch, config, kp, np.zeros(patch.C), jac=False)
    best, dmin = -1, np.finfo(np.float64).max
    for i, d in enumerate(candidates):
        e = np.asarray(d, dtype=np.float64).reshape(-1) - q
        s = float(e @ e)
        if s < dmin:
            best, dmin = i, s
    return best, dmin
