"""Fundamental-matrix estimation for the accelerated path.

Every other entry point of two-view verification needs cameras whose intrinsics can be trusted.  COLMAP's two-view estimation goes
the other way in two cases: a camera without a prior focal length (any photograph without EXIF) gets F and H only, and a camera
with one still gets F next to E, the pair being UNCALIBRATED when E explains noticeably fewer matches than F.  COLMAP is not
installable where this library runs, so the stage is native here: a batched, deterministic seven-point estimator with a local
optimisation over a rank-2 parametrisation on the GPU (pxr_fundamental; DESIGN.md section 23 -- NOT COLMAP's LO-RANSAC, and
parity with COLMAP is not pinned).

`fundamental_matrix_estimation` has pycolmap's shape; `two_view_config_uncalibrated` is the rule `TwoViewClassifier` applies when
its "fundamental" option is set.
"""
import inspect

import numpy as np

from ..engine import FundamentalProblem, fundamental_options
from . import two_view as _tv

_DEFAULTS = {name: p.default for name, p in inspect.signature(fundamental_options).parameters.items()}
_OPTION_KEYS = tuple(_DEFAULTS)
_NAMES = ("F", "status", "n_inliers", "n_trials", "inlier", "err")


def fundamental_engine_options(options=None):
    """The keyword arguments of engine.fundamental_options for an option dict (two_view._engine_options).  Unknown keys raise
    ValueError."""
    return _tv._engine_options(options, _OPTION_KEYS, "fundamental", fundamental_options)


def _estimate(ctx, batch, opts):
    """The seam to the GPU: host arrays {F, status, n_inliers, n_trials, inlier, err}."""
    return _tv._run(FundamentalProblem, _NAMES, ctx, batch, opts)


def two_view_config_uncalibrated(e_ok, n_e, f_ok, n_f, h_ok, n_h, n_r, both_trusted, max_H_inlier_ratio=0.8, min_E_F_inlier_ratio=0.95):
    """The class of a pair from what the three estimators report, the rules applied in this order:
    1. DEGENERATE if nothing succeeded.
    2. the epipolar model M is E when both cameras are trusted, E succeeded and (F failed or n_E >= min_E_F_inlier_ratio n_F);
       otherwise F if F succeeded; otherwise there is none.
    3. if H succeeded and (there is no M or n_H > max_H_inlier_ratio n_M): two_view_config's PANORAMIC (n_R > max_H_inlier_ratio
       n_H) / PLANAR when both cameras are trusted, PLANAR_OR_PANORAMIC when not -- the rotation-only count means nothing under a
       guessed focal length.
    4. otherwise CALIBRATED if M is E, UNCALIBRATED if M is F.
    (E succeeding under a camera that is not trusted, with F and H failing, leaves no model: DEGENERATE.)"""
    if not e_ok and not f_ok and not h_ok:
        return "DEGENERATE"
    model, n_m = None, 0
    if both_trusted and e_ok and (not f_ok or n_e >= min_E_F_inlier_ratio * n_f):
        model, n_m = "E", n_e
    elif f_ok:
        model, n_m = "F", n_f
    if h_ok and (model is None or n_h > max_H_inlier_ratio * n_m):
        if not both_trusted:
            return "PLANAR_OR_PANORAMIC"
        return "PANORAMIC" if n_r > max_H_inlier_ratio * n_h else "PLANAR"
    if model is None:
        return "DEGENERATE"
    return "CALIBRATED" if model == "E" else "UNCALIBRATED"


# the estimator whose inliers a pair of each class returns: the model that decided the class (DEGENERATE: none)
DECIDING_MODEL = {"CALIBRATED": "E", "UNCALIBRATED": "F", "PLANAR": "H", "PANORAMIC": "H", "PLANAR_OR_PANORAMIC": "H", "DEGENERATE": None}


def conditioning_camera(points):
    """The SIMPLE_PINHOLE camera that conditions a set of points (n, 2) for the seven-point system: centre = the centroid of the
    finite points, f = their mean distance from it / sqrt 2 (so that the normalised points sit at a mean distance of sqrt 2:
    Hartley's normalisation, done once on the host).  No finite point, or all in one spot: the identity."""
    from .reconstruction import Camera
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    pts = pts[np.isfinite(pts).all(1)]
    c, f = np.zeros(2), 1.0
    if len(pts):
        c = pts.mean(0)
        d = float(np.sqrt(((pts - c) ** 2).sum(1)).mean()) / np.sqrt(2.0)
        if d > 0.0 and np.isfinite(d):
            f = d
    return Camera(0, 0, 1, 1, [f, float(c[0]), float(c[1])])


def fundamental_in_pixels(F, camera1, camera2):
    """F_px = K2^-t F K1^-1 of two pinhole-family cameras, scaled to unit Frobenius norm: x2_px^t F_px x1_px = 0."""
    K1, K2 = _tv._calibration_matrix(camera1), _tv._calibration_matrix(camera2)
    Fp = np.linalg.inv(K2).T @ np.asarray(F, dtype=np.float64).reshape(3, 3) @ np.linalg.inv(K1)
    return Fp / np.linalg.norm(Fp)


def fundamental_matrix_estimation(points1, points2, options=None, camera1=None, camera2=None, ctx=None):
    """pycolmap.fundamental_matrix_estimation's shape: {"success", "F" (3, 3), "num_inliers", "inliers"}, or {"success": False}.
    points: (n, 2).  Without cameras each side is conditioned on the host (conditioning_camera), max_error is in the points' units,
    and "F" is returned in those units: x2^t F x1 = 0 for the points as given, unit Frobenius norm.  With two cameras the points
    are pixels (COLMAP convention), "F" relates the normalised planes of the cameras (unit Frobenius norm), and for two
    pinhole-family cameras (SIMPLE_PINHOLE, PINHOLE) "F_pixels" = K2^-t F K1^-1 (unit norm) is returned too."""
    opts = fundamental_engine_options(options)
    xy1, xy2 = _tv._points(points1, points2)
    if (camera1 is None) != (camera2 is None):
        raise ValueError("camera1 and camera2 go together")
    cams = [conditioning_camera(xy1), conditioning_camera(xy2)] if camera1 is None else [camera1, camera2]
    res = _estimate(ctx, _tv._single_pair_batch(xy1, xy2, cams), opts)
    if res["status"][0] != 0:
        return {"success": False}
    F = res["F"][0].reshape(3, 3).copy()
    out = {"success": True, "F": F, "num_inliers": int(res["n_inliers"][0]), "inliers": [bool(x) for x in res["inlier"]]}
    if camera1 is None:
        out["F"] = fundamental_in_pixels(F, cams[0], cams[1])
    elif camera1.model_id in (0, 1) and camera2.model_id in (0, 1):
        out["F_pixels"] = fundamental_in_pixels(F, camera1, camera2)
    return out
