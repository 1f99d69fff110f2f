"""Homography estimation and two-view configurations for the accelerated path.

An essential matrix fits a pair taken by a rotating camera, or a pair that shows one plane, with a translation direction that
means nothing, and nothing `TwoViewVerifier` returns says so.  pycolmap.verify_matches, which that class stands in for,
classifies such pairs from the ratio of homography inliers to essential-matrix inliers; COLMAP is not installable where this
library runs, so the stage is native here, for calibrated cameras: a batched, deterministic four-point estimator with local
optimisation and a rotation-only model on the GPU (pxr_homography; DESIGN.md section 22 -- NOT COLMAP's LO-RANSAC, and the
classes are decided by this library's own rules: parity with COLMAP is not pinned).  Fundamental-matrix estimation lives in
api/fundamental.py; `TwoViewClassifier` runs it only when its "fundamental" option is set.

`TwoViewClassifier.create(conf).classify_pairs(keypoints, cameras, pairs, matches, scores)` has the shape of
`TwoViewVerifier.verify_pairs`; `homography_matrix_estimation` has pycolmap's shape.
"""
import inspect

import numpy as np

from ..engine import HomographyProblem, homography_options
from . import fundamental as _fm
from . import two_view as _tv

_DEFAULTS = {name: p.default for name, p in inspect.signature(homography_options).parameters.items()}
_OPTION_KEYS = tuple(_DEFAULTS)
_NAMES = ("H", "rot_qvec", "status", "n_inliers", "n_rot_inliers", "n_trials", "inlier", "err")
CONFIGS = ("CALIBRATED", "PLANAR", "PANORAMIC", "DEGENERATE", "UNCALIBRATED", "PLANAR_OR_PANORAMIC")


def homography_engine_options(options=None):
    """The keyword arguments of engine.homography_options for an option dict (two_view._engine_options).  Unknown keys raise
    ValueError."""
    return _tv._engine_options(options, _OPTION_KEYS, "homography", homography_options)


def _estimate(ctx, batch, opts):
    """The seam to the GPU: host arrays {H, rot_qvec, status, n_inliers, n_rot_inliers, n_trials, inlier, err}."""
    return _tv._run(HomographyProblem, _NAMES, ctx, batch, opts)


def two_view_config(e_success, n_e, h_success, n_h, n_r, max_H_inlier_ratio=0.8):
    """The class of a pair from what the two estimators report, the rules applied in this order:
    DEGENERATE  neither model succeeded
    CALIBRATED  E succeeded and n_H / n_E <= max_H_inlier_ratio
    PANORAMIC   n_H / n_E above it, or only H succeeded -- and n_R / n_H > max_H_inlier_ratio
    PLANAR      the same, without the second condition."""
    if not e_success and not h_success:
        return "DEGENERATE"
    if e_success and (not h_success or n_h <= max_H_inlier_ratio * n_e):
        return "CALIBRATED"
    return "PANORAMIC" if n_r > max_H_inlier_ratio * n_h else "PLANAR"


two_view_config_uncalibrated = _fm.two_view_config_uncalibrated


def _identity_camera():
    from .reconstruction import Camera
    return Camera(0, 0, 1, 1, [1.0, 0.0, 0.0])


def homography_matrix_estimation(points1, points2, options=None, camera1=None, camera2=None, ctx=None):
    """pycolmap.homography_matrix_estimation's shape: {"success", "H" (3, 3), "num_inliers", "inliers"}, or {"success": False}.
    points: (n, 2).  Without cameras the points are used as they are (the stand-in is an identity SIMPLE_PINHOLE camera), so
    max_error is in the points' units and x2 ~ H x1 in those units.  With two cameras the points are pixels (COLMAP convention),
    H maps the normalised plane of camera 1 to that of camera 2 (unit Frobenius norm), and for two pinhole-family cameras
    (SIMPLE_PINHOLE, PINHOLE) "H_pixels" = K2 H K1^-1 is returned too."""
    opts = homography_engine_options(options)
    xy1, xy2 = _tv._points(points1, points2)
    if (camera1 is None) != (camera2 is None):
        raise ValueError("camera1 and camera2 go together")
    cams = [_identity_camera()] * 2 if camera1 is None else [camera1, camera2]
    res = _estimate(ctx, _tv._single_pair_batch(xy1, xy2, cams), opts)
    if res["status"][0] != 0:
        return {"success": False}
    H = res["H"][0].reshape(3, 3).copy()
    out = {"success": True, "H": H, "num_inliers": int(res["n_inliers"][0]), "inliers": [bool(x) for x in res["inlier"]]}
    if camera1 is not None and camera1.model_id in (0, 1) and camera2.model_id in (0, 1):
        out["H_pixels"] = _tv._calibration_matrix(camera2) @ H @ np.linalg.inv(_tv._calibration_matrix(camera1))
    return out


class TwoViewClassifier:
    """Geometric verification with a verdict on the configuration: the essential-matrix estimator of TwoViewVerifier and the
    homography estimator on the same batch, and per pair one of CONFIGS.  Opt-in: with "fundamental" set to a dict of
    fundamental-matrix options (possibly empty) the fundamental-matrix estimator runs on the same upload and the class comes from
    two_view_config_uncalibrated, which knows UNCALIBRATED and PLANAR_OR_PANORAMIC too; min_E_F_inlier_ratio is COLMAP's value as
    remembered (parity unpinned).  With "fundamental" left at None nothing else is launched and nothing returned changes."""
    default_conf = {"two_view": dict(_tv._DEFAULTS), "homography": dict(_DEFAULTS), "max_H_inlier_ratio": 0.8,
                    "keep": ("CALIBRATED", "PLANAR", "PANORAMIC"), "fundamental": None, "min_E_F_inlier_ratio": 0.95}

    def __init__(self, conf=None, ctx=None):
        conf = dict(conf or {})
        for k in conf:
            if k not in self.default_conf:
                raise ValueError("unknown classifier option %r (known: %s)" % (k, ", ".join(self.default_conf)))
        # (with "fundamental" set, the two classes only that path can name are kept too unless "keep" says otherwise)
        more = () if conf.get("fundamental") is None else ("UNCALIBRATED", "PLANAR_OR_PANORAMIC")
        keep = tuple(conf.get("keep", self.default_conf["keep"] + more))
        for c in keep:
            if c not in CONFIGS:
                raise ValueError("unknown configuration %r in keep (known: %s)" % (c, ", ".join(CONFIGS)))
        self.conf = {"two_view": {**_tv._DEFAULTS, **_tv.two_view_engine_options(conf.get("two_view"))},
                     "homography": {**_DEFAULTS, **homography_engine_options(conf.get("homography"))},
                     "max_H_inlier_ratio": float(conf.get("max_H_inlier_ratio", self.default_conf["max_H_inlier_ratio"])), "keep": keep,
                     "fundamental": None if conf.get("fundamental") is None else
                     {**_fm._DEFAULTS, **_fm.fundamental_engine_options(conf["fundamental"])},
                     "min_E_F_inlier_ratio": float(conf.get("min_E_F_inlier_ratio", self.default_conf["min_E_F_inlier_ratio"]))}
        self.ctx = ctx

    @classmethod
    def create(cls, conf=None, ctx=None):
        """conf: a dict over default_conf; unknown keys, at either level, raise ValueError."""
        return cls(conf, ctx)

    def classify_pairs(self, keypoints, cameras, pairs, matches, scores=None, prior_focal_length=None):
        """The arguments of TwoViewVerifier.verify_pairs (without poses).  All pairs go through both estimators in one launch each.
        Returns (matches, scores, geometries): per pair the dict TwoViewVerifier returns for the essential matrix ("success" is
        the essential matrix's) plus "config", "H" ((3, 3), normalised plane, or None), "num_inliers_H" and "num_inliers_R";
        the matches and scores are the inliers of the model with more inliers (the essential matrix on a tie), and none for a
        pair whose class is not in conf["keep"].
        With conf["fundamental"] set: a third launch for the fundamental matrix; prior_focal_length (a dict image name -> bool,
        a missing name means trusted) says whose focal length can be trusted -- the camera of an image that cannot is only a
        conditioning transform; the geometries gain "F" ((3, 3), normalised planes of the cameras given, or None) and
        "num_inliers_F", the class is two_view_config_uncalibrated's, and the matches and scores are the inliers of the model
        that decided it."""
        pairs, matches = list(pairs), list(matches)
        if len(pairs) != len(matches) or (scores is not None and len(scores) != len(pairs)):
            raise ValueError("pairs, matches and scores must have the same length")
        if not pairs:
            return [], (None if scores is None else []), []
        # one batch for the two or three seams: the first uploads it, the others share its device arrays
        batch = _tv._multi_pair_batch(pairs, matches, keypoints, cameras, (keypoints, cameras), "no keypoints or camera for image %r")
        off = batch["pair_offsets"]
        res_e = _tv._estimate(self.ctx, batch, self.conf["two_view"])
        res_h = _estimate(self.ctx, batch, self.conf["homography"])
        with_f = self.conf["fundamental"] is not None
        if with_f:
            res_f = _fm._estimate(self.ctx, batch, self.conf["fundamental"])
            trusted = dict(prior_focal_length or {})
        out_m, out_s, geoms = [], [], []
        for p, m in enumerate(matches):
            e_ok, h_ok = bool(res_e["status"][p] == 0), bool(res_h["status"][p] == 0)
            n_e, n_h, n_r = int(res_e["n_inliers"][p]), int(res_h["n_inliers"][p]), int(res_h["n_rot_inliers"][p])
            g = _tv._geometry(res_e, p, off[p], off[p + 1])
            g.update(config=two_view_config(e_ok, n_e, h_ok, n_h, n_r, self.conf["max_H_inlier_ratio"]),
                     H=res_h["H"][p].reshape(3, 3).copy() if h_ok else None, num_inliers_H=n_h, num_inliers_R=n_r)
            keep = (res_h if n_h > n_e else res_e)["inlier"][off[p]:off[p + 1]].astype(bool)
            if with_f:
                f_ok, n_f = bool(res_f["status"][p] == 0), int(res_f["n_inliers"][p])
                both = bool(trusted.get(pairs[p][0], True)) and bool(trusted.get(pairs[p][1], True))
                g.update(config=two_view_config_uncalibrated(e_ok, n_e, f_ok, n_f, h_ok, n_h, n_r, both, self.conf["max_H_inlier_ratio"],
                                                             self.conf["min_E_F_inlier_ratio"]),
                         F=res_f["F"][p].reshape(3, 3).copy() if f_ok else None, num_inliers_F=n_f)
                which = {"E": res_e, "F": res_f, "H": res_h}.get(_fm.DECIDING_MODEL[g["config"]])
                keep = which["inlier"][off[p]:off[p + 1]].astype(bool) if which else np.zeros(len(keep), bool)
            if g["config"] not in self.conf["keep"]:
                keep = np.zeros(len(keep), bool)
            kept = _tv._masked(m, None if scores is None else scores[p], keep)
            out_m.append(kept[0])
            out_s.append(kept[1])
            geoms.append(g)
        return out_m, (out_s if scores is not None else None), geoms
