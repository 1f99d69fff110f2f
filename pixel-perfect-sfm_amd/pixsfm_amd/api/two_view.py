"""Two-view geometry for the accelerated path: the matches of image pairs -> one relative pose and one inlier mask per pair.

The reference hands geometric verification to COLMAP (`pycolmap.verify_matches` in examples/refine_sift_aachen.py:51, and the
same step inside hloc's reconstruction and triangulation, which refine_hloc drives); COLMAP is not installable where this
library runs, so the stage is native here, for calibrated cameras: a batched, deterministic five-point estimator with local
optimisation on the GPU (pxr_two_view_geometry; DESIGN.md section 21 -- NOT COLMAP's LO-RANSAC, parity with it is not pinned).

`TwoViewVerifier.create(conf).verify_pairs(keypoints, cameras, pairs, matches, scores)` filters the two lists that
`DescriptorMatcher.match_pairs` (or read_matches_hloc) returns, so
`build_matching_graph(pairs, *verifier.verify_pairs(keypoints, cameras, pairs, matches, scores)[:2])` is the whole step.  With
`poses` it verifies against known poses, as hloc's triangulation does.  `essential_matrix_estimation` has pycolmap's shape.
"""
import inspect

import numpy as np

from ..engine import TwoViewProblem, two_view_options
from .keypoint_adjustment import default_context

# COLMAP's RANSACOptions / TwoViewGeometryOptions names and the estimator's own, with their defaults: those of engine.two_view_options
_DEFAULTS = {name: p.default for name, p in inspect.signature(two_view_options).parameters.items()}
_OPTION_KEYS = tuple(_DEFAULTS)
_NAMES = ("qvec", "tvec", "E", "status", "n_inliers", "n_trials", "inlier", "err")


def _engine_options(options, keys, what, builder):
    """The keyword arguments of an engine option builder for an option dict (a nested "ransac" dict, as pycolmap groups them, is
    flattened).  A key outside `keys` raises ValueError, which names the estimator as `what`."""
    opts = dict(options or {})
    ransac = opts.pop("ransac", None) or {}
    out = {}
    for k, v in list(dict(ransac).items()) + list(opts.items()):
        if k not in keys:
            raise ValueError("unknown %s option %r (known: %s)" % (what, k, ", ".join(keys)))
        out[k] = v
    builder(**out)                            # fail early on a value ctypes cannot take
    return out


def two_view_engine_options(options=None):
    """The keyword arguments of engine.two_view_options for an option dict (_engine_options).  Unknown keys raise ValueError."""
    return _engine_options(options, _OPTION_KEYS, "two-view", two_view_options)


class _Batch(dict):
    """A host pair batch that remembers the pair problem that uploaded it, so that the estimators run after the first share
    its device arrays (a pose prior is uploaded only by that first one)."""
    problem = None


def _run(problem_cls, names, ctx, batch, opts):
    """Construct a pair problem over `batch` -- over the upload a _Batch remembers, when it does -- run it and download its
    outputs: host arrays by name.  Nothing else in the two-view api modules touches the GPU."""
    ctx = ctx or default_context()
    prob = problem_cls(ctx, getattr(batch, "problem", None) or batch)
    if isinstance(batch, _Batch):
        batch.problem = prob
    return {k: a.download() for k, a in zip(names, prob.estimate(**opts))}


def _estimate(ctx, batch, opts):
    """The seam to the GPU: host arrays {qvec, tvec, E, status, n_inliers, n_trials, inlier, err}."""
    return _run(TwoViewProblem, _NAMES, ctx, batch, opts)


def _camera_table(cameras):
    """Distinct camera objects -> (index of every camera in the list, cam_model, cam_params)."""
    table, index, seen = [], [], {}
    for c in cameras:
        k = seen.get(id(c))
        if k is None:
            k = seen[id(c)] = len(table)
            table.append(c)
        index.append(k)
    params = np.zeros((len(table), 12))
    for i, c in enumerate(table):
        params[i, :len(c.params)] = c.params
    return np.array(index, np.int32), np.array([c.model_id for c in table], np.int32), params


def _calibration_matrix(camera):
    """K of a SIMPLE_PINHOLE or PINHOLE camera."""
    k = camera.params
    if camera.model_id == 0:
        return np.array([[k[0], 0.0, k[1]], [0.0, k[0], k[2]], [0.0, 0.0, 1.0]])
    return np.array([[k[0], 0.0, k[2]], [0.0, k[1], k[3]], [0.0, 0.0, 1.0]])


def _points(points1, points2):
    """The two point lists of one pair as (n, 2) float64 arrays of one length."""
    xy1, xy2 = np.asarray(points1, dtype=np.float64).reshape(-1, 2), np.asarray(points2, dtype=np.float64).reshape(-1, 2)
    if len(xy1) != len(xy2):
        raise ValueError("points1 and points2 must have the same length")
    return xy1, xy2


def _single_pair_batch(xy1, xy2, cameras):
    """The batch of one pair: its matches (n, 2) + (n, 2) under the two cameras."""
    index, model, params = _camera_table(cameras)
    return dict(pair_offsets=np.array([0, len(xy1)], np.int64), xy1=xy1, xy2=xy2, pair_camera=index.reshape(1, 2), cam_model=model,
                cam_params=params)


def _multi_pair_batch(pairs, matches, keypoints, cameras, required, missing):
    """The batch of a list of pairs from per-image keypoints and cameras and per-pair matches.  Every image of a pair must be
    a key of each of the dicts `required`, or KeyError(`missing` % name)."""
    xy1, xy2, cams = [], [], []
    for (a, b), m in zip(pairs, matches):
        for n in (a, b):
            if any(n not in table for table in required):
                raise KeyError(missing % (n,))
        m = np.asarray(m).reshape(-1, 2).astype(np.int64)
        xy1.append(np.asarray(keypoints[a], dtype=np.float64)[m[:, 0], :2])
        xy2.append(np.asarray(keypoints[b], dtype=np.float64)[m[:, 1], :2])
        cams += [cameras[a], cameras[b]]
    index, model, params = _camera_table(cams)
    off = np.concatenate([[0], np.cumsum([len(a) for a in xy1])]).astype(np.int64)
    return _Batch(pair_offsets=off, xy1=np.concatenate(xy1).reshape(-1, 2), xy2=np.concatenate(xy2).reshape(-1, 2),
                  pair_camera=index.reshape(-1, 2), cam_model=model, cam_params=params)


def _masked(matches, scores, keep):
    """The matches (M, 2) and the scores ((M,), or None) of one pair that the mask `keep` selects."""
    return np.asarray(matches).reshape(-1, 2)[keep], None if scores is None else np.asarray(scores).reshape(-1)[keep]


def _relative_pose(pose1, pose2):
    """The pose of camera 2 relative to camera 1 from two world-to-camera poses (qvec, tvec): R = R2 R1^t, t = t2 - R t1."""
    from ..synthetic import qvec_to_rotmat, rotmat_to_qvec
    (q1, t1), (q2, t2) = pose1, pose2
    R = qvec_to_rotmat(np.asarray(q2, dtype=np.float64)) @ qvec_to_rotmat(np.asarray(q1, dtype=np.float64)).T
    return rotmat_to_qvec(R), np.asarray(t2, dtype=np.float64) - R @ np.asarray(t1, dtype=np.float64)


def _geometry(res, p, lo, hi):
    if res["status"][p] != 0:
        return {"success": False}
    return {"success": True, "E": res["E"][p].reshape(3, 3).copy(), "qvec": res["qvec"][p].copy(), "tvec": res["tvec"][p].copy(),
            "num_inliers": int(res["n_inliers"][p]), "inliers": [bool(x) for x in res["inlier"][lo:hi]]}


def essential_matrix_estimation(points1, points2, camera1, camera2, options=None, ctx=None):
    """pycolmap.essential_matrix_estimation's shape: {"success", "E" (3, 3), "qvec", "tvec", "num_inliers", "inliers"}, or
    {"success": False}.  points: (n, 2) pixels (COLMAP convention); the pose is that of camera 2 relative to camera 1, |t| = 1."""
    opts = two_view_engine_options(options)
    xy1, xy2 = _points(points1, points2)
    return _geometry(_estimate(ctx, _single_pair_batch(xy1, xy2, [camera1, camera2]), opts), 0, 0, len(xy1))


class TwoViewVerifier:
    """Geometric verification of the matches of image pairs -- in place of pycolmap.verify_matches."""
    default_conf = dict(_DEFAULTS)

    def __init__(self, conf=None, ctx=None):
        self.conf = {**self.default_conf, **two_view_engine_options(conf)}
        self.ctx = ctx

    @classmethod
    def create(cls, conf=None, ctx=None):
        """conf: a dict over default_conf; unknown keys raise ValueError."""
        return cls(conf, ctx)

    def verify_pairs(self, keypoints, cameras, pairs, matches, scores=None, poses=None):
        """keypoints {image name: (n, >= 2) pixels}, cameras {image name: camera}, pairs [(name1, name2)], matches: per pair an
        (M, 2) array of (keypoint of name1, keypoint of name2), scores: per pair an (M,) array or None.  All pairs are verified
        in one launch.  poses {image name: (qvec, tvec)} (world to camera): no pose is estimated, the matches of a pair are
        classified under the relative pose of its two images.
        Returns (matches, scores, geometries): the inlier matches and their scores per pair, in the shape build_matching_graph
        takes (scores is None if none were given), and per pair the dict essential_matrix_estimation returns.  A pair that
        fails keeps no match."""
        pairs, matches = list(pairs), list(matches)
        if len(pairs) != len(matches) or (scores is not None and len(scores) != len(pairs)):
            raise ValueError("pairs, matches and scores must have the same length")
        if not pairs:
            return [], (None if scores is None else []), []
        required = (keypoints, cameras) if poses is None else (keypoints, cameras, poses)
        batch = _multi_pair_batch(pairs, matches, keypoints, cameras, required, "no keypoints, camera or pose for image %r")
        off = batch["pair_offsets"]
        if poses is not None:
            rel = [_relative_pose(poses[a], poses[b]) for a, b in pairs]
            batch["prior_qvec"] = np.array([r[0] for r in rel]).reshape(-1, 4)
            batch["prior_tvec"] = np.array([r[1] for r in rel]).reshape(-1, 3)
        res = _estimate(self.ctx, batch, self.conf)
        out_m, out_s, geoms = [], [], []
        for p, m in enumerate(matches):
            kept = _masked(m, None if scores is None else scores[p], res["inlier"][off[p]:off[p + 1]].astype(bool))
            out_m.append(kept[0])
            out_s.append(kept[1])
            geoms.append(_geometry(res, p, off[p], off[p + 1]))
        return out_m, (out_s if scores is not None else None), geoms
