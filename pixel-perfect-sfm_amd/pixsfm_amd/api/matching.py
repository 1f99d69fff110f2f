"""Descriptor matching for the accelerated path: descriptors of image pairs -> mutual nearest neighbours.

The reference takes its matches from hloc (`hloc.match_features.main` with the confs "NN-mutual", "NN-ratio" or
"NN-superpoint", read back by pixsfm/util/hloc.py:read_matches_hloc); hloc is not installable where this library runs, so the
stage is native here.  `DescriptorMatcher.create(conf).match_pairs(descriptors, pairs)` returns exactly the two lists
read_matches_hloc returns, so `build_matching_graph(pairs, *matcher.match_pairs(descriptors, pairs))` is the whole step, and
`pairs_2d3d_from_matches` turns the matches of a query against database images into what `QueryLocalizer.localize` takes.
The kernels (pxr_match_descriptors) reproduce bit for bit; parity with hloc is not pinned.
`match_pairs_guided` matches pairs again under the two-view models that verification found (COLMAP's guided matching;
pxr_match_guided): only candidates that agree with the model compete, which is what repeated structure needs.
"""
import numpy as np

from .._lib import GUIDE_EPIPOLAR, GUIDE_HOMOGRAPHY
from ..engine import MATCH_CONFS, MatchProblem, image_to_world
from . import base
from .fundamental import DECIDING_MODEL
from .keypoint_adjustment import default_context
from .two_view import _camera_table


class DescriptorMatcher:
    """Mutual-nearest-neighbour matching of image pairs -- in place of hloc.match_features.main + read_matches_hloc."""
    default_conf = {
        'ratio_threshold': None,       # Lowe's ratio (on distances, as hloc states it); None or 0: off
        'distance_threshold': None,    # largest descriptor distance of a match; None or 0: off
        'do_mutual_check': True,
        'max_batch_rows': 1 << 26,     # rows of the flat outputs of one launch; more pairs than that are split into several launches
    }

    def __init__(self, conf=None, ctx=None):
        if isinstance(conf, str):
            if conf not in MATCH_CONFS:
                raise ValueError("unknown matcher conf %r (known: %s)" % (conf, ", ".join(sorted(MATCH_CONFS))))
            conf = dict(MATCH_CONFS[conf])
        self.conf = base.merge_conf(self.default_conf, conf)
        if int(self.conf['max_batch_rows']) < 1:
            raise ValueError("max_batch_rows must be positive")
        self.ctx = ctx
        self.num_launches = 0

    @classmethod
    def create(cls, conf=None, ctx=None):
        """conf: "NN-mutual", "NN-ratio", "NN-superpoint", or a dict over default_conf."""
        return cls(conf, ctx)

    def options(self):
        return {k: self.conf[k] for k in ('ratio_threshold', 'distance_threshold', 'do_mutual_check')}

    # -- the one place that touches the GPU ---------------------------------------------------------------------------------------
    def _run(self, descriptors, pair_indices, guide=None):
        """descriptors: list of (n, D) float32 arrays; pair_indices: (P, 2) ints into it.  Returns per pair (matches0 (n_a,) int32,
        scores0 (n_a,) float32).  One launch covers all pairs and every image is uploaded once; when the flat outputs (the sum of
        the first images' sizes) would exceed conf max_batch_rows, the pairs are split into consecutive groups below that bound,
        one launch each (a single pair larger than the bound is a launch of its own).
        guide: (keypoints per image (n, 2) in the models' frame, per pair a kind, a (3, 3) model, a threshold) -- the gate of
        pxr_match_guided."""
        ctx = self.ctx or default_context()
        pair_indices = np.asarray(pair_indices, dtype=np.int64).reshape(-1, 2)
        out = [None] * len(pair_indices)
        if len(pair_indices) == 0:
            return out
        sizes = np.array([len(d) for d in descriptors], dtype=np.int64)
        if guide is not None:
            kinds, thresholds = np.asarray(guide[1], np.int32), np.asarray(guide[3], np.float64)
            models = np.asarray(guide[2], np.float64).reshape(-1, 9)
        problem = MatchProblem(ctx, descriptors, pair_indices, keypoints=None if guide is None else guide[0])   # uploads every image once
        groups, first, rows = [], 0, 0
        for p, (ia, _) in enumerate(pair_indices):
            if p > first and rows + sizes[ia] > int(self.conf['max_batch_rows']):
                groups.append((first, p))
                first, rows = p, 0
            rows += sizes[ia]
        groups.append((first, len(pair_indices)))
        for lo, hi in groups:
            sub = problem if len(groups) == 1 else MatchProblem(ctx, problem.d_desc, pair_indices[lo:hi], image_offsets=problem.image_offsets,
                                                                keypoints=problem.d_xy)
            if guide is None:
                d_m, d_s, _ = sub.run(**self.options())
            else:
                d_m, d_s, _ = sub.run_guided(kinds[lo:hi], models[lo:hi], thresholds[lo:hi], **self.options())
            self.num_launches += 1
            m, s, off = d_m.download(), d_s.download(), sub.pair_offsets
            for p in range(lo, hi):
                out[p] = (m[off[p - lo]:off[p - lo + 1]], s[off[p - lo]:off[p - lo + 1]])
        return out

    def _indexed(self, descriptors, pairs):
        names = []
        for pair in pairs:
            for n in pair:
                if n not in descriptors:
                    raise KeyError("no descriptors for image %r" % (n,))
                if n not in names:
                    names.append(n)
        index = {n: k for k, n in enumerate(names)}
        arrays = [np.ascontiguousarray(descriptors[n], dtype=np.float32) for n in names]
        for n, a in zip(names, arrays):
            if a.ndim != 2:
                raise ValueError("descriptors of %r must be (n, D), not %s (hloc stores (D, n): transpose)" % (n, a.shape))
        return arrays, np.array([(index[a], index[b]) for a, b in pairs], dtype=np.int64).reshape(-1, 2)

    def match_raw(self, descriptors, pairs):
        """hloc's per-pair datasets: [{"matches0": (n_1,) int32 with -1 for no match, "matching_scores0": (n_1,) float32}]."""
        pairs = list(pairs)
        arrays, idx = self._indexed(descriptors, pairs)
        return [{"matches0": m, "matching_scores0": s} for m, s in self._run(arrays, idx)]

    def match_pairs(self, descriptors, pairs):
        """descriptors {image name: (n, D) float32, L2-normalised}, pairs [(name1, name2)] -> (matches, scores): per pair an (M, 2)
        uint64 array of (keypoint of name1, keypoint of name2) and an (M,) float32 array, what read_matches_hloc returns.  One
        launch for all pairs, every image uploaded once; split into several launches past conf max_batch_rows (see _run)."""
        return _kept(self.match_raw(descriptors, pairs))

    # -- guided matching: only candidates that agree with the pair's two-view model compete (pxr_match_guided)
    def match_raw_guided(self, descriptors, keypoints, cameras, pairs, geometries, max_error=4.0):
        """match_raw under the pairs' two-view models: hloc's per-pair datasets, where only candidates that agree with the model of
        the pair competed.  See match_pairs_guided; a pair without a usable model has all matches0 = -1 and is not launched."""
        pairs, geometries = list(pairs), list(geometries)
        if len(pairs) != len(geometries):
            raise ValueError("pairs and geometries must have the same length")
        if not (max_error >= 0.0):
            raise ValueError("max_error must not be negative")
        for pair in pairs:
            for n in pair:
                if n not in descriptors:
                    raise KeyError("no descriptors for image %r" % (n,))
        picked = [guided_model(g) for g in geometries]
        live = [p for p, k in enumerate(picked) if k is not None]
        out = [{"matches0": np.full(len(descriptors[a]), -1, np.int32), "matching_scores0": np.zeros(len(descriptors[a]), np.float32)}
               for a, _ in pairs]
        if not live:
            return out
        # only the images of the pairs with a model are read, normalised and uploaded
        arrays, idx = self._indexed(descriptors, [pairs[p] for p in live])
        names = [None] * len(arrays)
        for p, (ia, ib) in zip(live, idx):
            names[ia], names[ib] = pairs[p]
        xy = []
        for n, a in zip(names, arrays):
            if n not in keypoints or n not in cameras:
                raise KeyError("no keypoints or camera for image %r" % (n,))
            k = np.asarray(keypoints[n], dtype=np.float64)
            k = k.reshape(0, 2) if k.size == 0 else k
            if k.ndim != 2 or k.shape[1] < 2 or len(k) != len(a):
                raise ValueError("keypoints of %r must be (%d, >= 2), one row per descriptor, not %s" % (n, len(a), k.shape))
            xy.append(k[:, :2])
        ctx = self.ctx or default_context()
        index, cam_model, cam_params = _camera_table([cameras[n] for n in names])
        uv = [image_to_world(ctx, cam_model, cam_params, k, np.full(len(k), c, np.int32))[0] for k, c in zip(xy, index)]   # once per image
        thr = [guided_threshold(picked[p][0], cameras[pairs[p][0]], cameras[pairs[p][1]], max_error) for p in live]
        res = self._run(arrays, idx, guide=(uv, [GUIDE_KINDS[picked[p][0]] for p in live], [picked[p][1] for p in live], thr))
        for p, (m, s) in zip(live, res):
            out[p] = {"matches0": m, "matching_scores0": s}
        return out

    def match_pairs_guided(self, descriptors, keypoints, cameras, pairs, geometries, max_error=4.0):
        """match_pairs under the pairs' two-view models (COLMAP's guided matching): descriptors, pairs as in match_pairs; keypoints
        {image name: (n, >= 2) pixels} and cameras {image name: camera} as TwoViewVerifier.verify_pairs takes them; geometries: per
        pair what verify_pairs / classify_pairs returned.  Every image is normalised once (engine.image_to_world); the model is
        guided_model(geometry) and the threshold guided_threshold's, the estimators' own for max_error pixels.  A keypoint that
        cannot be undistorted matches nothing.  Returns (matches, scores) in match_pairs' shape; a pair without a usable model
        ("success" False, DEGENERATE, a model that is None) comes back empty and is not launched: images that only such pairs name
        are neither normalised nor uploaded and need no keypoints or camera.  An image without features is fine on either side."""
        return _kept(self.match_raw_guided(descriptors, keypoints, cameras, pairs, geometries, max_error))


def _kept(raw):
    """hloc's per-pair datasets -> (matches, scores): the (M, 2) uint64 and (M,) float32 arrays read_matches_hloc returns."""
    matches, scores = [], []
    for r in raw:
        m = r["matches0"]
        idx = np.where(m != -1)[0]
        matches.append(np.stack([idx, m[idx]], -1).astype(np.uint64))
        scores.append(r["matching_scores0"][idx].astype(np.float32))
    return matches, scores


GUIDE_KINDS = {"E": GUIDE_EPIPOLAR, "F": GUIDE_EPIPOLAR, "H": GUIDE_HOMOGRAPHY}


def guided_model(geometry):
    """The model a pair is matched under: ("E" | "F" | "H", (3, 3) float64 in the normalised plane), or None.  With a "config"
    (TwoViewClassifier.classify_pairs) the model that decided it (fundamental.DECIDING_MODEL); without one
    (TwoViewVerifier.verify_pairs) E when "success".  None: no success, DEGENERATE, or the model is missing."""
    if "config" in geometry:
        if geometry["config"] not in DECIDING_MODEL:
            raise ValueError("unknown configuration %r (known: %s)" % (geometry["config"], ", ".join(DECIDING_MODEL)))
        letter = DECIDING_MODEL[geometry["config"]]
    else:
        letter = "E" if geometry.get("success") else None
    model = geometry.get(letter) if letter else None
    if model is None:
        return None
    return letter, np.asarray(model, dtype=np.float64).reshape(3, 3)


def mean_focal(camera):
    """The focal length the estimators divide a pixel threshold by: f, or the mean of fx and fy."""
    return float(camera.params[0]) if camera.model_id in (0, 2, 3, 8, 9) else 0.5 * (float(camera.params[0]) + float(camera.params[1]))


def guided_threshold(letter, camera_a, camera_b, max_error):
    """max_error pixels in the normalised plane, as the estimator of the model scores it: E and F over both cameras
    ((max_error / f_a + max_error / f_b) / 2), H over the second (max_error / f_b)."""
    if letter not in GUIDE_KINDS:
        raise ValueError("unknown model %r (known: %s)" % (letter, ", ".join(GUIDE_KINDS)))
    if letter == "H":
        return max_error / mean_focal(camera_b)
    return (max_error / mean_focal(camera_a) + max_error / mean_focal(camera_b)) / 2


def pairs_2d3d_from_matches(matches_per_db_image, db_point3D_ids):
    """The 2D-3D pairs of a query from its matches against database images, in the form QueryLocalizer.localize takes.

    matches_per_db_image: {db image: (M, 2) (query keypoint, db keypoint)} (or a list of (db image, matches) in the order to
    visit); db_point3D_ids: {db image: (n_keypoints,) the 3D point of every keypoint, -1 for none}.  Matches whose database
    keypoint has no 3D point are dropped, duplicate (query keypoint, point) pairs are dropped; the result is grouped by query
    keypoint in order of first appearance, and within one keypoint by first appearance of the point id.
    Returns (point2D_idxs (K,) int64, point3D_ids (K,) int64)."""
    items = matches_per_db_image.items() if hasattr(matches_per_db_image, "items") else matches_per_db_image
    by_kp = {}
    for db, m in items:
        ids = np.asarray(db_point3D_ids[db]).reshape(-1)
        for q, k in np.asarray(m, dtype=np.int64).reshape(-1, 2):
            pid = int(ids[k])
            if pid < 0:
                continue
            seen = by_kp.setdefault(int(q), [])
            if pid not in seen:
                seen.append(pid)
    p2d = [q for q, ids in by_kp.items() for _ in ids]
    p3d = [pid for ids in by_kp.values() for pid in ids]
    return np.asarray(p2d, dtype=np.int64), np.asarray(p3d, dtype=np.int64)
