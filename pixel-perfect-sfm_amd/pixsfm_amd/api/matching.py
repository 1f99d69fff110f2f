"""Descriptor matching for the accelerated path: descriptors of image pairs -> mutual nearest neighbours.

The reference takes its matches from hloc (`hloc.match_features.main` with the confs "NN-mutual", "NN-ratio" or
"NN-superpoint", read back by pixsfm/util/hloc.py:read_matches_hloc); hloc is not installable where this library runs, so the
stage is native here.  `DescriptorMatcher.create(conf).match_pairs(descriptors, pairs)` returns exactly the two lists
read_matches_hloc returns, so `build_matching_graph(pairs, *matcher.match_pairs(descriptors, pairs))` is the whole step, and
`pairs_2d3d_from_matches` turns the matches of a query against database images into what `QueryLocalizer.localize` takes.
The kernels (pxr_match_descriptors) reproduce bit for bit; parity with hloc is not pinned.
"""
import numpy as np

from ..engine import MATCH_CONFS, MatchProblem
from . import base
from .keypoint_adjustment import default_context


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
    def _run(self, descriptors, pair_indices):
        """descriptors: list of (n, D) float32 arrays; pair_indices: (P, 2) ints into it.  Returns per pair (matches0 (n_a,) int32,
        scores0 (n_a,) float32).  One launch covers all pairs and every image is uploaded once; when the flat outputs (the sum of
        the first images' sizes) would exceed conf max_batch_rows, the pairs are split into consecutive groups below that bound,
        one launch each (a single pair larger than the bound is a launch of its own)."""
        ctx = self.ctx or default_context()
        pair_indices = np.asarray(pair_indices, dtype=np.int64).reshape(-1, 2)
        out = [None] * len(pair_indices)
        if len(pair_indices) == 0:
            return out
        sizes = np.array([len(d) for d in descriptors], dtype=np.int64)
        problem = MatchProblem(ctx, descriptors, pair_indices)           # uploads every image once
        groups, first, rows = [], 0, 0
        for p, (ia, _) in enumerate(pair_indices):
            if p > first and rows + sizes[ia] > int(self.conf['max_batch_rows']):
                groups.append((first, p))
                first, rows = p, 0
            rows += sizes[ia]
        groups.append((first, len(pair_indices)))
        for lo, hi in groups:
            sub = problem if len(groups) == 1 else MatchProblem(ctx, problem.d_desc, pair_indices[lo:hi], image_offsets=problem.image_offsets)
            d_m, d_s, _ = sub.run(**self.options())
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
        matches, scores = [], []
        for r in self.match_raw(descriptors, pairs):
            m = r["matches0"]
            idx = np.where(m != -1)[0]
            matches.append(np.stack([idx, m[idx]], -1).astype(np.uint64))
            scores.append(r["matching_scores0"][idx].astype(np.float32))
        return matches, scores


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
