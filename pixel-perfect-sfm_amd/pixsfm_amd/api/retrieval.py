"""Image retrieval for the accelerated path: local descriptors -> a global descriptor per image -> the image pairs to match.

The reference takes its pairs from hloc: `pairs_from_exhaustive` in the demo, `pairs_from_retrieval` over global descriptors in
examples/sfm+loc_aachen.py (read back by pixsfm/localize.py through parse_retrieval).  hloc's retrieval models need weights and
stay out of this library; what is native here is the classical weight-free descriptor: VLAD with intra-normalisation over a
vocabulary learned from the scene's own local descriptors (pxr_vocab_train, pxr_vlad_aggregate), and the dense top-k over the
global descriptors (pxr_retrieval_topk), DESIGN.md section 26.  `pairs_from_retrieval` takes any {name: vector}, so global
descriptors computed elsewhere go through the same selection.  The kernels reproduce bit for bit; parity with hloc is not pinned.

    extractor = GlobalDescriptorExtractor.create({'n_clusters': 64})
    global_descriptors = extractor.fit_describe(descriptors)            # {name: (n, D)} as SiftExtractor.extract_images returns
    pairs = unique_pairs(pairs_from_retrieval(global_descriptors, num_matched=20))
    matches, scores = DescriptorMatcher.create("NN-ratio").match_pairs(descriptors, pairs)
"""
import numpy as np

from .. import engine
from . import base
from .keypoint_adjustment import default_context


class GlobalDescriptorExtractor:
    """VLAD global descriptors over a vocabulary fitted to the scene.  A vocabulary learned from one scene must be refitted when
    the scene changes; a query set is described with the database's vocabulary (fit on the database, describe both)."""
    default_conf = {
        'n_clusters': 64,        # K: the global descriptor has K * D entries (at most 32768)
        'n_iterations': 10,      # of spherical k-means
        'max_train': 262144,     # descriptors the vocabulary is learned from, evenly spread over all of them
    }

    def __init__(self, conf=None, ctx=None):
        self.conf = base.merge_conf(self.default_conf, conf)
        self.ctx = ctx
        self.vocabulary = None

    @classmethod
    def create(cls, conf=None, ctx=None):
        return cls(conf, ctx)

    @staticmethod
    def _arrays(descriptors):
        names = list(descriptors)
        arrays = [np.ascontiguousarray(descriptors[n], dtype=np.float32) for n in names]
        for n, a in zip(names, arrays):
            if a.ndim != 2:
                raise ValueError("descriptors of %r must be (n, D), not %s (hloc stores (D, n): transpose)" % (n, a.shape))
        return names, arrays

    def fit(self, descriptors):
        """Learn the vocabulary from {name: (n, D) float32, L2-normalised}.  Deterministic: a function of the descriptors and of
        the order of the names."""
        _, arrays = self._arrays(descriptors)
        self.vocabulary = engine.VladVocabulary.train(self.ctx or default_context(), arrays, int(self.conf['n_clusters']),
                                                      int(self.conf['n_iterations']), int(self.conf['max_train']))
        return self

    def describe(self, descriptors):
        """{name: (n, D)} -> {name: (K * D,) float32} of unit norm (zero for an image without valid descriptors)."""
        if self.vocabulary is None:
            raise RuntimeError("fit() the vocabulary first")
        names, arrays = self._arrays(descriptors)
        if not names:
            return {}
        g = self.vocabulary.aggregate(arrays).download()
        return {n: g[k] for k, n in enumerate(names)}

    def fit_describe(self, descriptors):
        return self.fit(descriptors).describe(descriptors)

    @property
    def centroids(self):
        """(K, D) float32, or None before fit()."""
        return None if self.vocabulary is None else self.vocabulary.centroids


def pairs_from_retrieval(global_descriptors, num_matched, query_names=None, db_names=None, min_score=None, match_mask=None, ctx=None):
    """hloc.pairs_from_retrieval: per query image its `num_matched` most similar database images, as a list [(query, db)] in query
    order and then rank (hloc writes the same list to a text file).  global_descriptors {name: (Dg,) float32}; query_names /
    db_names default to all names; a query that is also in the database never pairs with itself; min_score: the smallest
    similarity kept; match_mask (n_query, n_db) bool: False = excluded.  Ties go to the database image that comes first."""
    names = list(global_descriptors)
    query_names = names if query_names is None else list(query_names)
    db_names = names if db_names is None else list(db_names)
    for n in list(query_names) + list(db_names):
        if n not in global_descriptors:
            raise KeyError("no global descriptor for image %r" % (n,))
    if not query_names or not db_names:
        return []
    if match_mask is not None and np.asarray(match_mask).shape != (len(query_names), len(db_names)):
        raise ValueError("match_mask must be (n_query, n_db) = (%d, %d)" % (len(query_names), len(db_names)))
    stack = lambda ns: np.ascontiguousarray(np.stack([np.asarray(global_descriptors[n], dtype=np.float32).reshape(-1) for n in ns]))  # noqa: E731
    db = stack(db_names)
    query = db if query_names == db_names else stack(query_names)
    where = {n: k for k, n in reversed(list(enumerate(db_names)))}
    query_self = np.array([where.get(n, -1) for n in query_names], dtype=np.int32)
    top, _, found = engine.retrieval_topk(ctx or default_context(), query, db, int(num_matched), query_self=query_self, mask=match_mask,
                                          min_score=min_score)
    top, found = np.asarray(top), np.asarray(found)
    return [(q, db_names[j]) for i, q in enumerate(query_names) for j in top[i, :found[i]]]


def unique_pairs(pairs):
    """The first occurrence of every unordered pair, in order: the list DescriptorMatcher.match_pairs and build_matching_graph
    take (retrieval returns (a, b) and (b, a) whenever each is among the other's neighbours)."""
    seen, out = set(), []
    for a, b in pairs:
        key = frozenset((a, b))
        if key not in seen:
            seen.add(key)
            out.append((a, b))
    return out


def pairs_from_exhaustive(names, ref_names=None):
    """hloc.pairs_from_exhaustive: every unordered pair of `names`, or with ref_names every (name, ref_name)."""
    names = list(names)
    if ref_names is not None:
        return [(a, b) for a in names for b in ref_names]
    return [(names[i], names[j]) for i in range(len(names)) for j in range(i + 1, len(names))]
