"""GPU: pixsfm_amd.api.retrieval end to end.  A ring of 24 images over 600 points, each seen by a window of neighbouring images
(retrieval_cases.ring_scene: D = 32, K = 16, num_matched = 4): the library's pairs equal the reference's exactly, and the
reference's pairs are good ones -- at least 0.9 of them between images that share at least 20 points, their union connecting all
24 images (tests/test_retrieval_cpu.py checks the same without a GPU).  A ring of 12 images then goes through DescriptorMatcher
-> TwoViewVerifier -> IncrementalMapper on retrieved pairs and on exhaustive pairs: the same images are registered."""
import numpy as np
import pytest

import retrieval_cases as rc

pytestmark = pytest.mark.gpu


def test_retrieved_pairs_equal_the_reference_and_follow_the_scene(ctx):
    from pixsfm_amd.api import GlobalDescriptorExtractor, pairs_from_retrieval, unique_pairs
    desc, pts = rc.ring_scene()
    names = list(desc)
    ex = GlobalDescriptorExtractor.create({"n_clusters": 16, "n_iterations": 10}, ctx=ctx)
    g = ex.fit_describe(desc)
    cen, cnt, empty = rc.vocab_train(np.concatenate([desc[n] for n in names]), 16, 10)
    assert ex.centroids.tobytes() == cen.tobytes() and ex.vocabulary.n_empty == empty and np.array_equal(ex.vocabulary.counts, cnt)
    rG = rc.vlad([desc[n] for n in names], cen)[0]
    assert list(g) == names and all(g[n].dtype == np.float32 and g[n].tobytes() == rG[k].tobytes() for k, n in enumerate(names))
    pairs = pairs_from_retrieval(g, 4, ctx=ctx)
    ref = rc.pairs_from_retrieval(dict(zip(names, rG)), 4)
    assert pairs == ref and len(pairs) == 24 * 4
    good = sum(len(pts[a] & pts[b]) >= 20 for a, b in ref)
    assert good >= 0.9 * len(ref), good
    assert rc.connected(names, ref)
    assert all(a != b for a, b in pairs) and len(unique_pairs(pairs)) < len(pairs)
    # queries described with the database's vocabulary; a query that is in the database never pairs with itself
    q = names[:3]
    again = ex.describe({n: desc[n] for n in q})
    assert all(again[n].tobytes() == g[n].tobytes() for n in q)
    sub = pairs_from_retrieval(g, 2, query_names=q, db_names=names[1:], ctx=ctx)
    assert sub == rc.pairs_from_retrieval(g, 2, q, names[1:]) and all(a != b for a, b in sub)


def test_retrieved_pairs_register_the_images_exhaustive_pairs_register(ctx):
    from pixsfm_amd.api import (DescriptorMatcher, GlobalDescriptorExtractor, IncrementalMapper, TwoViewVerifier, base, build_matching_graph,
                                pairs_from_exhaustive, pairs_from_retrieval, unique_pairs)
    from pixsfm_amd.api.reconstruction import Camera
    names, kps, descs = rc.pipeline_scene()
    cameras = {n: Camera(1, "SIMPLE_RADIAL", 1000, 1000, rc.PIPELINE_PARAMS) for n in names}
    g = GlobalDescriptorExtractor.create({"n_clusters": 16}, ctx=ctx).fit_describe(descs)
    retrieved = unique_pairs(pairs_from_retrieval(g, 4, ctx=ctx))
    exhaustive = pairs_from_exhaustive(names)
    assert len(exhaustive) == 66 and len(retrieved) < len(exhaustive) and rc.connected(names, retrieved)
    registered = {}
    for kind, pairs in (("retrieved", retrieved), ("exhaustive", exhaustive)):
        matches, scores = DescriptorMatcher.create("NN-mutual", ctx=ctx).match_pairs(descs, pairs)
        matches, scores, geoms = TwoViewVerifier.create({}, ctx=ctx).verify_pairs(kps, cameras, pairs, matches, scores)
        graph = build_matching_graph(pairs, matches, scores)
        model, summary = IncrementalMapper.create({}, ctx=ctx).reconstruct(cameras, kps, graph, pairs, geoms,
                                                                           track_labels=base.compute_track_labels(graph))
        registered[kind] = sorted(im.name for im in model.images.values())
        print(kind, len(pairs), "pairs,", summary["num_reg_images"], "images,", summary["num_points3D"], "points")
    assert len(registered["exhaustive"]) >= 3
    assert registered["retrieved"] == registered["exhaustive"]
