#!/usr/bin/env python
"""From descriptors to a model without a given pair list: GlobalDescriptorExtractor (a VLAD vocabulary fitted to the scene's own
descriptors) -> pairs_from_retrieval (num_matched = 8 neighbours per image) -> DescriptorMatcher -> TwoViewClassifier ->
IncrementalMapper -> geometric bundle adjustment, on a synthetic ring of 40 images -- and the same run on exhaustive pairs (780 of
them) next to it: pairs matched, images registered, points, reprojection error.  The scene, the gauge and the bundle adjustment
are those of examples/reconstruct_from_matches.py.

    python examples/retrieve_match_reconstruct.py          # needs an MI355X and the built libpixsfm_hip.so
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pixel-perfect-sfm_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from reconstruct_from_matches import PARAMS, adjust, errors, make_scene            # noqa: E402

from pixsfm_amd.api import (DescriptorMatcher, GlobalDescriptorExtractor, IncrementalMapper, TwoViewClassifier, base,  # noqa: E402
                            build_matching_graph, pairs_from_exhaustive, pairs_from_retrieval, unique_pairs)
from pixsfm_amd.api.keypoint_adjustment import default_context                    # noqa: E402
from pixsfm_amd.api.reconstruction import Camera                                   # noqa: E402
from pixsfm_amd.api.triangulation import mean_reprojection_error                  # noqa: E402


def reconstruct(names, cameras, kps, descs, pairs):
    """Match, classify, map and adjust over `pairs`: (model, summary, pairs with a geometry, seconds)."""
    t0 = time.perf_counter()
    matches, scores = DescriptorMatcher.create("NN-mutual").match_pairs(descs, pairs)
    matches, scores, geoms = TwoViewClassifier.create({}).classify_pairs(kps, cameras, pairs, matches, scores)
    graph = build_matching_graph(pairs, matches, scores)
    model, summary = IncrementalMapper.create({}).reconstruct(cameras, kps, graph, pairs, geoms, track_labels=base.compute_track_labels(graph))
    if summary["num_reg_images"] >= 3:
        id_of = {im.name: i for i, im in model.images.items()}
        adjust(model, *(id_of[n] for n in summary["initial_pair"]))
    return model, summary, sum(bool(g["success"]) for g in geoms), time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=40)
    ap.add_argument("--points", type=int, default=1200)
    ap.add_argument("--num-matched", type=int, default=8)
    ap.add_argument("--clusters", type=int, default=32)
    args = ap.parse_args()
    names, poses, kps, descs, owner, X = make_scene(args.images, args.points)
    cameras = {n: Camera(1, "SIMPLE_RADIAL", 1000, 1000, PARAMS) for n in names}

    t0 = time.perf_counter()
    extractor = GlobalDescriptorExtractor.create({"n_clusters": args.clusters})
    global_descriptors = extractor.fit_describe(descs)
    retrieved = unique_pairs(pairs_from_retrieval(global_descriptors, args.num_matched))
    t_retrieval = time.perf_counter() - t0
    exhaustive = pairs_from_exhaustive(names)
    shared = lambda a, b: len(set(owner[a][owner[a] >= 0]) & set(owner[b][owner[b] >= 0]))   # noqa: E731
    print("%d images, %d descriptors; vocabulary of %d words (%d empty), global descriptors of %d entries, retrieval in %.3f s"
          % (len(names), sum(len(d) for d in descs.values()), args.clusters, extractor.vocabulary.n_empty,
             len(next(iter(global_descriptors.values()))), t_retrieval))
    print("retrieved pairs that share at least 20 points: %d of %d (exhaustive: %d of %d)"
          % (sum(shared(a, b) >= 20 for a, b in retrieved), len(retrieved), sum(shared(a, b) >= 20 for a, b in exhaustive), len(exhaustive)))

    print("%-12s %7s %10s %10s %8s %10s %13s %9s" % ("pairs", "matched", "geometries", "registered", "points", "reproj px", "rotation deg", "seconds"))
    for title, pairs in (("retrieved", retrieved), ("exhaustive", exhaustive)):
        model, summary, n_geom, seconds = reconstruct(names, cameras, kps, descs, pairs)
        if summary["num_reg_images"] < 3:
            print("%-12s %7d %10d %10d" % (title, len(pairs), n_geom, summary["num_reg_images"]))
            continue
        rot, _, _ = errors(model, poses, owner, X)
        print("%-12s %7d %10d %10d %8d %10.4f %13.5f %9.2f" % (title, len(pairs), n_geom, summary["num_reg_images"], len(model.points3D),
                                                              mean_reprojection_error(default_context(), model), rot, seconds))
    print("pairs saved: %d of %d" % (len(exhaustive) - len(retrieved), len(exhaustive)))


if __name__ == "__main__":
    main()
