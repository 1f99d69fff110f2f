#!/usr/bin/env python
"""Localize a batch of held-out images against a map of two well-separated places: two rings of cameras, each around its own
cloud of points, with two images of each ring held out as queries.  Retrieval is played by lists that mix the images of both
places.  MapLocalizer.localize_queries matches all queries against their lists in one launch, gathers the 2D-3D pairs on the
device and estimates all poses in one launch -- once over each query's whole list, once per covisibility cluster of the list
(pixsfm/localize.py with covisibility_clustering) -- next to the per-query loop over DescriptorMatcher.match_pairs,
pairs_2d3d_from_matches and absolute_pose_estimation.  Prints pairs_from_covisibility's first pairs, the clusters and the pose errors.
Then the pixel-perfect half on a scene with feature patches: QueryLocalizer.localize per query next to
QueryLocalizer.localize_batch (keypoint adjustment, PnP and query bundle adjustment one launch each over all queries).

    python examples/localize_queries.py          # needs an MI355X and the built libpixsfm_hip.so
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pixel-perfect-sfm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import map_localization_cases as lc                                                # noqa: E402  (the scene of the tests)
from pixsfm_amd import synthetic                                                   # noqa: E402
from pixsfm_amd.api import (DescriptorMatcher, MapLocalizer, absolute_pose_estimation, pairs_2d3d_from_matches,  # noqa: E402
                            pairs_from_covisibility)

MATCHER = {"distance_threshold": 0.7}


def pose_error(q, t, truth):
    R, Rt = synthetic.qvec_to_rotmat(q), synthetic.qvec_to_rotmat(truth[0])
    return np.degrees(np.arccos(np.clip((np.trace(R @ Rt.T) - 1) / 2, -1, 1))), np.linalg.norm(-R.T @ t + Rt.T @ truth[1])


def main():
    tp = lc.two_places()
    rec, scene, queries = tp["reconstruction"], tp["scene"], tp["queries"]
    cameras = {q: scene["camera"] for q in queries}
    print("map: %d images, %d points; queries: %s" % (len(rec.images), len(rec.points3D), ", ".join(queries)))
    print("pairs_from_covisibility(num_matched=2):", pairs_from_covisibility(rec, 2)[:6], "...")

    for clustering in (False, True):
        loc = MapLocalizer(rec, {"matcher": MATCHER, "covisibility_clustering": clustering})
        t0 = time.perf_counter()
        res = loc.localize_queries(cameras, scene["keypoints"], tp["descriptors"], tp["retrieval"])
        print("\nlocalize_queries, covisibility_clustering=%s (%.1f ms for the batch)" % (clustering, 1e3 * (time.perf_counter() - t0)))
        for q in queries:
            r = res[q]
            rot, centre = pose_error(r["qvec"], r["tvec"], scene["poses"][q])
            print("  %s: %s, %d clusters %s, best %d, %d inliers of %d pairs, rotation %.4f deg, centre %.5f"
                  % (q, "ok" if r["success"] else "FAILED", len(r["clusters"]), [len(c) for c in r["clusters"]], r["best_cluster"],
                     r["num_inliers"], len(r["inliers"]), rot, centre))

    print("\nthe per-query loop (match_pairs, pairs_2d3d_from_matches, absolute_pose_estimation)")
    by_name = {im.name: im for im in rec.images.values()}
    matcher = DescriptorMatcher.create(MATCHER)
    for q in queries:
        t0 = time.perf_counter()
        pairs = [(q, db) for db in tp["retrieval"][q]]
        matches, _ = matcher.match_pairs(tp["descriptors"], pairs)
        ids = {db: np.array([p.point3D_id for p in by_name[db].points2D]) for _, db in pairs}
        p2d, p3d = pairs_2d3d_from_matches([(db, m) for (_, db), m in zip(pairs, matches)], ids)
        r = absolute_pose_estimation(scene["keypoints"][q][p2d], [rec.points3D[i].xyz for i in p3d], scene["camera"],
                                     estimation_options={"ransac": {"max_error": 12}})
        rot, centre = pose_error(r["qvec"], r["tvec"], scene["poses"][q])
        print("  %s: %d inliers of %d pairs, rotation %.4f deg, centre %.5f (%.1f ms)"
              % (q, r["num_inliers"], len(p2d), rot, centre, 1e3 * (time.perf_counter() - t0)))

    batched_refinement()


def batched_refinement():
    """The pixel-perfect half on a scene that has feature patches (three held-out images of a synthetic map, a fifth of the 2D-3D
    pairs wrong): QueryLocalizer.localize per query, and QueryLocalizer.localize_batch -- keypoint adjustment, PnP and the query
    bundle adjustment one launch each over all queries."""
    from copy import deepcopy

    import test_query_ba_gpu as tq                                                 # the scene of the tests
    from pixsfm_amd.api.keypoint_adjustment import default_context
    s = tq.make_scene(default_context())
    loc, qs = s["localizer"], s["queries"]
    for name, run in (("localize() per query", lambda: [loc.localize(q["keypoints"].copy(), q["kp_idx"], q["p3d_id"], deepcopy(s["camera"]),
                                                                      query_fmaps=[q["fmap"]]) for q in qs]),
                      ("localize_batch()", lambda: loc.localize_batch([tq._as_dict(s, q) for q in qs]))):
        run()                                                                      # the first call loads the kernels
        t0 = time.perf_counter()
        res = run()
        print("\n%s: %.1f ms for %d queries" % (name, 1e3 * (time.perf_counter() - t0), len(qs)))
        for q, r in zip(qs, res):
            ang, centre = tq._pose_error(q, r)
            print("  %d inliers of %d pairs (%d wrong ones among the pairs, %d among the inliers), rotation %.3e rad, centre %.3e"
                  % (r["num_inliers"], len(q["kp_idx"]), int(q["wrong"].sum()), int(np.array(r["inliers"])[q["wrong"]].sum()), ang, centre))


if __name__ == "__main__":
    main()
