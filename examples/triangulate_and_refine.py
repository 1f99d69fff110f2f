#!/usr/bin/env python
"""Known poses in, a refined model out: synthetic posed images, noisy keypoints with gross outliers and a match graph ->
track labels -> triangulation (TrackTriangulator, in place of hloc.triangulation.main / pycolmap.triangulate_points) ->
geometric bundle adjustment of the triangulated model.  Prints the point error after each stage.

    python examples/triangulate_and_refine.py            # needs an MI355X and the built libpixsfm_hip.so
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pixel-perfect-sfm_amd"))

from pixsfm_amd import synthetic                                                   # noqa: E402
from pixsfm_amd.api import BundleAdjuster, TrackTriangulator, base                 # noqa: E402
from pixsfm_amd.api.reconstruction import Camera, Image, Reconstruction            # noqa: E402


def make_scene(n_images=12, n_points=400, views=6, sigma=0.5, p_outlier=0.1, seed=0):
    rng = np.random.default_rng(seed)
    qvec, tvec = synthetic.ring_cameras(n_images, rng=rng)
    params = [1200.0, 500.0, 500.0, 0.02]                                          # SIMPLE_RADIAL
    rec = Reconstruction()
    rec.add_camera(Camera(1, "SIMPLE_RADIAL", 1000, 1000, params))
    names = ["image%02d.jpg" % i for i in range(n_images)]
    for i in range(n_images):
        rec.add_image(Image(i + 1, names[i], 1, qvec[i], tvec[i]))
    X = rng.uniform(-1, 1, (n_points, 3))
    keypoints = {n: [] for n in names}
    graph = base.Graph()
    for p in range(n_points):
        first = rng.integers(n_images)
        seen = [(first + j) % n_images for j in range(views)]                      # neighbouring images see the point
        idx = []
        for i in seen:
            xy = synthetic.project(2, params, qvec[i], tvec[i], X[p]) + rng.normal(0, sigma, 2)
            if rng.random() < p_outlier:                                           # a wrong detection
                a = rng.uniform(0, 2 * np.pi)
                xy = xy + rng.uniform(100, 300) * np.array([np.cos(a), np.sin(a)])
            idx.append(len(keypoints[names[i]]))
            keypoints[names[i]].append(xy)
        for a in range(views - 1):                                                 # matches along the chain of views
            graph.register_matches(names[seen[a]], names[seen[a + 1]], [[idx[a], idx[a + 1]]], [rng.uniform(0.5, 1.0)])
    return rec, {n: np.array(k).reshape(-1, 2) for n, k in keypoints.items()}, graph, X


def main():
    rec, keypoints, graph, X = make_scene()
    labels = base.compute_track_labels(graph)
    triangulator = TrackTriangulator.create({"refine": False})
    model, summary = triangulator.triangulate(rec, keypoints, graph, track_labels=labels)
    print("triangulation: %d tracks -> %d points (status %s), mean track length %.2f, mean reprojection error %.3f px"
          % (summary["num_tracks"], summary["num_points3D"], summary["status"], summary["mean_track_length"],
             summary["mean_reprojection_error"]))

    def errors(m):
        # a point's scene point: the one nearest to it (the scene points are ~0.2 apart, the errors ~0.005)
        P = np.array([m.points3D[i].xyz for i in m.point3D_ids()])
        return np.sqrt(((P[:, None, :] - X[None, :, :]) ** 2).sum(-1)).min(1)
    e0 = errors(model)
    print("point error after triangulation:           median %.5f   max %.5f" % (np.median(e0), e0.max()))

    refined, _ = TrackTriangulator.create({"refine": True}).triangulate(rec, keypoints, graph, track_labels=labels)
    e1 = errors(refined)
    print("point error after points-only refinement:  median %.5f   max %.5f" % (np.median(e1), e1.max()))

    out = BundleAdjuster.create({"strategy": "geometric"}).refine(refined)
    e2 = errors(refined)
    print("point error after geometric BA:            median %.5f   max %.5f   (%s)" % (np.median(e2), e2.max(), out["summary"].BriefReport()))


if __name__ == "__main__":
    main()
