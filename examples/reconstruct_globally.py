#!/usr/bin/env python
"""A low-parallax sequence that the incremental mapper gives up on, reconstructed by the global mapper.

A ring of 100 images, 3.6 degrees between neighbours, 1500 points each seen by six consecutive images, 0.5 px of keypoint noise,
matches from ground truth, geometries from TwoViewVerifier.  No pair of images shares a hundred points under sixteen degrees of
parallax, so IncrementalMapper ends in `no_initial_pair`; GlobalMapper averages the pairs' rotations, positions all centres and
points at once, and refines with the same triangulation and bundle adjustment.  The errors against ground truth are printed after
align_reconstructions (a model without given poses has its own frame and scale).

    python examples/reconstruct_globally.py            # needs an MI355X and the built libpixsfm_hip.so
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pixel-perfect-sfm_amd"))

from pixsfm_amd import synthetic                                                   # noqa: E402
from pixsfm_amd.api import (BundleAdjustmentSetup, GeometricBundleOptimizer, GlobalMapper, IncrementalMapper,  # noqa: E402
                            TwoViewVerifier, align_reconstructions, build_matching_graph, compare_reconstructions)
from pixsfm_amd.api.keypoint_adjustment import default_context                    # noqa: E402
from pixsfm_amd.api.reconstruction import Camera, Image, Reconstruction            # noqa: E402
from pixsfm_amd.api.triangulation import mean_reprojection_error                  # noqa: E402

PARAMS = [1200.0, 500.0, 500.0, 0.02]                                              # SIMPLE_RADIAL


def make_scene(n_images, n_points, views=6, sigma=0.5, seed=0):
    """Names, ground-truth poses, keypoints, and the point behind every keypoint."""
    rng = np.random.default_rng(seed)
    qvec, tvec = synthetic.ring_cameras(n_images, rng=rng)
    names = ["image%03d.jpg" % i for i in range(n_images)]
    X = rng.uniform(-1, 1, (n_points, 3))
    kps, owner = {n: [] for n in names}, {n: [] for n in names}
    for p in range(n_points):
        first = rng.integers(n_images)
        for j in range(views):
            i = (first + j) % n_images
            kps[names[i]].append(synthetic.project(2, PARAMS, qvec[i], tvec[i], X[p]) + rng.normal(0, sigma, 2))
            owner[names[i]].append(p)
    return (names, {names[i]: (qvec[i], tvec[i]) for i in range(n_images)}, {n: np.array(kps[n]) for n in names},
            {n: np.array(owner[n]) for n in names})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--points", type=int, default=1500)
    args = ap.parse_args()
    names, poses, kps, owner = make_scene(args.images, args.points)
    camera = Camera(1, "SIMPLE_RADIAL", 1000, 1000, PARAMS)
    cameras = {n: camera for n in names}
    pairs, matches = [], []
    for a in range(len(names)):
        for b in range(a + 1, len(names)):
            common, ia, ib = np.intersect1d(owner[names[a]], owner[names[b]], return_indices=True)
            if len(common):
                pairs.append((names[a], names[b]))
                matches.append(np.stack([ia, ib], 1))
    _, _, geoms = TwoViewVerifier.create({}).verify_pairs(kps, cameras, pairs, matches)
    print("%d images, %d pairs with matches, %d with a geometry" % (len(names), len(pairs), sum(bool(g["success"]) for g in geoms)))
    graph = build_matching_graph(pairs, matches, [np.ones(len(m)) for m in matches])
    labels = [int(owner[graph.image_id_to_name[node.image_id]][int(node.feature_idx)]) for node in graph.nodes]

    _, summary = IncrementalMapper.create({}).reconstruct(cameras, kps, graph, pairs, geoms, track_labels=labels)
    print("incremental mapper: %s after %d initial-pair trials" % (summary["status"], len(summary["init_trials"])))

    model, summary = GlobalMapper.create({}).reconstruct(cameras, kps, graph, pairs, geoms, track_labels=labels)
    print("global mapper: %s, root %s, %d of %d images, %d points; %d averaging iterations, residual histogram %s, %d positioning rounds"
          % (summary["status"], summary["root"], summary["num_reg_images"], len(names), summary["num_points3D"],
             summary.get("rotation_iterations", 0), summary.get("residual_histogram"), summary.get("positioning_rounds", 0)))
    if summary["num_reg_images"] < 3:
        return
    id_of = {im.name: i for i, im in model.images.items()}
    setup = BundleAdjustmentSetup()
    setup.add_images(model.reg_image_ids())
    setup.set_constant_pose(id_of[summary["root"]])
    far = id_of[summary["gauge_image"]]
    setup.set_constant_tvec(far, [int(np.argmax(np.abs(model.images[far].tvec)))])
    setup.set_constant_camera(1)
    GeometricBundleOptimizer({'loss': {'name': 'trivial', 'params': []}, 'print_summary': False}, setup).run(model)

    truth = Reconstruction()
    truth.add_camera(camera)
    for i, im in model.images.items():
        truth.add_image(Image(i, im.name, 1, *poses[im.name]))
    sim3, inliers = align_reconstructions(model, truth, max_error=0.5)
    diff = compare_reconstructions(model, truth, sim3)
    print("after alignment (%d of %d centres inliers): max rotation error %.4f deg, max centre error %.4f (ring radius 10), mean "
          "reprojection error %.4f px" % (inliers.sum(), len(inliers), max(diff["dR"]), max(diff["dt"]),
                                          mean_reprojection_error(default_context(), model)))


if __name__ == "__main__":
    main()
