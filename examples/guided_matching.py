#!/usr/bin/env python
"""What guided matching is for: a scene in which EVERY point has a twin -- another 3D point with the same descriptor, as the
windows of one facade have.  The ratio test then discards nearly every true match (the second best is as good as the best), and
mutual nearest neighbours keep a coin toss.  Once a pair has a two-view model, it is matched again under the model
(DescriptorMatcher.match_pairs_guided): only candidates near the epipolar line compete, the twin drops out, and the ratio test
passes.  Stages, each classified (TwoViewClassifier) and triangulated:

    A  NN-ratio                        -> classify
    B  NN-mutual                       -> classify
    C  guided NN-ratio under B's models -> classify again

    python examples/guided_matching.py            # needs an MI355X and the built libpixsfm_hip.so
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pixel-perfect-sfm_amd"))
sys.path.insert(0, os.path.join(ROOT, "examples"))

from match_verify_triangulate import PARAMS, count, unit                           # noqa: E402
from pixsfm_amd import synthetic                                                   # noqa: E402
from pixsfm_amd.api import DescriptorMatcher, TrackTriangulator, TwoViewClassifier  # noqa: E402
from pixsfm_amd.api.reconstruction import Camera, Image, Reconstruction            # noqa: E402


def make_scene(n_images=6, n_points=200, dim=64, sigma=0.5, desc_noise=0.03, seed=0):
    """Posed images that all see 2 n_points points; point n_points + k carries the descriptor of point k.  Per observation
    descriptor noise (renormalised) and keypoint noise in pixels; keypoints in shuffled order."""
    rng = np.random.default_rng(seed)
    qvec, tvec = synthetic.ring_cameras(n_images, rng=rng)
    names = ["image%02d.jpg" % i for i in range(n_images)]
    camera = Camera(1, "SIMPLE_RADIAL", 1000, 1000, PARAMS)
    rec = Reconstruction()
    rec.add_camera(camera)
    for i in range(n_images):
        rec.add_image(Image(i + 1, names[i], 1, qvec[i], tvec[i]))
    X = rng.uniform(-1, 1, (2 * n_points, 3))
    D = unit(rng.standard_normal((n_points, dim)))
    D = np.concatenate([D, D])
    kps, descs, owner = {}, {}, {}
    for i, n in enumerate(names):
        order = rng.permutation(2 * n_points)
        kps[n] = np.array([synthetic.project(2, PARAMS, qvec[i], tvec[i], X[p]) for p in order]) + rng.normal(0, sigma, (len(order), 2))
        descs[n] = unit(D[order] + desc_noise * rng.standard_normal((len(order), dim)) / np.sqrt(dim)).astype(np.float32)
        owner[n] = order
    return rec, camera, names, kps, descs, owner


def stage(title, rec, names, kps, cams, owner, pairs, matches, scores):
    """Classify the matches of a stage, triangulate what the classifier keeps, print right / wrong before and after."""
    total, wrong = count(owner, pairs, matches, scores)[:2]
    kept_m, kept_s, geoms = TwoViewClassifier.create({}).classify_pairs(kps, cams, pairs, matches, scores)
    k_total, k_wrong, _, _, graph, labels = count(owner, pairs, kept_m, kept_s)
    points = 0
    if k_total:
        points = TrackTriangulator.create({}).triangulate(rec, {n: kps[n] for n in names}, graph, track_labels=labels)[1]["num_points3D"]
    print("%-34s %5d right %5d wrong | classified: %2d of %2d pairs with a model, %5d right %5d wrong | %4d points triangulated"
          % (title, total - wrong, wrong, sum(bool(g["success"]) for g in geoms), len(pairs), k_total - k_wrong, k_wrong, points))
    return geoms


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--max-error", type=float, default=4.0, help="the gate's threshold in pixels")
    args = ap.parse_args()
    rec, camera, names, kps, descs, owner = make_scene()
    cams = {n: camera for n in names}
    pairs = [(names[i], names[i + 1]) for i in range(len(names) - 1)] + [(names[i], names[i + 2]) for i in range(len(names) - 2)]
    print("%d images of %d keypoints, %d pairs; every point has a twin with the same descriptor" % (len(names), len(owner[names[0]]), len(pairs)))
    ratio, mutual = DescriptorMatcher.create("NN-ratio"), DescriptorMatcher.create("NN-mutual")
    stage("A  NN-ratio:", rec, names, kps, cams, owner, pairs, *ratio.match_pairs(descs, pairs))
    geoms = stage("B  NN-mutual:", rec, names, kps, cams, owner, pairs, *mutual.match_pairs(descs, pairs))
    guided = ratio.match_pairs_guided(descs, kps, cams, pairs, geoms, max_error=args.max_error)
    stage("C  guided NN-ratio under B's models:", rec, names, kps, cams, owner, pairs, *guided)


if __name__ == "__main__":
    main()
