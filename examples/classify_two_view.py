#!/usr/bin/env python
"""What the two-view configurations are for: one cloud of points seen by a camera that translates, by a camera that only
rotates, and a wall seen by a camera that translates in front of it.  TwoViewVerifier fits an essential matrix to all three
pairs and reports success with a relative pose for each -- for the rotating camera a pose whose translation direction means
nothing, since the pair has no baseline.  TwoViewClassifier runs the homography estimator on the same matches and says which
pair is which: CALIBRATED, PANORAMIC, PLANAR.

Then the translating pair once more, and a camera that moves forward while it turns, handed over with the focal length stated
x 0.7 (a photograph without EXIF and a guessed focal length): the essential matrix still "verifies" both, the second with a third
of its inliers gone and nothing that says why; with "fundamental" set the classifier runs the seven-point estimator next to it,
which finds the matches that are there, and the forward pair is called UNCALIBRATED.  The sideways pair is one of the geometries
that barely constrain the focal length: E keeps nearly everything there, and only a camera declared untrusted makes it UNCALIBRATED.

    python examples/classify_two_view.py            # needs an MI355X and the built libpixsfm_hip.so
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pixel-perfect-sfm_amd"))

from pixsfm_amd import synthetic                                                   # noqa: E402
from pixsfm_amd.api import TwoViewClassifier, TwoViewVerifier                      # noqa: E402
from pixsfm_amd.api.reconstruction import Camera                                   # noqa: E402

PARAMS = [1200.0, 500.0, 500.0, 0.02]                                              # SIMPLE_RADIAL
EXPECTED = {"translating": "CALIBRATED", "rotating": "PANORAMIC", "wall": "PLANAR"}
WRONG_FOCAL = 0.7


def project(X, R, t):
    """SIMPLE_RADIAL pixels of the points X under the pose (R, t)."""
    p = X @ R.T + t
    u, v = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
    s = 1.0 + PARAMS[3] * (u * u + v * v)
    return np.stack([PARAMS[0] * u * s + PARAMS[1], PARAMS[0] * v * s + PARAMS[2]], 1)


def rotation(axis, angle):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    return synthetic.qvec_to_rotmat(np.concatenate([[np.cos(0.5 * angle)], np.sin(0.5 * angle) * axis]))


def make_scene(n=300, outliers=0.25, sigma=0.5, seed=0):
    """keypoints, pairs and matches of three image pairs; every pair has n matches, a share `outliers` of them wrong."""
    rng = np.random.default_rng(seed)
    rays = np.concatenate([rng.uniform(-0.3, 0.3, (n, 2)), np.ones((n, 1))], 1)
    cloud = rays * rng.uniform(3.0, 12.0, (n, 1))                                  # depths 3-12 in front of the first camera
    normal = np.array([0.25, -0.1, 1.0])
    wall = rays * (7.0 / (rays @ normal))[:, None]                                 # the plane normal . X = 7
    views = {"translating": (cloud, rotation([0.2, 1.0, 0.1], 0.08), np.array([1.5, 0.2, 0.3])),
             "rotating": (cloud, rotation([0.1, 1.0, -0.2], 0.15), np.zeros(3)),
             "wall": (wall, rotation([0.2, 1.0, 0.1], 0.08), np.array([1.5, 0.2, 0.3]))}
    keypoints, pairs, matches = {}, [], []
    for name, (X, R, t) in views.items():
        a, b = name + "_1.jpg", name + "_2.jpg"
        xy1 = project(X, np.eye(3), np.zeros(3)) + rng.normal(0, sigma, (n, 2))
        xy2 = project(X, R, t) + rng.normal(0, sigma, (n, 2))
        wrong = rng.permutation(n)[:int(outliers * n)]
        xy2[wrong] = rng.uniform(0, 1000, (len(wrong), 2))
        keypoints[a], keypoints[b] = xy1, xy2
        pairs.append((a, b))
        matches.append(np.stack([np.arange(n), np.arange(n)], 1))
    return keypoints, pairs, matches


def main():
    keypoints, pairs, matches = make_scene()
    camera = Camera(1, "SIMPLE_RADIAL", 1000, 1000, PARAMS)
    cameras = {name: camera for name in keypoints}
    _, _, plain = TwoViewVerifier.create({}).verify_pairs(keypoints, cameras, pairs, matches)
    kept, _, geoms = TwoViewClassifier.create({}).classify_pairs(keypoints, cameras, pairs, matches)
    print("%-12s %-11s %5s %5s %5s   %s" % ("pair", "class", "n_E", "n_H", "n_R", "matches kept"))
    for (a, _), g, m in zip(pairs, geoms, kept):
        print("%-12s %-11s %5d %5d %5d   %d" % (a[:-6], g["config"], g.get("num_inliers", 0), g["num_inliers_H"], g["num_inliers_R"], len(m)))
    g = plain[1]
    print("TwoViewVerifier alone on the rotating pair: success %s, %d inliers, translation direction (%.3f, %.3f, %.3f) -- of a camera that did not move"
          % (g["success"], g["num_inliers"], *g["tvec"]))
    got = {a[:-6]: g["config"] for (a, _), g in zip(pairs, geoms)}
    assert got == EXPECTED, got

    # two pairs with a focal length that is off: the translating pair of above, and a camera that moves forward while it turns
    rng = np.random.default_rng(1)
    n = 300
    rays = np.concatenate([rng.uniform(-0.3, 0.3, (n, 2)), np.ones((n, 1))], 1)
    cloud = rays * rng.uniform(3.0, 12.0, (n, 1))
    keypoints["forward_1.jpg"] = project(cloud, np.eye(3), np.zeros(3)) + rng.normal(0, 0.5, (n, 2))
    xy2 = project(cloud, rotation([0.3, 1.0, 0.2], 0.25), np.array([0.4, 0.2, 1.2])) + rng.normal(0, 0.5, (n, 2))
    wrong = rng.permutation(n)[:n // 4]
    xy2[wrong] = rng.uniform(0, 1000, (len(wrong), 2))
    keypoints["forward_2.jpg"] = xy2
    two, two_matches = [pairs[0], ("forward_1.jpg", "forward_2.jpg")], [matches[0]] * 2
    guessed = Camera(2, "SIMPLE_RADIAL", 1000, 1000, [WRONG_FOCAL * PARAMS[0]] + PARAMS[1:])
    with_f = TwoViewClassifier.create({"fundamental": {}})
    print("with the fundamental matrix next to it; focal length stated x %.1f where it says wrong:" % WRONG_FOCAL)
    for label, cam, prior in (("true", camera, True), ("wrong, trusted", guessed, True), ("wrong, no prior", guessed, False)):
        m, _, gs = with_f.classify_pairs(keypoints, {x: cam for x in keypoints}, two, two_matches, prior_focal_length={x: prior for x in keypoints})
        for (x, _), g, kept_m in zip(two, gs, m):
            print("  %-12s %-16s %-13s n_E %3d  n_F %3d  matches kept %d" % (x[:-6], label, g["config"], g.get("num_inliers", 0), g["num_inliers_F"], len(kept_m)))
            got[x[:-6] + ", " + label] = g["config"]
    # sideways motion barely constrains the focal length: E keeps nearly all of F's inliers and the pair stays CALIBRATED unless
    # the camera is declared untrusted; forward motion does, and E loses a third of them
    assert got["translating, true"] == got["forward, true"] == "CALIBRATED" and got["forward, wrong, trusted"] == "UNCALIBRATED", got
    assert got["translating, wrong, no prior"] == got["forward, wrong, no prior"] == "UNCALIBRATED", got
    return got


if __name__ == "__main__":
    main()
