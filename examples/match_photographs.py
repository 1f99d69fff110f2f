#!/usr/bin/env python
"""Photographs in, verified matches out, without leaving the library: two views of a photograph pinned to a wall are rendered
from known cameras and written as PNG files; SiftExtractor finds keypoints and descriptors, DescriptorMatcher("NN-ratio")
matches them, TwoViewClassifier says what kind of pair it is.  The scene is a plane, so the class should be PLANAR, and a match
can be checked against the mapping the plane induces between the two views.

    python examples/match_photographs.py            # needs an MI355X and the built libpixsfm_hip.so
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pixel-perfect-sfm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))                                   # real_scene: the golden tile and its renderer

import real_scene as rs                                                            # noqa: E402
from pixsfm_amd.api import DescriptorMatcher, SiftExtractor, TwoViewClassifier      # noqa: E402
from pixsfm_amd.api.reconstruction import Camera                                   # noqa: E402


def plane_map(kp, Ra, ta, Rb, tb):
    """COLMAP pixels of view a -> the plane z = 0 -> COLMAP pixels of view b."""
    d = np.stack([(kp[:, 0] - rs.VIEW / 2) / rs.FOCAL, (kp[:, 1] - rs.VIEW / 2) / rs.FOCAL, np.ones(len(kp))], -1) @ Ra
    c = -Ra.T @ ta
    X = c + (-c[2] / d[:, 2])[:, None] * d
    p = X @ Rb.T + tb
    return np.stack([rs.FOCAL * p[:, 0] / p[:, 2] + rs.VIEW / 2, rs.FOCAL * p[:, 1] / p[:, 2] + rs.VIEW / 2], -1)


def main():
    from PIL import Image
    Rs, ts = rs.cameras(2, 3)
    tile = rs.load_tile(0)
    names = ["left.png", "right.png"]
    with tempfile.TemporaryDirectory() as d:
        for name, R, t in zip(names, Rs, ts):
            Image.fromarray(np.round(rs.render_view(tile, R, t).transpose(1, 2, 0)).astype(np.uint8)).save(os.path.join(d, name))
        keypoints, descriptors = SiftExtractor.create().extract_images(d, names)
    print("features: %d and %d" % tuple(len(keypoints[n]) for n in names))
    matches, _ = DescriptorMatcher.create("NN-ratio").match_pairs(descriptors, [tuple(names)])
    m = matches[0].astype(np.int64)
    a, b = keypoints[names[0]][m[:, 0]], keypoints[names[1]][m[:, 1]]
    err = np.linalg.norm(plane_map(a, Rs[0], ts[0], Rs[1], ts[1]) - b, axis=1)
    print("matches: %d, of which %d within 3 px of the plane-induced mapping (median error %.2f px)" % (len(m), (err <= 3).sum(), np.median(err)))
    cam = Camera(1, "SIMPLE_PINHOLE", rs.VIEW, rs.VIEW, [rs.FOCAL, rs.VIEW / 2, rs.VIEW / 2])
    kept, _, geoms = TwoViewClassifier.create({}).classify_pairs(keypoints, {n: cam for n in names}, [tuple(names)], [matches[0]])
    g = geoms[0]
    print("two-view configuration: %s (%d inliers of the homography, %d matches kept)" % (g["config"], g["num_inliers_H"], len(kept[0])))
    return g["config"]


if __name__ == "__main__":
    main()
