#!/usr/bin/env python
"""Localize a held-out image against a refined model: a synthetic scene of nine posed images with featuremetric patches, eight of
them the map; the ninth is localized from 2D-3D pairs with perturbed keypoints and 20 % wrong pairs -- once by PnP alone
(the batched GPU estimator that stands in for pycolmap.absolute_pose_estimation), once with query keypoint adjustment before and
query bundle adjustment after it (QueryLocalizer, pixsfm/localization/main.py).  Prints the pose errors.

    python examples/localize_query.py            # needs an MI355X and the built libpixsfm_hip.so
"""
import os
import sys
from copy import deepcopy

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pixel-perfect-sfm_amd"))

from pixsfm_amd import synthetic                                                   # noqa: E402
from pixsfm_amd.api import QueryLocalizer, features                                # noqa: E402
from pixsfm_amd.api.reconstruction import Camera, reconstruction_from_flat         # noqa: E402


def make_scene(n_images=9, n_points=150, seed=3, keypoint_noise=1.5, wrong=0.2):
    full = synthetic.make_ba_problem(n_cams=n_images, n_points=n_points, obs_per_point=5, channels=64, patch_size=16, seed=seed,
                                     perturb=False, shared_camera=True)
    held = full["obs_image"] == 0                                                  # image 0 is the query
    m = ~held
    flat = dict(full, obs_image=full["obs_image"][m] - 1, obs_point=full["obs_point"][m], obs_patch=full["obs_patch"][m],
                centers=full["centers"][m], image_camera=full["image_camera"][1:], qvec=full["qvec"][1:], tvec=full["tvec"][1:])
    rec, patch_of = reconstruction_from_flat(flat)
    fmaps = {}
    for (image_id, p2d), pi in patch_of.items():
        fm = fmaps.setdefault(rec.images[image_id].name, features.FeatureMap())
        fm.patches[p2d] = features.FeaturePatch(full["patches"][pi], full["corners"][pi], full["scales"][pi])
    manager = features.FeatureManager([features.FeatureSet(fmaps)])
    rng = np.random.default_rng(seed + 1)
    sel = np.flatnonzero(held)
    nq = len(sel)
    keypoints = full["centers"][sel] + rng.uniform(-keypoint_noise, keypoint_noise, (nq, 2))
    kp_idx, p3d_id = list(range(nq)), [int(p) + 1 for p in full["obs_point"][sel]]
    for i in rng.permutation(nq)[:int(wrong / (1 - wrong) * nq)]:                  # wrong pairs: a keypoint with another point
        kp_idx.append(int(i)); p3d_id.append(p3d_id[int(rng.integers(nq))])
    fmap = features.FeatureMap.from_arrays(full["patches"][sel], np.arange(nq), full["corners"][sel], (1.0, 1.0))
    camera = Camera(1, "SIMPLE_RADIAL", 1000, 1000, full["cam_params"][0, :4])
    return rec, manager, keypoints, kp_idx, p3d_id, fmap, camera, full["gt_qvec"][0], full["gt_tvec"][0]


def pose_error(q, t, gt_q, gt_t):
    R0, R1 = synthetic.qvec_to_rotmat(gt_q), synthetic.qvec_to_rotmat(q)
    ang = np.arccos(np.clip((np.trace(R0.T @ R1) - 1) / 2, -1, 1))
    return np.rad2deg(ang), np.linalg.norm(R1.T @ t - R0.T @ gt_t)


def main():
    rec, manager, keypoints, kp_idx, p3d_id, fmap, camera, gt_q, gt_t = make_scene()
    print("map: %d images, %d points; query: %d keypoints, %d 2D-3D pairs" % (len(rec.images), len(rec.points3D), len(keypoints), len(kp_idx)))
    for name, conf in (("PnP alone", {"QKA": {"apply": False}, "QBA": {"apply": False}}), ("QKA + PnP + QBA", None)):
        localizer = QueryLocalizer(rec, conf, dense_features=manager)
        pose = localizer.localize(keypoints, kp_idx, p3d_id, deepcopy(camera), query_fmaps=[fmap])
        if not pose["success"]:
            print("%-16s failed" % name)
            continue
        rot, centre = pose_error(pose["qvec"], pose["tvec"], gt_q, gt_t)
        print("%-16s %3d inliers, rotation error %.5f deg, camera centre error %.6f" % (name, pose["num_inliers"], rot, centre))


if __name__ == "__main__":
    main()
