#!/usr/bin/env python
"""How certain is a refined model?  The ring scene of examples/reconstruct_from_matches.py (known poses, tracks from the scene's
own keypoints) -> TrackTriangulator -> geometric bundle adjustment with that example's gauge -> estimate_ba_covariance.  Prints the
five least certain images and points, and checks that the standard deviation of a point's DEPTH -- its position along the mean
viewing ray of the cameras that see it, given those cameras -- grows with its distance from them.

    python examples/pose_uncertainty.py            # needs an MI355X and the built libpixsfm_hip.so
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pixel-perfect-sfm_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pixsfm_amd import synthetic                                                   # noqa: E402
from pixsfm_amd.api import BundleAdjustmentSetup, GeometricBundleOptimizer, TrackTriangulator, base, estimate_ba_covariance  # noqa: E402
from pixsfm_amd.api.reconstruction import Camera, Image, Reconstruction            # noqa: E402
from reconstruct_from_matches import PARAMS, make_scene                            # noqa: E402

OPTIONS = {'loss': {'name': 'trivial', 'params': []}, 'print_summary': False}


def example_setup(rec, first_id, second_id):
    """the gauge of reconstruct_from_matches.adjust: one pose, one translation component of a second image, the cameras"""
    setup = BundleAdjustmentSetup()
    setup.add_images(rec.reg_image_ids())
    setup.set_constant_pose(first_id)
    setup.set_constant_tvec(second_id, [int(np.argmax(np.abs(rec.images[second_id].tvec)))])
    for c in rec.cameras:
        setup.set_constant_camera(c)
    return setup


def track_graph(names, owner):
    """the scene's own tracks as a matching graph: keypoints that show the same point are matched in a chain"""
    seen, pairs, matches, scores = {}, [], [], []
    for n in names:
        for k, p in enumerate(owner[n]):
            if p >= 0:
                seen.setdefault(int(p), []).append((n, k))
    by_pair = {}
    for obs in seen.values():
        for (a, i), (b, j) in zip(obs[:-1], obs[1:]):
            by_pair.setdefault((a, b), []).append((i, j))
    for pair, m in by_pair.items():
        pairs.append(pair); matches.append(np.array(m)); scores.append(np.ones(len(m)))
    return pairs, matches, scores


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=12)
    ap.add_argument("--points", type=int, default=400)
    args = ap.parse_args()
    names, poses, kps, descs, owner, X = make_scene(args.images, args.points)
    from pixsfm_amd.api import build_matching_graph
    pairs, matches, scores = track_graph(names, owner)
    graph = build_matching_graph(pairs, matches, scores)
    labels = base.compute_track_labels(graph)
    rec = Reconstruction()
    rec.add_camera(Camera(1, "SIMPLE_RADIAL", 1000, 1000, PARAMS))
    for i, n in enumerate(names):
        rec.add_image(Image(i + 1, n, 1, *poses[n]))
    rec, _ = TrackTriangulator.create({}).triangulate(rec, kps, graph, track_labels=labels)
    GeometricBundleOptimizer(OPTIONS, example_setup(rec, 1, 2)).run(rec)
    cov = estimate_ba_covariance(GeometricBundleOptimizer(OPTIONS, example_setup(rec, 1, 2)), rec, scale="posterior")
    s = cov.summary
    print("%d images, %d points, %d residuals, %d parameters; sigma^2 of the residuals %.3f px^2; %.2f ms linearise, %.2f ms factor + "
          "inverse, %.2f ms points" % (len(rec.images), len(rec.points3D), s["num_residuals"], s["num_parameters"], s["factor"],
                                       s["ms_linearise"], s["ms_factor_inverse"], s["ms_points"]))

    q2r = synthetic.qvec_to_rotmat
    rows = []
    for i in rec.reg_image_ids():
        c = cov.pose_cov(i)
        rows.append((np.degrees(np.sqrt(np.trace(c[:3, :3]))), np.sqrt(np.trace(c[3:, 3:])), i))
    print("least certain images (sigma of the rotation in degrees, of the translation in scene units):")
    for rot, tr, i in sorted(rows, reverse=True)[:5]:
        print("  %-14s %.5f deg  %.6f" % (rec.images[i].name, rot, tr))

    # With the whole model free but for the gauge, every point carries the model's common uncertainty against the two anchoring
    # images.  The depth of a point AGAINST THE CAMERAS THAT SEE IT is the triangulation's own: the same problem with every pose
    # held (Sigma_p = inv(V_p)).
    held = example_setup(rec, 1, 2)
    held.constant_tvecs.clear()
    for i in rec.reg_image_ids():
        held.set_constant_pose(i)
    given_cameras = estimate_ba_covariance(GeometricBundleOptimizer(OPTIONS, held), rec, scale="posterior")
    centres = {i: -q2r(im.qvec).T @ im.tvec for i, im in rec.images.items()}
    depth, sigma_depth, total = [], [], []
    for p, pt in rec.points3D.items():
        c, cg = cov.point_cov(p), given_cameras.point_cov(p)
        if not np.all(np.isfinite(c)) or not c.any() or not np.all(np.isfinite(cg)):
            continue
        rays = np.array([pt.xyz - centres[e.image_id] for e in pt.track.elements])
        ray = rays.mean(0) / np.linalg.norm(rays.mean(0))
        depth.append(np.linalg.norm(rays, axis=1).mean())
        sigma_depth.append(np.sqrt(ray @ cg @ ray))
        total.append((np.sqrt(np.trace(c)), p))
    print("least certain points (sigma in scene units, track length):")
    for sg, p in sorted(total, reverse=True)[:5]:
        print("  point %-6d %.6f  %d" % (p, sg, rec.points3D[p].track.length()))
    depth, sigma_depth = np.array(depth), np.array(sigma_depth)
    order = np.argsort(depth)
    near, far = order[:len(order) // 3], order[-(len(order) // 3):]
    rho = np.corrcoef(np.argsort(np.argsort(depth)), np.argsort(np.argsort(sigma_depth)))[0, 1]
    print("sigma of the depth given the cameras: nearest third %.6f, farthest third %.6f (median); rank correlation with the distance %.3f"
          % (np.median(sigma_depth[near]), np.median(sigma_depth[far]), rho))
    assert np.median(sigma_depth[far]) > np.median(sigma_depth[near]) and rho > 0, "depth uncertainty does not grow with distance"


if __name__ == "__main__":
    main()
