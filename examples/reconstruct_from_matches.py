#!/usr/bin/env python
"""From descriptors to a model without given poses: DescriptorMatcher -> TwoViewClassifier -> IncrementalMapper -> geometric bundle
adjustment, on a synthetic ring scene (keypoints with descriptors, 0.5 px of keypoint noise, keypoints that nothing else sees).
The same keypoints and tracks then go through the known-pose pipeline (TrackTriangulator with the ground-truth poses + the same
bundle adjustment), and the errors of both against ground truth are printed side by side: poses and points after a similarity
alignment (a model without given poses has its own frame and scale).

    python examples/reconstruct_from_matches.py            # needs an MI355X and the built libpixsfm_hip.so
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pixel-perfect-sfm_amd"))

from pixsfm_amd import synthetic                                                   # noqa: E402
from pixsfm_amd.api import (BundleAdjustmentSetup, DescriptorMatcher, GeometricBundleOptimizer, IncrementalMapper,  # noqa: E402
                            TrackTriangulator, TwoViewClassifier, base, build_matching_graph)
from pixsfm_amd.api.keypoint_adjustment import default_context                    # noqa: E402
from pixsfm_amd.api.reconstruction import Camera, Image, Reconstruction            # noqa: E402
from pixsfm_amd.api.triangulation import mean_reprojection_error                  # noqa: E402

PARAMS = [1200.0, 500.0, 500.0, 0.02]                                              # SIMPLE_RADIAL


def unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def make_scene(n_images, n_points, views=6, n_extra=40, dim=128, sigma=0.5, desc_noise=0.15, seed=0):
    """Names, ground-truth poses, keypoints with descriptors, and the point behind every keypoint (-1: nothing else sees it)."""
    rng = np.random.default_rng(seed)
    qvec, tvec = synthetic.ring_cameras(n_images, rng=rng)
    names = ["image%02d.jpg" % i for i in range(n_images)]
    X = rng.uniform(-1, 1, (n_points, 3))
    D = unit(rng.standard_normal((n_points, dim)))
    kps, descs, owner = {n: [] for n in names}, {n: [] for n in names}, {n: [] for n in names}
    for p in range(n_points):
        first = rng.integers(n_images)
        for j in range(views):                                                     # neighbouring images see the point
            i = (first + j) % n_images
            kps[names[i]].append(synthetic.project(2, PARAMS, qvec[i], tvec[i], X[p]) + rng.normal(0, sigma, 2))
            descs[names[i]].append(unit(D[p] + desc_noise * rng.standard_normal(dim) / np.sqrt(dim)))
            owner[names[i]].append(p)
    for n in names:
        for _ in range(n_extra):
            kps[n].append(rng.uniform(0, 1000, 2)); descs[n].append(unit(rng.standard_normal(dim))); owner[n].append(-1)
        order = rng.permutation(len(owner[n]))
        kps[n] = np.array(kps[n])[order]
        descs[n] = np.array(descs[n], dtype=np.float32)[order]
        owner[n] = np.array(owner[n])[order]
    return names, {names[i]: (qvec[i], tvec[i]) for i in range(n_images)}, kps, descs, owner, X


def similarity(src, dst):
    """(s, R, t) with dst ~ s R src + t in the least-squares sense (Umeyama)."""
    mu_s, mu_d = src.mean(0), dst.mean(0)
    a, b = src - mu_s, dst - mu_d
    U, S, Vt = np.linalg.svd(b.T @ a / len(src))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    R = U @ D @ Vt
    s = np.trace(np.diag(S) @ D) / (a ** 2).sum() * len(src)
    return s, R, mu_d - s * R @ mu_s


def errors(rec, poses, owner, X):
    """(max rotation error in degrees, max centre error, median point error) against ground truth after the alignment."""
    q2r = synthetic.qvec_to_rotmat
    ims = [rec.images[i] for i in sorted(rec.images)]
    c_est = np.array([-q2r(im.qvec).T @ im.tvec for im in ims])
    c_gt = np.array([-q2r(poses[im.name][0]).T @ poses[im.name][1] for im in ims])
    s, R, t = similarity(c_est, c_gt)
    rot = [np.degrees(np.arccos(np.clip((np.trace(q2r(im.qvec) @ R.T @ q2r(poses[im.name][0]).T) - 1) / 2, -1, 1))) for im in ims]
    cen = np.linalg.norm((s * (R @ c_est.T)).T + t - c_gt, axis=1)
    pts = []
    for p in rec.points3D.values():
        e = p.track.elements[0]
        point = owner[rec.images[e.image_id].name][e.point2D_idx]
        if point >= 0:
            pts.append(np.linalg.norm(s * R @ p.xyz + t - X[point]))
    return max(rot), cen.max(), float(np.median(pts))


def adjust(rec, first_id, second_id):
    """Geometric bundle adjustment, intrinsics constant, the gauge fixed on two images."""
    setup = BundleAdjustmentSetup()
    setup.add_images(rec.reg_image_ids())
    setup.set_constant_pose(first_id)
    setup.set_constant_tvec(second_id, [int(np.argmax(np.abs(rec.images[second_id].tvec)))])
    for c in rec.cameras:
        setup.set_constant_camera(c)
    GeometricBundleOptimizer({'loss': {'name': 'trivial', 'params': []}, 'print_summary': False}, setup).run(rec)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=12)
    ap.add_argument("--points", type=int, default=400)
    args = ap.parse_args()
    names, poses, kps, descs, owner, X = make_scene(args.images, args.points)
    camera = Camera(1, "SIMPLE_RADIAL", 1000, 1000, PARAMS)
    cameras = {n: camera for n in names}
    pairs = [(names[i], names[j]) for i in range(len(names)) for j in range(i + 1, len(names))]
    matches, scores = DescriptorMatcher.create("NN-mutual").match_pairs(descs, pairs)
    matches, scores, geoms = TwoViewClassifier.create({}).classify_pairs(kps, cameras, pairs, matches, scores)
    print("%d images, %d pairs, %d with a geometry: %s" % (len(names), len(pairs), sum(bool(g["success"]) for g in geoms),
                                                          {c: sum(g["config"] == c for g in geoms) for c in sorted({g["config"] for g in geoms})}))
    graph = build_matching_graph(pairs, matches, scores)
    labels = base.compute_track_labels(graph)

    model, summary = IncrementalMapper.create({}).reconstruct(cameras, kps, graph, pairs, geoms, track_labels=labels)
    print("mapper: %s, initial pair %s, %d of %d images registered in %d rounds %s, %d points"
          % (summary["status"], summary["initial_pair"], summary["num_reg_images"], len(names), len(summary["rounds"]),
             [(r["candidates"], r["registered"]) for r in summary["rounds"]], summary["num_points3D"]))
    if summary["num_reg_images"] < 3:
        return
    id_of = {im.name: i for i, im in model.images.items()}
    first, second = (id_of[n] for n in summary["initial_pair"])
    adjust(model, first, second)

    known = Reconstruction()
    known.add_camera(camera)
    for i, im in model.images.items():                                             # the same images, ground-truth poses
        known.add_image(Image(i, im.name, 1, *poses[im.name]))
    reference, _ = TrackTriangulator.create({}).triangulate(known, kps, graph, track_labels=labels)
    adjust(reference, first, second)

    print("%-22s %10s %14s %14s %14s %8s" % ("", "reproj px", "rotation deg", "centre", "median point", "points"))
    for title, rec in (("mapper + BA", model), ("known poses + BA", reference)):
        rot, cen, pts = errors(rec, poses, owner, X)
        print("%-22s %10.4f %14.5f %14.5f %14.5f %8d" % (title, mean_reprojection_error(default_context(), rec), rot, cen, pts,
                                                         len(rec.points3D)))


if __name__ == "__main__":
    main()
