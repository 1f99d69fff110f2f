#!/usr/bin/env python
"""Descriptors and poses in, a refined model and a query pose out, without leaving the library: synthetic posed images whose
keypoints carry descriptors (a random unit vector per 3D point plus per-observation noise, renormalised) and some unmatched
keypoints -> DescriptorMatcher (in place of hloc.match_features + read_matches_hloc) -> build_matching_graph -> track labels ->
TrackTriangulator -> geometric bundle adjustment.  Then a held-out image: its descriptors matched against the map's images ->
pairs_2d3d_from_matches -> absolute_pose_estimation.

    python examples/match_triangulate_refine.py            # needs an MI355X and the built libpixsfm_hip.so
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pixel-perfect-sfm_amd"))

from pixsfm_amd import synthetic                                                   # noqa: E402
from pixsfm_amd.api import (BundleAdjuster, DescriptorMatcher, TrackTriangulator, absolute_pose_estimation, base,  # noqa: E402
                            build_matching_graph, pairs_2d3d_from_matches)
from pixsfm_amd.api.reconstruction import Camera, Image, Reconstruction            # noqa: E402

PARAMS = [1200.0, 500.0, 500.0, 0.02]                                              # SIMPLE_RADIAL


def unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def make_scene(n_images=10, n_points=400, views=6, n_extra=40, dim=128, sigma=0.5, desc_noise=0.15, seed=0):
    """Image 0 is held out (the query); the others are the map.  Returns the map's Reconstruction (poses only), keypoints and
    descriptors of every image, the point behind every keypoint (-1: an unmatched keypoint), the scene points and the poses."""
    rng = np.random.default_rng(seed)
    qvec, tvec = synthetic.ring_cameras(n_images, rng=rng)
    names = ["image%02d.jpg" % i for i in range(n_images)]
    rec = Reconstruction()
    rec.add_camera(Camera(1, "SIMPLE_RADIAL", 1000, 1000, PARAMS))
    for i in range(1, n_images):
        rec.add_image(Image(i, names[i], 1, qvec[i], tvec[i]))
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
    for n in names:                                                                # keypoints nothing else sees
        for _ in range(n_extra):
            kps[n].append(rng.uniform(0, 1000, 2)); descs[n].append(unit(rng.standard_normal(dim))); owner[n].append(-1)
        order = rng.permutation(len(owner[n]))
        kps[n] = np.array(kps[n])[order]
        descs[n] = np.array(descs[n], dtype=np.float32)[order]
        owner[n] = np.array(owner[n])[order]
    return rec, names, kps, descs, owner, X, qvec, tvec


def pose_error(q, t, gt_q, gt_t):
    R0, R1 = synthetic.qvec_to_rotmat(gt_q), synthetic.qvec_to_rotmat(q)
    ang = np.arccos(np.clip((np.trace(R0.T @ R1) - 1) / 2, -1, 1))
    return np.rad2deg(ang), np.linalg.norm(R1.T @ t - R0.T @ gt_t)


def main():
    rec, names, kps, descs, owner, X, qvec, tvec = make_scene()
    query, db = names[0], names[1:]
    matcher = DescriptorMatcher.create("NN-ratio")

    # ---- the map: match every pair of map images in one launch, build the graph, label the tracks
    pairs = [(db[i], db[j]) for i in range(len(db)) for j in range(i + 1, len(db))]
    matches, scores = matcher.match_pairs(descs, pairs)
    right = sum(int((owner[a][m[:, 0].astype(int)] == owner[b][m[:, 1].astype(int)]).sum()) for (a, b), m in zip(pairs, matches))
    print("matching: %d pairs in %d launch, %d matches, %d of them between keypoints of one point"
          % (len(pairs), matcher.num_launches, sum(len(m) for m in matches), right))
    graph = build_matching_graph(pairs, matches, scores)
    labels = base.compute_track_labels(graph)
    generated = {}
    for n in db:
        for k, p in enumerate(owner[n]):
            if p >= 0:
                generated.setdefault(int(p), set()).add((n, k))
    generated = {p: t for p, t in generated.items() if len(t) >= 2}
    found = {}
    for node, lab in zip(graph.nodes, labels):
        found.setdefault(lab, set()).add((graph.image_id_to_name[node.image_id], int(node.feature_idx)))
    found = {frozenset(t) for t in found.values()}
    print("tracks: %d generated, %d recovered exactly" % (len(generated), sum(frozenset(t) in found for t in generated.values())))

    # ---- triangulation and geometric bundle adjustment
    db_kps = {n: kps[n] for n in db}
    model, summary = TrackTriangulator.create({}).triangulate(rec, db_kps, graph, track_labels=labels)
    print("triangulation: %d tracks -> %d points, mean reprojection error %.3f px"
          % (summary["num_tracks"], summary["num_points3D"], summary["mean_reprojection_error"]))

    def errors(m):
        P = np.array([m.points3D[i].xyz for i in m.point3D_ids()])
        return np.sqrt(((P[:, None, :] - X[None, :, :]) ** 2).sum(-1)).min(1)
    e0 = errors(model)
    out = BundleAdjuster.create({"strategy": "geometric"}).refine(model)
    e1 = errors(model)
    print("point error: median %.5f after triangulation, %.5f after geometric BA (%s)" % (np.median(e0), np.median(e1), out["summary"].BriefReport()))

    # ---- the held-out image: matches against every map image -> 2D-3D pairs -> pose
    q_pairs = [(query, n) for n in db]
    q_matches, _ = matcher.match_pairs(descs, q_pairs)
    image_of = {im.name: im for im in model.images.values()}
    point_ids = {n: np.array([p.point3D_id for p in image_of[n].points2D]) for n in db}
    p2d, p3d = pairs_2d3d_from_matches([(n, m) for (_, n), m in zip(q_pairs, q_matches)], point_ids)
    print("query: %d keypoints, %d matches against %d map images -> %d 2D-3D pairs" % (len(kps[query]), sum(len(m) for m in q_matches), len(db), len(p2d)))
    pose = absolute_pose_estimation(kps[query][p2d], np.array([model.points3D[int(i)].xyz for i in p3d]),
                                    Camera(1, "SIMPLE_RADIAL", 1000, 1000, PARAMS))
    if not pose["success"]:
        print("query pose: failed")
        return
    rot, centre = pose_error(pose["qvec"], pose["tvec"], qvec[0], tvec[0])
    print("query pose: %d inliers, rotation error %.5f deg, camera centre error %.6f" % (pose["num_inliers"], rot, centre))


if __name__ == "__main__":
    main()
