#!/usr/bin/env python
"""What geometric verification is for: the scene of examples/match_triangulate_refine.py with REPEATED STRUCTURE -- a share of
the 3D points carries the descriptor of another point, as windows of one facade do.  Mutual nearest neighbours then join
keypoints of different points; one such match merges two tracks in the match graph, and the triangulator throws the merged track
away.  The script matches all pairs, then builds graph, track labels and points twice: from the raw matches, and from the matches
that TwoViewVerifier keeps (five-point estimation per pair; with --known-poses, classification under the map's poses as hloc's
triangulation does).  It prints wrong matches, merged tracks and triangulated points for both.

    python examples/match_verify_triangulate.py            # needs an MI355X and the built libpixsfm_hip.so
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pixel-perfect-sfm_amd"))

from pixsfm_amd import synthetic                                                   # noqa: E402
from pixsfm_amd.api import DescriptorMatcher, TrackTriangulator, TwoViewVerifier, base, build_matching_graph  # noqa: E402
from pixsfm_amd.api.reconstruction import Camera, Image, Reconstruction            # noqa: E402

PARAMS = [1200.0, 500.0, 500.0, 0.02]                                              # SIMPLE_RADIAL


def unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def make_scene(n_images=9, n_points=400, views=6, n_extra=40, dim=128, sigma=0.5, desc_noise=0.15, repeated=0.2, seed=0):
    """Posed images, keypoints with descriptors, the point behind every keypoint (-1: an unmatched keypoint).  A share `repeated`
    of the points takes the descriptor of another point."""
    rng = np.random.default_rng(seed)
    qvec, tvec = synthetic.ring_cameras(n_images, rng=rng)
    names = ["image%02d.jpg" % i for i in range(n_images)]
    camera = Camera(1, "SIMPLE_RADIAL", 1000, 1000, PARAMS)
    rec = Reconstruction()
    rec.add_camera(camera)
    for i in range(n_images):
        rec.add_image(Image(i + 1, names[i], 1, qvec[i], tvec[i]))
    X = rng.uniform(-1, 1, (n_points, 3))
    D = unit(rng.standard_normal((n_points, dim)))
    twins = rng.permutation(n_points)[:int(repeated * n_points)]
    for p in twins:
        D[p] = D[(p + 1 + rng.integers(n_points - 1)) % n_points]
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
    poses = {names[i]: (qvec[i], tvec[i]) for i in range(n_images)}
    return rec, camera, names, kps, descs, owner, poses, len(twins)


def count(owner, pairs, matches, scores):
    """Graph and track labels of one set of matches: (matches, wrong matches, tracks, merged tracks, graph, labels).  A match is
    wrong when its keypoints belong to different points; a track is merged when it holds keypoints of two or more points."""
    total = sum(len(m) for m in matches)
    wrong = sum(int((owner[a][m[:, 0].astype(int)] != owner[b][m[:, 1].astype(int)]).sum()) for (a, b), m in zip(pairs, matches))
    graph = build_matching_graph(pairs, matches, scores)
    labels = base.compute_track_labels(graph)
    tracks = {}
    for node, lab in zip(graph.nodes, labels):
        tracks.setdefault(lab, set()).add(int(owner[graph.image_id_to_name[node.image_id]][int(node.feature_idx)]))
    merged = sum(len(points - {-1}) >= 2 for points in tracks.values())
    return total, wrong, len(tracks), merged, graph, labels


def report(title, rec, names, kps, owner, pairs, matches, scores):
    """count() and the triangulation of the tracks; returns (wrong matches, merged tracks)."""
    total, wrong, n_tracks, merged, graph, labels = count(owner, pairs, matches, scores)
    model, summary = TrackTriangulator.create({}).triangulate(rec, {n: kps[n] for n in names}, graph, track_labels=labels)
    print("%-22s %6d matches, %4d wrong; %4d tracks, %3d of them merged (keypoints of two or more points); %4d points triangulated"
          % (title + ":", total, wrong, n_tracks, merged, summary["num_points3D"]))
    return wrong, merged


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeated", type=float, default=0.2, help="share of the points that carry another point's descriptor")
    ap.add_argument("--known-poses", action="store_true", help="verify against the map's poses instead of estimating one per pair")
    args = ap.parse_args()
    rec, camera, names, kps, descs, owner, poses, n_twins = make_scene(repeated=args.repeated)
    pairs = [(names[i], names[j]) for i in range(len(names)) for j in range(i + 1, len(names))]
    matches, scores = DescriptorMatcher.create("NN-mutual").match_pairs(descs, pairs)
    print("%d images, %d pairs, %d of 400 points with another point's descriptor" % (len(names), len(pairs), n_twins))
    raw = report("without the verifier", rec, names, kps, owner, pairs, matches, scores)
    verifier = TwoViewVerifier.create({})
    v_matches, v_scores, geoms = verifier.verify_pairs(kps, {n: camera for n in names}, pairs, matches, scores,
                                                       poses=poses if args.known_poses else None)
    print("verifier: %d of %d pairs have a geometry (%s)" % (sum(g["success"] for g in geoms), len(pairs),
                                                            "poses given" if args.known_poses else "five-point estimation"))
    ver = report("with the verifier", rec, names, kps, owner, pairs, v_matches, v_scores)
    print("wrong matches %d -> %d, merged tracks %d -> %d" % (raw[0], ver[0], raw[1], ver[1]))


if __name__ == "__main__":
    main()
