#!/usr/bin/env python
"""How good is a model?  The synthetic ring scene of examples/reconstruct_from_matches.py with its points on the faces of a cube,
so that there is a surface to scan: the "scan" is a dense regular sampling of those faces.  The matches go through
IncrementalMapper; the model (which has its own frame and scale) is aligned to the known poses with align_reconstructions; then
pose errors with their AUC and the cloud's accuracy / completeness against the scan are printed, before and after the geometric
bundle adjustment.  The mapper runs as a quick pass here, one Levenberg-Marquardt iteration in each of its own adjustments
(--mapper-iterations), so that the adjustment afterwards has work to do and the measures show it; with the mapper's default of 50
its poses are converged already and the adjustment only confirms them (the AUC then moves by 1e-9 percentage points, in either
direction).  A sparse model covers little of a dense scan: the completeness is small by construction.

    python examples/evaluate_reconstruction.py            # needs an MI355X and the built libpixsfm_hip.so
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pixel-perfect-sfm_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from reconstruct_from_matches import PARAMS, adjust, unit                          # noqa: E402
from pixsfm_amd import synthetic                                                   # noqa: E402
from pixsfm_amd.api import (DescriptorMatcher, IncrementalMapper, TwoViewClassifier, align_reconstructions, base,  # noqa: E402
                            build_matching_graph, compare_reconstructions, compute_auc, evaluate_point_cloud)
from pixsfm_amd.api.reconstruction import Camera, Image, Reconstruction            # noqa: E402

TOLERANCES = (0.01, 0.02, 0.05)            # of the cloud, in scene units (the cube has side 2, the cameras are 10 away)
POSE_THRESHOLDS = (0.01, 0.02, 0.05, 0.1)  # of the projection centres


def cube_points(rng, n):
    """n points uniform on the faces of the cube [-1, 1]^3."""
    x = rng.uniform(-1, 1, (n, 3))
    axis = rng.integers(0, 3, n)
    x[np.arange(n), axis] = rng.choice([-1.0, 1.0], n)
    return x


def cube_scan(step):
    """The faces of the cube sampled on a regular grid of the given step."""
    g = np.arange(-1.0, 1.0 + step / 2, step)
    u, v = (a.reshape(-1) for a in np.meshgrid(g, g, indexing="ij"))
    faces = []
    for axis in range(3):
        for side in (-1.0, 1.0):
            f = np.empty((len(u), 3))
            f[:, axis], f[:, (axis + 1) % 3], f[:, (axis + 2) % 3] = side, u, v
            faces.append(f)
    return np.concatenate(faces)


def make_scene(n_images, n_points, views=6, n_extra=40, dim=128, sigma=0.5, desc_noise=0.15, seed=0):
    """As make_scene of reconstruct_from_matches.py, the points on the cube's faces: names, ground-truth poses, keypoints and
    descriptors per image."""
    rng = np.random.default_rng(seed)
    qvec, tvec = synthetic.ring_cameras(n_images, rng=rng)
    names = ["image%02d.jpg" % i for i in range(n_images)]
    X = cube_points(rng, n_points)
    D = unit(rng.standard_normal((n_points, dim)))
    kps, descs = {n: [] for n in names}, {n: [] for n in names}
    for p in range(n_points):
        first = rng.integers(n_images)
        for j in range(min(views, n_images)):
            i = (first + j) % n_images
            kps[names[i]].append(synthetic.project(2, PARAMS, qvec[i], tvec[i], X[p]) + rng.normal(0, sigma, 2))
            descs[names[i]].append(unit(D[p] + desc_noise * rng.standard_normal(dim) / np.sqrt(dim)))
    for n in names:
        for _ in range(n_extra):
            kps[n].append(rng.uniform(0, 1000, 2)); descs[n].append(unit(rng.standard_normal(dim)))
        order = rng.permutation(len(kps[n]))
        kps[n] = np.array(kps[n])[order]
        descs[n] = np.array(descs[n], dtype=np.float32)[order]
    return names, {names[i]: (qvec[i], tvec[i]) for i in range(n_images)}, kps, descs


def evaluate(model, truth, scan, max_error=0.5):
    """Align `model` to the known poses, then pose errors and cloud measures; None where the alignment fails."""
    out = align_reconstructions(model, truth, max_error=max_error)
    if out is None:
        return None
    sim, inliers = out
    cmp_ = compare_reconstructions(model, truth, sim)
    cloud = evaluate_point_cloud(sim.transform_reconstruction(model), scan, tolerances=TOLERANCES, voxel_size=0.05)
    return {"scale": sim.scale, "inliers": int(inliers.sum()), "dt": cmp_["dt"], "dR": cmp_["dR"],
            "auc": compute_auc(cmp_["dt"], POSE_THRESHOLDS), "cloud": cloud}


def run(n_images=12, n_points=400, scan_step=0.005, seed=0, mapper_iterations=1):
    """The core of the example: {"summary", "mapper", "adjusted"} with the evaluations before and after the bundle adjustment;
    mapper_iterations: the iteration limit of the mapper's own adjustments."""
    names, poses, kps, descs = make_scene(n_images, n_points, seed=seed)
    camera = Camera(1, "SIMPLE_RADIAL", 1000, 1000, PARAMS)
    cameras = {n: camera for n in names}
    pairs = [(names[i], names[j]) for i in range(len(names)) for j in range(i + 1, len(names))]
    matches, scores = DescriptorMatcher.create("NN-mutual").match_pairs(descs, pairs)
    matches, scores, geoms = TwoViewClassifier.create({}).classify_pairs(kps, cameras, pairs, matches, scores)
    graph = build_matching_graph(pairs, matches, scores)
    labels = base.compute_track_labels(graph)
    mapper = IncrementalMapper.create({'ba_max_num_iterations': int(mapper_iterations)})
    model, summary = mapper.reconstruct(cameras, kps, graph, pairs, geoms, track_labels=labels)
    result = {"summary": summary, "mapper": None, "adjusted": None}
    if summary["num_reg_images"] < 3:
        return result
    truth = Reconstruction()
    truth.add_camera(camera)
    for i, n in enumerate(names):
        truth.add_image(Image(i + 1, n, 1, *poses[n]))
    scan = cube_scan(scan_step)
    result["mapper"] = evaluate(model, truth, scan)
    id_of = {im.name: i for i, im in model.images.items()}
    adjust(model, *(id_of[n] for n in summary["initial_pair"]))
    result["adjusted"] = evaluate(model, truth, scan)
    result["n_scan"] = len(scan)
    return result


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=12)
    ap.add_argument("--points", type=int, default=400)
    ap.add_argument("--scan-step", type=float, default=0.005)
    ap.add_argument("--mapper-iterations", type=int, default=1, help="iteration limit of the mapper's own adjustments")
    args = ap.parse_args()
    res = run(args.images, args.points, args.scan_step, mapper_iterations=args.mapper_iterations)
    s = res["summary"]
    print("mapper: %s, %d of %d images registered, %d points; scan of %d points" % (s["status"], s["num_reg_images"], args.images,
                                                                                  s["num_points3D"], res.get("n_scan", 0)))
    for title in ("mapper", "adjusted"):
        e = res[title]
        if e is None:
            print("%-9s no alignment" % title)
            continue
        print("%-9s scale %.5f, %d inlier centres, centre error max %.5f, rotation error max %.5f deg" % (
            title, e["scale"], e["inliers"], e["dt"].max(), e["dR"].max()))
        print("          pose AUC @ %s: %s" % (POSE_THRESHOLDS, ["%.2f" % a for a in e["auc"]]))
        c = e["cloud"]
        print("          accuracy @ %s: %s   completeness: %s   voxels (model, scan): %s" % (
            TOLERANCES, ["%.4f" % a for a in c["accuracy"]], ["%.4f" % a for a in c["completeness"]], c["n_voxels"]))


if __name__ == "__main__":
    main()
