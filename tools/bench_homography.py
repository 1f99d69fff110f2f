#!/usr/bin/env python3
"""Batched homography estimation (pxr_homography) at verification scale, next to the essential-matrix estimator
(pxr_two_view_geometry) on the same batch: 1000 image pairs of 1000 matches, half of them outliers, a third each in front of a
plane, rotation-only and general.

    python tools/bench_homography.py --out profiles/homography_bench.json

Reports for both estimators the HIP-event time of every kernel (medians and spread over --repeats launches after a warm-up),
the wall time of a call, pairs per second and the samples drawn, per kind of pair what the homography estimator ends at, and
runs the numpy reference of tests/homography_cases.py on one pair of every kind for scale (and checks that it agrees with the
kernels there).  There is no earlier implementation to compare with and no target.  bench.py is the project's yardstick and is
not touched."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pixel-perfect-sfm_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


from _bench_runs import stats, timed_runs  # noqa: E402


def summary(n_pairs, kernels, wall, n_trials, status):
    gpu_ms = sum(stats(v)["median"] for v in kernels.values())
    hyp_ms = stats(kernels["hypotheses"])["median"]
    return {"kernel_ms": {name: stats(v) for name, v in kernels.items()}, "kernels_total_ms": gpu_ms, "call_wall_ms": stats(wall),
            "pairs_per_second_kernels": n_pairs / (gpu_ms * 1e-3), "samples_drawn": int(n_trials.sum()), "mean_trials": float(n_trials.mean()),
            "samples_per_second_hypotheses_kernel": float(n_trials.sum()) / (hyp_ms * 1e-3),
            "status_counts": np.bincount(status, minlength=4).tolist()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--matches", type=int, default=1000)
    ap.add_argument("--outliers", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--numpy-pairs", type=int, default=3, help="pairs the numpy reference also runs: the first of every kind (0: none)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import homography_cases as hc
    import twoview_cases as tv
    from pixsfm_amd.engine import Context, HomographyProblem, TwoViewProblem
    kinds = [("planar", "rotation", "general")[p % 3] for p in range(args.pairs)]
    # outliers uniform in the image, no minimum distance: the generators' distance test is a Python loop over the outliers
    batch = hc.make_pairs(kinds, [args.matches] * args.pairs, (1, 2, 8), seed=7, p_outlier=args.outliers, min_outlier=None)
    kind = np.array(kinds)
    ctx = Context(0)
    prob_e = TwoViewProblem(ctx, batch)
    prob_h = HomographyProblem(ctx, prob_e)
    out_h, kern_h, wall_h = timed_runs(ctx, prob_h.estimate, args.repeats)
    out_e, kern_e, wall_e = timed_runs(ctx, prob_e.estimate, args.repeats)
    res = {k: a.download() for k, a in zip(hc.NAMES, out_h)}
    res_e = {k: a.download() for k, a in zip(tv.NAMES, out_e)}
    ok = res["status"] == 0
    mask, truth = res["inlier"].astype(bool), batch["true_inlier"]
    per_kind = {}
    for name in ("planar", "rotation", "general"):
        sel = kind == name
        rows = np.repeat(sel & ok, args.matches)
        per_kind[name] = {
            "pairs": int(sel.sum()), "status_counts": np.bincount(res["status"][sel], minlength=4).tolist(),
            "mean_trials": float(res["n_trials"][sel].mean()),
            "median_n_H_over_n_E": float(np.median(res["n_inliers"][sel] / np.maximum(res_e["n_inliers"][sel], 1))),
            "median_n_R_over_n_H": float(np.median(res["n_rot_inliers"][sel & ok] / res["n_inliers"][sel & ok])) if (sel & ok).any() else None,
            "generated_inliers_in_the_masks": float(mask[truth & rows].mean()) if rows.any() else None,
            "generated_outliers_in_the_masks": float(mask[~truth & rows].mean()) if rows.any() else None,
        }
    result = {
        "scene": {"pairs": args.pairs, "matches_per_pair": args.matches, "outlier_fraction": args.outliers, "kinds": "planar / rotation / general in turn"},
        "homography": summary(args.pairs, kern_h, wall_h, res["n_trials"], res["status"]),
        "two_view_geometry": summary(args.pairs, kern_e, wall_e, res_e["n_trials"], res_e["status"]),
        "homography_by_kind": per_kind,
    }
    if args.numpy_pairs > 0:
        secs = {}
        for p in range(min(args.numpy_pairs, args.pairs, 3)):
            t0 = time.perf_counter()
            ref = hc.reference(hc.single(batch, p))
            secs[kinds[p]] = time.perf_counter() - t0
            assert ref["status"][0] == res["status"][p] and ref["n_trials"][0] == res["n_trials"][p]
            assert ref["n_inliers"][0] == res["n_inliers"][p] and ref["n_rot_inliers"][0] == res["n_rot_inliers"][p]
        mean = float(np.mean(list(secs.values())))
        result["numpy"] = {"seconds_per_pair_by_kind": secs, "seconds_per_pair": mean, "pairs_per_second": 1.0 / mean}
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
