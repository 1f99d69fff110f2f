#!/usr/bin/env python3
"""Batched fundamental-matrix estimation (pxr_fundamental) at verification scale, next to the essential-matrix and homography
estimators (pxr_two_view_geometry, pxr_homography) on the batch of tools/bench_homography.py: 1000 image pairs of 1000 matches,
half of them outliers, a third each in front of a plane, rotation-only and general.

    python tools/bench_fundamental.py --out profiles/fundamental_bench.json

Reports for the three estimators the HIP-event time of every kernel (medians and spread over --repeats launches after a warm-up),
the wall time of a call, pairs per second and the samples drawn, per kind of pair what the fundamental-matrix estimator ends at,
and runs the numpy reference of tests/fundamental_cases.py on one pair of every kind for scale (and checks that it agrees with the
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--matches", type=int, default=1000)
    ap.add_argument("--outliers", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--numpy-pairs", type=int, default=3, help="pairs the numpy reference also runs: the first of every kind (0: none)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import fundamental_cases as fc
    import homography_cases as hc
    import twoview_cases as tv
    from _bench_runs import timed_runs
    from bench_homography import summary
    from pixsfm_amd.engine import Context, FundamentalProblem, HomographyProblem, TwoViewProblem
    kinds = [("planar", "rotation", "general")[p % 3] for p in range(args.pairs)]
    # the batch of bench_homography.py: outliers uniform in the image, no minimum distance
    batch = hc.make_pairs(kinds, [args.matches] * args.pairs, (1, 2, 8), seed=7, p_outlier=args.outliers, min_outlier=None)
    kind = np.array(kinds)
    ctx = Context(0)
    prob_e = TwoViewProblem(ctx, batch)
    prob_h, prob_f = HomographyProblem(ctx, prob_e), FundamentalProblem(ctx, prob_e)
    out_f, kern_f, wall_f = timed_runs(ctx, prob_f.estimate, args.repeats)
    out_h, kern_h, wall_h = timed_runs(ctx, prob_h.estimate, args.repeats)
    out_e, kern_e, wall_e = timed_runs(ctx, prob_e.estimate, args.repeats)
    res = {k: a.download() for k, a in zip(fc.NAMES, out_f)}
    res_h = {k: a.download() for k, a in zip(hc.NAMES, out_h)}
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
            "median_n_E_over_n_F": float(np.median(res_e["n_inliers"][sel] / np.maximum(res["n_inliers"][sel], 1))),
            "generated_inliers_in_the_masks": float(mask[truth & rows].mean()) if rows.any() else None,
            "generated_outliers_in_the_masks": float(mask[~truth & rows].mean()) if rows.any() else None,
        }
    result = {
        "scene": {"pairs": args.pairs, "matches_per_pair": args.matches, "outlier_fraction": args.outliers, "kinds": "planar / rotation / general in turn"},
        "fundamental": summary(args.pairs, kern_f, wall_f, res["n_trials"], res["status"]),
        "two_view_geometry": summary(args.pairs, kern_e, wall_e, res_e["n_trials"], res_e["status"]),
        "homography": summary(args.pairs, kern_h, wall_h, res_h["n_trials"], res_h["status"]),
        "fundamental_by_kind": per_kind,
    }
    if args.numpy_pairs > 0:
        secs, agrees = {}, []
        for p in range(min(args.numpy_pairs, args.pairs, 3)):
            t0 = time.perf_counter()
            ref = fc.reference(fc.single(batch, p))
            secs[kinds[p]] = time.perf_counter() - t0
            agrees.append(bool(ref["status"][0] == res["status"][p] and ref["n_trials"][0] == res["n_trials"][p] and
                               ref["n_inliers"][0] == res["n_inliers"][p]))
        mean = float(np.mean(list(secs.values())))
        result["numpy"] = {"seconds_per_pair_by_kind": secs, "seconds_per_pair": mean, "pairs_per_second": 1.0 / mean,
                           "agrees_with_the_kernels": agrees}
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    assert all(result.get("numpy", {}).get("agrees_with_the_kernels", [])), "the numpy reference and the kernels disagree"


if __name__ == "__main__":
    main()
