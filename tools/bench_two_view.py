#!/usr/bin/env python3
"""Batched two-view geometry (pxr_two_view_geometry) at verification scale: 1000 image pairs of 1000 matches, half of them
outliers.

    python tools/bench_two_view.py --out profiles/two_view_bench.json

Reports the HIP-event time of every kernel (medians and spread over --repeats launches after a warm-up), the wall time of a
call, pairs per second and the samples drawn, and runs the numpy reference of tests/twoview_cases.py on one pair for scale (and
checks that it agrees with the kernels there).  There is no earlier implementation to compare with and no target.  bench.py is
the project's yardstick and is not touched."""
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
    ap.add_argument("--numpy-pairs", type=int, default=1, help="pairs the numpy reference also runs (0: none)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import twoview_cases as tv
    from _bench_runs import stats, timed_runs
    from pixsfm_amd.engine import Context, TwoViewProblem
    # outliers uniform in the image, no minimum distance: the generator's distance test is a Python loop over the outliers
    batch = tv.make_pairs([args.matches] * args.pairs, (1, 2, 8), seed=7, p_outlier=args.outliers, min_outlier_sampson=None)
    ctx = Context(0)
    prob = TwoViewProblem(ctx, batch)
    out, kernels, wall = timed_runs(ctx, prob.estimate, args.repeats)
    res = {k: a.download() for k, a in zip(tv.NAMES, out)}
    status, n_trials = res["status"], res["n_trials"]
    ok = status == 0
    d = np.array([tv.pose_distance(batch["gt_qvec"][i], batch["gt_tvec"][i], res["qvec"][i], res["tvec"][i]) for i in np.flatnonzero(ok)])
    gpu_ms = sum(stats(v)["median"] for v in kernels.values())
    hyp_ms = stats(kernels["hypotheses"])["median"]
    result = {
        "scene": {"pairs": args.pairs, "matches_per_pair": args.matches, "outlier_fraction": args.outliers},
        "kernel_ms": {name: stats(v) for name, v in kernels.items()},
        "kernels_total_ms": gpu_ms, "call_wall_ms": stats(wall),
        "pairs_per_second_kernels": args.pairs / (gpu_ms * 1e-3),
        "samples_drawn": int(n_trials.sum()), "mean_trials": float(n_trials.mean()),
        "samples_per_second_hypotheses_kernel": float(n_trials.sum()) / (hyp_ms * 1e-3),
        "status_counts": np.bincount(status, minlength=4).tolist(),
        "generated_inliers_in_the_masks": float(res["inlier"].astype(bool)[batch["true_inlier"] & np.repeat(ok, args.matches)].mean()),
        "generated_outliers_in_the_masks": float(res["inlier"].astype(bool)[~batch["true_inlier"] & np.repeat(ok, args.matches)].mean()),
        "median_rotation_error_rad": float(np.median(d[:, 0])) if len(d) else None,
    }
    if args.numpy_pairs > 0:
        secs = []
        for p in range(min(args.numpy_pairs, args.pairs)):
            t0 = time.perf_counter()
            ref = tv.reference(tv.single(batch, p))
            secs.append(time.perf_counter() - t0)
            assert ref["status"][0] == status[p] and ref["n_trials"][0] == n_trials[p] and ref["n_inliers"][0] == res["n_inliers"][p]
        result["numpy"] = {"pairs": len(secs), "seconds_per_pair": float(np.median(secs)), "pairs_per_second": 1.0 / float(np.median(secs))}
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
