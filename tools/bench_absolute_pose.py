#!/usr/bin/env python3
"""Batched absolute pose estimation (pxr_absolute_pose) at localization scale: 1000 queries of 2000 correspondences, half of
them outliers.

    python tools/bench_absolute_pose.py --out profiles/absolute_pose_bench.json

Reports the HIP-event time of every kernel (medians and spread over --repeats launches after a warm-up), the wall time of a
call, queries per second, and hypothesis x correspondence evaluations per second: one evaluation is one pose scored against
one correspondence in the hypothesis loop, counted as samples drawn x poses per sample x correspondences, with the poses per
sample measured on a few queries by the numpy reference of tests/abspose_cases.py (which also gives a numpy time for one
query, for scale).  There is no earlier implementation to compare with and no target.  bench.py is the project's yardstick and
is not touched."""
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
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--correspondences", type=int, default=2000)
    ap.add_argument("--outliers", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--numpy-queries", type=int, default=1, help="queries the numpy reference also runs (0: none)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import abspose_cases as ac
    from _bench_runs import stats, timed_runs
    from pixsfm_amd.engine import AbsolutePoseProblem, Context
    batch = ac.make_queries([args.correspondences] * args.queries, (2, 1, 4), seed=7, p_outlier=args.outliers)
    ctx = Context(0)
    prob = AbsolutePoseProblem(ctx, batch)
    out, kernels, wall = timed_runs(ctx, prob.estimate, args.repeats)
    q, t, status, n_inl, n_trials, inl = (a.download() for a in out[:6])
    ok = status == 0
    d = np.array([ac.pose_distance(batch["gt_qvec"][i], batch["gt_tvec"][i], q[i], t[i]) for i in np.flatnonzero(ok)])
    gpu_ms = sum(stats(v)["median"] for v in kernels.values())
    result = {
        "scene": {"queries": args.queries, "correspondences_per_query": args.correspondences, "outlier_fraction": args.outliers},
        "kernel_ms": {name: stats(v) for name, v in kernels.items()},
        "kernels_total_ms": gpu_ms, "call_wall_ms": stats(wall),
        "queries_per_second_kernels": args.queries / (gpu_ms * 1e-3),
        "status_counts": np.bincount(status, minlength=4).tolist(), "mean_trials": float(n_trials.mean()),
        "inlier_masks_equal_generated": bool(np.array_equal(inl.astype(bool), batch["true_inlier"])),
        "median_rotation_error_rad": float(np.median(d[:, 0])) if len(d) else None,
    }
    if args.numpy_queries > 0:
        poses, secs = [], []
        for qi in range(min(args.numpy_queries, args.queries)):
            one = ac.single(batch, qi)
            n = args.correspondences
            m = int(one["cam_model"][one["query_camera"][0]])
            k = one["cam_params"][one["query_camera"][0]]
            uv, _ = ac.image_to_world(m, k, one["xy"])
            per = [len(ac.p3p(uv[list(s)], one["xyz"][list(s)])) for s in (ac.sample(0, h, n) for h in range(int(n_trials[qi])))]
            poses.append(float(np.mean(per)))
            t0 = time.perf_counter()
            ref = ac.reference(one)
            secs.append(time.perf_counter() - t0)
            assert ref["status"][0] == status[qi] and ref["n_trials"][0] == n_trials[qi] and ref["n_inliers"][0] == n_inl[qi]
        evals = float(n_trials.sum()) * float(np.mean(poses)) * args.correspondences
        hyp_ms = stats(kernels["hypotheses"])["median"]
        result["poses_per_sample"] = float(np.mean(poses))
        result["hypothesis_correspondence_evaluations"] = evals
        result["evaluations_per_second_hypotheses_kernel"] = evals / (hyp_ms * 1e-3)
        result["numpy"] = {"queries": len(secs), "seconds_per_query": float(np.median(secs)),
                           "queries_per_second": 1.0 / float(np.median(secs))}
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
