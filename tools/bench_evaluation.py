#!/usr/bin/env python3
"""Cloud evaluation (pxr_cloud_nearest, pxr_cloud_voxel_fractions) at the size of a laser scan: a synthetic scan of 2e7 points on
a few planes and a sphere inside a 40 m box, a model of 2e5 points near those surfaces, tolerances 1 / 2 / 5 cm, voxels of 1 cm.

    python tools/bench_evaluation.py --out profiles/evaluation_bench.json

Both directions (accuracy: the model queries the scan; completeness: the scan queries the model) run once untimed, then --repeats
times; reported are the medians of the HIP-event times of the kernels (the *_timed entry points), the candidates tested per query
(counted on the host from the occupancy of the 27 cells around a query, on a sample of the queries; two cells that share a
bucket add a few more), the bytes the query kernel moves against the 5.5 TB/s the microarchitecture guide measures for gathered
whole rows, and for scale scipy.spatial.cKDTree.query(distance_upper_bound, workers=16) on the same arrays with its agreement.
Nobody fixed a target for any of this.  bench.py is the project's yardstick and is not touched."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pixel-perfect-sfm_amd"))

GATHER_BYTES_PER_SECOND = 5.5e12
TOLERANCES = (0.01, 0.02, 0.05)


def stats(values):
    v = sorted(float(x) for x in values)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "all": [round(x, 4) for x in values]}


def surfaces(rng, n, box=40.0):
    """n points on four planes and a sphere inside a box of the given side."""
    half = box / 2
    part = rng.integers(0, 5, n)
    x = rng.uniform(-half, half, (n, 3))
    x[part == 0, 2] = -half + 1.0                                      # floor
    x[part == 1, 0] = -half + 2.0                                      # two walls
    x[part == 2, 1] = half - 3.0
    x[part == 3, 2] = 0.25 * x[part == 3, 0] + 5.0                     # a slanted roof
    s = part == 4
    d = rng.standard_normal((int(s.sum()), 3))
    x[s] = 6.0 * d / np.linalg.norm(d, axis=1, keepdims=True) + np.array([3.0, -2.0, 1.0])
    return x


def cells_tested(ref, query, max_dist, sample, rng):
    """Mean and maximum number of reference points in the 27 cells around a query (the library's cell side), over a sample."""
    h = max_dist * (1.0 + 2.0 ** -20)
    pack = lambda c: ((c[:, 0] + (1 << 20)) << 42) | ((c[:, 1] + (1 << 20)) << 21) | (c[:, 2] + (1 << 20))   # noqa: E731
    keys, counts = np.unique(pack(np.floor(ref / h).astype(np.int64)), return_counts=True)
    q = query[rng.choice(len(query), min(sample, len(query)), replace=False)]
    cq = np.floor(q / h).astype(np.int64)
    tested = np.zeros(len(q), np.int64)
    for n in range(27):
        k = pack(cq + np.array([n % 3 - 1, (n // 3) % 3 - 1, n // 9 - 1]))
        at = np.minimum(np.searchsorted(keys, k), len(keys) - 1)
        tested += np.where(keys[at] == k, counts[at], 0)
    return float(tested.mean()), int(tested.max()), int(counts.max()), len(keys)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scan", type=int, default=20_000_000)
    ap.add_argument("--model", type=int, default=200_000)
    ap.add_argument("--voxel", type=float, default=0.01)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-kdtree", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from pixsfm_amd.engine import Context, cloud_nearest, cloud_voxel_fractions
    rng = np.random.default_rng(0)
    scan = surfaces(rng, args.scan)
    model = scan[rng.choice(args.scan, args.model, replace=False)] + rng.normal(0, 0.015, (args.model, 3))
    reach = max(TOLERANCES)
    ctx = Context(0)
    d_scan, d_model = ctx.to_device(scan, np.float64), ctx.to_device(model, np.float64)
    directions = {"accuracy": (d_scan, d_model, scan, model), "completeness": (d_model, d_scan, model, scan)}
    result = {"scene": {"scan_points": args.scan, "model_points": args.model, "box_m": 40.0, "tolerances": TOLERANCES, "max_dist": reach,
                        "voxel_size": args.voxel, "model_noise_sigma": 0.015}, "repeats": args.repeats}
    outputs = {}
    for name, (d_ref, d_query, ref, query) in directions.items():
        index, dist2 = cloud_nearest(ctx, d_ref, d_query, reach)             # untimed settle (allocates the workspace)
        cloud_voxel_fractions(ctx, d_query, dist2, args.voxel, TOLERANCES)
        kernels, wall = {}, []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            index, dist2, ms = cloud_nearest(ctx, d_ref, d_query, reach, timed=True)
            frac, n_vox, ms2 = cloud_voxel_fractions(ctx, d_query, dist2, args.voxel, TOLERANCES, timed=True)
            wall.append(1e3 * (time.perf_counter() - t0))
            for k, v in list(ms.items()) + list(ms2.items()):
                kernels.setdefault(k, []).append(v)
        med = {k: stats(v)["median"] for k, v in kernels.items()}
        mean_t, max_t, max_cell, n_cells = cells_tested(ref, query, reach, 200_000, rng)
        nq, nr = len(query), len(ref)
        query_bytes = nq * (24.0 + 12.0 + 27 * 8.0 + mean_t * 28.0)
        outputs[name] = (index.download(), dist2.download())
        result[name] = {
            "n_ref": nr, "n_query": nq, "kernel_ms": {k: stats(v) for k, v in kernels.items()}, "call_wall_ms": stats(wall),
            "fractions": [float(x) for x in frac], "n_voxels": n_vox, "queries_with_a_neighbour": int((outputs[name][0] >= 0).sum()),
            "candidates_tested_per_query_mean": mean_t, "candidates_tested_per_query_max": max_t, "largest_cell": max_cell,
            "occupied_cells": n_cells, "queries_per_second": nq / (med["query"] * 1e-3),
            "query_bytes": query_bytes, "query_bytes_per_second": query_bytes / (med["query"] * 1e-3),
            "query_fraction_of_gather_rate": query_bytes / (med["query"] * 1e-3) / GATHER_BYTES_PER_SECOND,
            "grid_bytes_per_second": nr * (2 * 24.0 + 28.0 + 8.0) / (med["grid"] * 1e-3),
        }
    if not args.no_kdtree:
        from scipy.spatial import cKDTree
        result["ckdtree"] = {}
        for name, (_, _, ref, query) in directions.items():
            t0 = time.perf_counter()
            tree = cKDTree(ref)
            t1 = time.perf_counter()
            d, j = tree.query(query, distance_upper_bound=reach, workers=16)
            t2 = time.perf_counter()
            index, dist2 = outputs[name]
            found = np.isfinite(d)
            both = found & (index >= 0)
            ours_ms = sum(result[name]["kernel_ms"][k]["median"] for k in ("grid", "query"))
            result["ckdtree"][name] = {
                "build_ms": 1e3 * (t1 - t0), "query_ms": 1e3 * (t2 - t1), "found_differs_from_ours": int((found != (index >= 0)).sum()),
                "index_differs_from_ours": int((j[both] != index[both]).sum()),
                "max_distance_difference": float(np.abs(np.sqrt(dist2[both]) - d[both]).max()) if both.any() else 0.0,
                "build_plus_query_over_our_kernels": 1e3 * (t2 - t0) / ours_ms, "query_over_our_query": 1e3 * (t2 - t1) / result[name]["kernel_ms"]["query"]["median"]}
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
