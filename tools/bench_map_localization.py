#!/usr/bin/env python3
"""The kernels of batched map localization at scale (csrc/pxr_localize.hip).

    python tools/bench_map_localization.py --out profiles/map_localization_bench.json

Part 1 (covisibility: --images 1000 map images, --observations 1000000 in tracks of five images 1, 3 or 10 apart on a ring):
pxr_covisibility_timed with --num-matched 20 partners, per kernel; for scale the same counts as numpy's B^t B (B = tracks x images
incidence, float32, in blocks of 20 000 tracks, diagonal dropped), which must agree exactly.
Part 2 (the gather: --queries 1000 x --retrieved 20 database images x --keypoints 2000 per image; 60 % of the query keypoints
matched per pair, half of the database keypoints with a point): pxr_covisibility_clusters_timed on the lists and
pxr_localization_pairs_timed with one problem per query, per kernel; for scale the host loop api.matching.pairs_2d3d_from_matches on
--host-queries 5 of the queries (matches downloaded first, as that route needs them), extrapolated to all.
One process, one untimed warm-up run per entry point, then the median of --repeats runs of the HIP-event times of the *_timed
entry points.  Nobody has fixed a target for these numbers: this writes down what is measured."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("", "tests", "oracle", "pixel-perfect-sfm_amd"):
    sys.path.insert(0, os.path.join(ROOT, p))


def stats(values):
    v = sorted(float(x) for x in values)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def timed_runs(run, read, repeats):
    run()                                                                                         # warm-up
    rows = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        run()
        rows.append(dict(read(), wall=1e3 * (time.perf_counter() - t0)))
    return {k: stats([r[k] for r in rows]) for k in rows[0]}


def covisibility_part(ctx, args):
    from pixsfm_amd.engine import CovisibilityGraph
    n, nb = args.images, 5
    n_tracks = args.observations // nb
    rng = np.random.default_rng(0)
    first = rng.integers(0, n, n_tracks)
    strides = np.array([1, 3, 10])[rng.integers(0, 3, n_tracks)]
    obs_image = ((first[:, None] + strides[:, None] * np.arange(nb)[None]) % n).astype(np.int32)
    offsets = np.arange(0, n_tracks * nb + 1, nb)
    graph = CovisibilityGraph(ctx, offsets, obs_image.reshape(-1), n)
    ms = timed_runs(lambda: graph.topk(args.num_matched, timed=True), lambda: graph.kernel_ms, args.repeats)
    t0 = time.perf_counter()
    count = np.zeros((n, n), np.float64)
    for lo in range(0, n_tracks, 20000):
        block = obs_image[lo:lo + 20000]
        B = np.zeros((len(block), n), np.float32)
        np.add.at(B, (np.repeat(np.arange(len(block)), nb), block.reshape(-1)), 1.0)
        count += B.T @ B
    np.fill_diagonal(count, 0)
    numpy_ms = 1e3 * (time.perf_counter() - t0)
    assert np.array_equal(graph.counts(), count.astype(np.int32)), "the counts differ from numpy's"
    pairs = float(n_tracks) * nb * (nb - 1)
    return {"images": n, "observations": int(n_tracks * nb), "tracks": int(n_tracks), "num_matched": args.num_matched, "kernel_ms": ms,
            "ordered_pairs": pairs, "atomic_adds_per_ns": pairs / (ms["count"]["median"] * 1e6), "numpy_BtB_ms": numpy_ms,
            "mean_partners": float((count > 0).sum(1).mean())}, graph


def gather_part(ctx, args, graph):
    from pixsfm_amd.api import pairs_2d3d_from_matches
    from pixsfm_amd.engine import LocalizationPairs, MatchProblem
    Q, R, K, n_db = args.queries, args.retrieved, args.keypoints, graph.n_images
    rng = np.random.default_rng(1)
    n_set = Q + n_db
    image_offsets = np.arange(0, (n_set + 1) * K, K, dtype=np.int64)
    # a query's list: R neighbours of a random map image (covisible among themselves) -- half of them from a second spot
    spot = rng.integers(0, n_db, (Q, 2))
    ret = ((spot[:, [0] * (R // 2) + [1] * (R - R // 2)] + np.tile(np.arange(R), (Q, 1))) % n_db).astype(np.int32)
    pairs = np.stack([np.repeat(np.arange(Q), R), Q + ret.reshape(-1)], 1).astype(np.int32)
    match = MatchProblem(ctx, np.zeros((n_set * K, 1), np.float32), pairs, image_offsets=image_offsets)
    n_rows = int(match.pair_offsets[-1])
    matches0 = rng.integers(0, K, n_rows, dtype=np.int32)
    matches0[rng.random(n_rows, dtype=np.float32) >= 0.6] = -1
    n_points = n_db * K // 10
    kp_point = rng.integers(0, n_points, n_set * K)
    kp_point[rng.random(n_set * K, dtype=np.float32) < 0.5] = -1
    kp_point[:Q * K] = -1
    gather = LocalizationPairs(ctx, match, rng.uniform(0, 1000, (n_set * K, 2)), kp_point, rng.uniform(-1, 1, (n_points, 3)))
    d_m = ctx.to_device(matches0, np.int32)
    problem_offsets = np.arange(0, Q * R + 1, R)
    cap = n_rows
    out = dict(corr_offsets=ctx.empty((Q + 1,), np.int64), corr_kp=ctx.empty((cap,), np.int32), corr_point=ctx.empty((cap,), np.int64),
               corr_xy=ctx.empty((cap, 2), np.float64), corr_xyz=ctx.empty((cap, 3), np.float64))
    last = {}

    def run():
        last["out"] = gather.gather(d_m, problem_offsets, np.arange(Q * R), timed=True, out=out)
    ms = timed_runs(run, lambda: gather.kernel_ms, args.repeats)
    ret_offsets = np.arange(0, Q * R + 1, R)
    cl = timed_runs(lambda: last.update(cl=graph.clusters(ret_offsets, ret.reshape(-1), timed=True)), lambda: graph.kernel_ms, args.repeats)
    # the host route for a few queries: download the matches, loop
    hq = min(args.host_queries, Q)
    t0 = time.perf_counter()
    host_m = d_m.download()
    n_host = 0
    for q in range(hq):
        items, ids = [], {}
        for r in range(R):
            p = q * R + r
            m = host_m[match.pair_offsets[p]:match.pair_offsets[p + 1]]
            k = np.flatnonzero(m >= 0)
            items.append((r, np.stack([k, m[k]], 1)))
            db = pairs[p, 1]
            ids[r] = kp_point[image_offsets[db]:image_offsets[db + 1]]
        n_host += len(pairs_2d3d_from_matches(items, ids)[0])
    host_ms = 1e3 * (time.perf_counter() - t0)
    offs = last["out"]["corr_offsets"].download()
    assert int(offs[hq]) == n_host, "the host loop found another number of pairs"
    return {"queries": Q, "retrieved": R, "keypoints": K, "match_rows": n_rows, "lanes": Q * K, "pairs_emitted": int(last["out"]["n_corr"]),
            "gather_kernel_ms": ms, "clusters_kernel_ms": cl, "mean_clusters": float(last["cl"][1].download().mean()),
            "host_loop": {"queries": hq, "ms": host_ms, "ms_extrapolated_to_all": host_ms * Q / hq}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--observations", type=int, default=1000000)
    ap.add_argument("--num-matched", type=int, default=20)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--retrieved", type=int, default=20)
    ap.add_argument("--keypoints", type=int, default=2000)
    ap.add_argument("--host-queries", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pixsfm_amd.engine import Context
    ctx = Context(0)
    covis, graph = covisibility_part(ctx, args)
    result = {"covisibility": covis, "localization": gather_part(ctx, args, graph)}
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
