#!/usr/bin/env python3
"""Incremental mapping on a ring scene: milliseconds per stage per round, and registered images per second.

    python tools/bench_mapping.py --images 50 --points 2000 --views 15 --out profiles/mapping_bench.json

Scene (tests/mapping_cases.py ring_scene): N ring images of one SIMPLE_RADIAL camera, P points each seen by V neighbouring images,
keypoint noise 0.5 px, tracks from ground truth, one match per shared track between every two images that share any, geometries
from TwoViewVerifier (timed apart: it is the stage before the mapper).  On a ring the pairs with the most matches are the
neighbours, whose parallax (360 / N degrees) is below init_min_tri_angle for N > 22: the mapper turns them down one by one, so
init_max_trials is raised to --init-max-trials (default: every pair) and the time of that search is reported apart.
Timing: one untimed warm-up run of the whole mapper (code objects, the context's workspace), then --repeats runs; a run's wall
time is a host clock around reconstruct() -- which includes the one walk over the input objects before and after -- and ends in
device synchronisation (every stage downloads its results); the stages' times are the HIP-event times of the *_timed entry points
(triangulation, visibility, absolute pose) and a host clock around the bundle adjustment's solve.  Medians over the repeats; the
per-round table is that of the last run.  max_images_per_round limits the batch (0: every candidate of a round at once)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "oracle", "pixel-perfect-sfm_amd"):
    sys.path.insert(0, os.path.join(ROOT, p))


def stats(values):
    v = sorted(float(x) for x in values)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=50)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--views", type=int, default=15)
    ap.add_argument("--init-max-trials", type=int, default=0)
    ap.add_argument("--max-images-per-round", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import mapping_cases as mc
    from pixsfm_amd.api import IncrementalMapper, TwoViewVerifier
    from pixsfm_amd.engine import Context
    scene = mc.ring_scene(n_images=args.images, n_points=args.points, views=args.views, seed=0)
    pairs, matches = mc.matches_from_labels(scene)
    graph, labels = mc.graph_and_labels(scene, pairs, matches)
    ctx = Context(0)
    verifier = TwoViewVerifier.create({}, ctx=ctx)
    verifier.verify_pairs(scene["keypoints"], scene["cameras"], pairs, matches)                  # warm-up
    t0 = time.perf_counter()
    geoms = verifier.verify_pairs(scene["keypoints"], scene["cameras"], pairs, matches)[2]
    verify_ms = 1e3 * (time.perf_counter() - t0)
    mapper = IncrementalMapper.create({'max_images_per_round': args.max_images_per_round,
                                       'init_max_trials': args.init_max_trials or len(pairs)}, ctx=ctx)

    def run():
        t0 = time.perf_counter()
        rec, summary = mapper.reconstruct(scene["cameras"], scene["keypoints"], graph, pairs, geoms, track_labels=labels)
        return rec, summary, 1e3 * (time.perf_counter() - t0)
    run()                                                                                         # warm-up
    walls, stages, inits = [], {}, []
    for _ in range(args.repeats):
        rec, summary, wall = run()
        walls.append(wall)
        inits.append(summary["init_wall_ms"])
        for k, v in summary["kernel_ms"].items():
            stages.setdefault(k, []).append(v)
    wall = stats(walls)
    rot, cen = mc.pose_errors(rec, scene["poses"]) if len(rec.images) >= 3 else (float("nan"), float("nan"))
    result = {
        "scene": {"images": args.images, "points": args.points, "views": args.views, "pairs": len(pairs), "observations": int(sum(len(k) for k in scene["keypoints"].values()))},
        "max_images_per_round": args.max_images_per_round, "status": summary["status"], "registered": summary["num_reg_images"],
        "points3D": summary["num_points3D"], "rounds": len(summary["rounds"]),
        "verify_pairs_wall_ms": verify_ms, "reconstruct_wall_ms": wall,
        "initial_pair": summary["initial_pair"], "initial_pair_trials": len(summary["init_trials"]), "init_wall_ms": stats(inits),
        "images_per_second": summary["num_reg_images"] / (wall["median"] * 1e-3),
        "stage_ms_per_run": {k: stats(v) for k, v in stages.items()},
        "per_round": [dict(candidates=r["candidates"], registered=r["registered"], points=r["points"], **{k: round(v, 4) for k, v in r["ms"].items()})
                      for r in summary["rounds"]],
        "mean_reprojection_error_px": summary.get("mean_reprojection_error"),
        "max_rotation_error_deg": rot, "max_centre_error": cen,
    }
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
