#!/usr/bin/env python3
"""Global mapping next to incremental mapping on the ring of tools/bench_mapping.py, and one positioning-only run at scale.

    python tools/bench_global_mapping.py --out profiles/global_mapping_bench.json

Part 1 (the ring: 50 images, 2000 points seen by 15 neighbours = 30 000 observations, 700 pairs; tests/mapping_cases.py ring_scene,
geometries from TwoViewVerifier): GlobalMapper.reconstruct and IncrementalMapper.reconstruct (init_max_trials = every pair, as in
bench_mapping.py) in the same process, one untimed warm-up run each, then --repeats runs; wall times are host clocks around
reconstruct() (every stage ends in a download, so in device synchronisation), stage times are the HIP-event times of the *_timed
entry points.  Medians.  (IncrementalMapper as another commit has it: that commit's tools/bench_mapping.py on the same ring, run
in the same session.)
Part 2 (--scale-images 1000 --scale-observations 1000000: ring images, tracks of five images 3, 10 or 40 apart, ground-truth rotations,
pairs between images one or two such steps apart): pxr_global_positioning_timed alone, per stage and round, the bytes the contraction adds per second (72 per
3 x 3 block it issues, 25 blocks per track of five less those in the lower triangle), the Cholesky's share, and the shader clock
sampled during the timed runs (bench.py's telemetry sampler)."""
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


def ring_part(ctx, args):
    import mapping_cases as mc
    from pixsfm_amd.api import GlobalMapper, IncrementalMapper, TwoViewVerifier
    scene = mc.ring_scene(n_images=args.images, n_points=args.points, views=args.views, seed=0)
    pairs, matches = mc.matches_from_labels(scene)
    graph, labels = mc.graph_and_labels(scene, pairs, matches)
    geoms = TwoViewVerifier.create({}, ctx=ctx).verify_pairs(scene["keypoints"], scene["cameras"], pairs, matches)[2]
    out = {"scene": {"images": args.images, "points": args.points, "views": args.views, "pairs": len(pairs),
                     "observations": int(sum(len(k) for k in scene["keypoints"].values()))}}
    for name, mapper in (("global", GlobalMapper.create({}, ctx=ctx)),
                         ("incremental", IncrementalMapper.create({'init_max_trials': len(pairs)}, ctx=ctx))):
        def run():
            t0 = time.perf_counter()
            rec, summary = mapper.reconstruct(scene["cameras"], scene["keypoints"], graph, pairs, geoms, track_labels=labels)
            return rec, summary, 1e3 * (time.perf_counter() - t0)
        run()                                                                                     # warm-up
        walls, stages = [], {}
        for _ in range(args.repeats):
            rec, summary, wall = run()
            walls.append(wall)
            for k, v in summary["kernel_ms"].items():
                stages.setdefault(k, []).append(v)
        rot, cen = mc.pose_errors(rec, scene["poses"]) if len(rec.images) >= 3 else (float("nan"), float("nan"))
        res = {"status": summary["status"], "registered": summary["num_reg_images"], "points3D": summary["num_points3D"],
               "reconstruct_wall_ms": stats(walls), "stage_ms_per_run": {k: stats(v) for k, v in stages.items()},
               "mean_reprojection_error_px": summary.get("mean_reprojection_error"), "max_rotation_error_deg": rot, "max_centre_error": cen}
        if name == "global":
            res.update({k: summary.get(k) for k in ("rotation_iterations", "positioning_rounds", "rotation_kernel_ms", "positioning_kernel_ms",
                                                    "zero_weight_observations", "zero_weight_pairs", "refinement_wall_ms")})
        else:
            res.update(rounds=len(summary["rounds"]), init_wall_ms=summary.get("init_wall_ms"))
        out[name] = res
    return out


def scale_part(ctx, args):
    import global_mapping_cases as gc
    from pixsfm_amd.engine import GlobalPositioningProblem
    n, nb = args.scale_images, 5
    n_tracks = args.scale_observations // nb
    rng = np.random.default_rng(0)
    q, t, c = gc.ring_poses(n, rng)
    X = rng.uniform(-2.0, 2.0, (n_tracks, 3))
    first = rng.integers(0, n, n_tracks)
    # a track's five images are 3, 10 or 40 images apart (1, 3.6 or 14.4 degrees at n = 1000): short tracks tie neighbours, long ones
    # close loops; one stride alone that divides n would split the ring into components
    strides = np.array([3, 10, 40])[rng.integers(0, 3, n_tracks)]
    obs_image = ((first[:, None] + strides[:, None] * np.arange(nb)[None]) % n).reshape(-1)
    xy = gc.project(q[obs_image], t[obs_image], X[np.repeat(np.arange(n_tracks), nb)]) + rng.normal(0.0, 0.5, (len(obs_image), 2))
    pairs = np.array([(i, (i + s * k) % n) for s in (3, 10, 40) for k in (1, 2) for i in range(n)], np.int32)    # images that share tracks
    pq, pt, pw, _ = gc.noisy_pairs(rng, q, c, pairs, outlier_share=0.0)
    b = gc.pair_directions(q, pairs, pt)
    prob = GlobalPositioningProblem(ctx, dict(track_offsets=np.arange(0, len(obs_image) + 1, nb), obs_image=obs_image, obs_xy=xy,
                                              image_camera=np.zeros(n, np.int32), qvec=q, cam_model=[0],
                                              cam_params=[[gc.FOCAL, gc.WIDTH / 2, gc.HEIGHT / 2]]), pairs, b, pw, 0)
    prob.solve(timed=True)                                                                        # warm-up
    runs, last = [], {}

    def loop():
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            last["out"] = prob.solve(timed=True)
            runs.append(dict(prob.kernel_ms, wall=1e3 * (time.perf_counter() - t0)))
    try:                                                                                          # the shader clock during the timed runs
        import bench
        telemetry = bench.GpuTelemetry(0).sample_while(loop, interval=0.002)
    except Exception as e:  # noqa: BLE001
        telemetry = {"note": "no telemetry: %r" % (e,)}
        if not runs:
            loop()
    out = last["out"]
    rounds = max(out["rounds"], 1)
    per_round = {k: stats([r[k] / rounds for r in runs]) for k in runs[0]}
    aligned = gc.similarity_align(out["centre"].download(), c)[0]
    # blocks issued per track of five distinct images: 10 pairs i < j (9 entries) and 5 diagonal blocks (6 entries)
    added_bytes = n_tracks * (10 * 9 + 5 * 6) * 8
    total = sum(per_round[k]["median"] for k in ("tracks", "contraction", "gauge_pack", "cholesky", "update"))
    return {"images": n, "observations": int(len(obs_image)), "tracks": int(n_tracks), "pairs": int(len(pairs)), "status": out["status"],
            "rounds": out["rounds"], "ms_per_round": per_round,
            "contraction_added_bytes_per_round": added_bytes,
            "contraction_added_GB_per_s": added_bytes / (per_round["contraction"]["median"] * 1e-3) / 1e9,
            "share_of_a_round": {k: per_round[k]["median"] / total for k in ("tracks", "contraction", "gauge_pack", "cholesky", "update")},
            "max_centre_error": float(np.linalg.norm(aligned - c, axis=1).max()), "telemetry": telemetry}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=50)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--views", type=int, default=15)
    ap.add_argument("--scale-images", type=int, default=1000)
    ap.add_argument("--scale-observations", type=int, default=1000000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pixsfm_amd.engine import Context
    ctx = Context(0)
    result = {"ring": ring_part(ctx, args)}
    if args.scale_images > 1:
        result["positioning_at_scale"] = scale_part(ctx, args)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
