#!/usr/bin/env python3
"""Track triangulation at the benchmark scene's shape: HIP-event times of the kernels of pxr_triangulate_tracks, tracks per
second, and the same estimator in numpy (tests/triangulation_cases.py, through the C oracle's camera models) on a sample of
the tracks for scale.

    python tools/bench_triangulation.py --out profiles/triangulation_bench.json

Scene: 200 ring cameras (SIMPLE_RADIAL), 200k tracks of 5 views = 1M observations, keypoint noise 0.5 px, 20 % of the
observations displaced by 100-300 px.  Timing: pxr_triangulate_tracks_timed brackets each kernel with HIP events on the
context's stream; one untimed warm-up call (it also grows the context's workspace), then --repeats calls; medians and the
spread are reported.  The wall time of a call adds the host part: the offsets' copy, validation and the sort by length."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tools", "tests", "oracle", "pixel-perfect-sfm_amd"):
    sys.path.insert(0, os.path.join(ROOT, p))


from _bench_runs import stats as _stats, timed_runs  # noqa: E402


def stats(values):
    return _stats(values, keep_all=False)


def make_scene(n_cams, n_tracks, track_len, sigma, p_outlier, seed):
    from pixsfm_amd import synthetic
    rng = np.random.default_rng(seed)
    q, t = synthetic.ring_cameras(n_cams, rng=rng)
    R = np.stack([synthetic.qvec_to_rotmat(x) for x in q])
    k = np.array([1200.0, 500.0, 500.0, 0.02])
    X = rng.uniform(-1, 1, (n_tracks, 3))
    cams = np.argsort(rng.random((n_tracks, n_cams)), axis=1)[:, :track_len].astype(np.int32)      # distinct cameras per track
    obs_image = cams.reshape(-1)
    p = np.einsum("nij,nj->ni", R[obs_image], np.repeat(X, track_len, 0)) + t[obs_image]
    u, v = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
    rad = 1.0 + k[3] * (u * u + v * v)
    xy = np.stack([k[0] * u * rad + k[1], k[0] * v * rad + k[2]], 1) + rng.normal(0, sigma, (len(u), 2))
    bad = rng.random(len(u)) < p_outlier
    a, r = rng.uniform(0, 2 * np.pi, len(u)), rng.uniform(100, 300, len(u))
    xy[bad] += (r[:, None] * np.stack([np.cos(a), np.sin(a)], 1))[bad]
    return dict(track_offsets=np.arange(n_tracks + 1, dtype=np.int64) * track_len, obs_image=obs_image, obs_xy=xy,
                image_camera=np.zeros(n_cams, np.int32), qvec=q, tvec=t, cam_model=np.array([2], np.int32),
                cam_params=k[None, :], gt_xyz=X, true_inlier=~bad)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cams", type=int, default=200)
    ap.add_argument("--tracks", type=int, default=200_000)
    ap.add_argument("--track-len", type=int, default=5)
    ap.add_argument("--outliers", type=float, default=0.2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--numpy-sample", type=int, default=2000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from pixsfm_amd.engine import Context, TriangulationProblem
    scene = make_scene(args.cams, args.tracks, args.track_len, 0.5, args.outliers, seed=7)
    ctx = Context(0)
    prob = TriangulationProblem(ctx, scene)
    out, kernels, wall = timed_runs(ctx, prob.triangulate, args.repeats)
    xyz, status, n_inl = out[0].download(), out[1].download(), out[2].download()
    ok = status == 0
    gpu_ms = sum(stats(v)["median"] for v in kernels.values())
    result = {
        "scene": {"cameras": args.cams, "tracks": args.tracks, "observations": len(scene["obs_image"]), "outlier_fraction": args.outliers},
        "kernel_ms": {name: stats(v) for name, v in kernels.items()},
        "kernels_total_ms": gpu_ms, "call_wall_ms": stats(wall),
        "tracks_per_second_kernels": args.tracks / (gpu_ms * 1e-3), "tracks_per_second_call": args.tracks / (stats(wall)["median"] * 1e-3),
        "status_counts": np.bincount(status, minlength=4).tolist(), "mean_inliers": float(n_inl[ok].mean()),
        "median_point_error": float(np.median(np.linalg.norm(xyz[ok] - scene["gt_xyz"][ok], axis=1))),
    }
    if args.numpy_sample > 0:
        import triangulation_cases as tc
        m = min(args.numpy_sample, args.tracks)
        sub = dict(scene, track_offsets=scene["track_offsets"][:m + 1], obs_image=scene["obs_image"][:m * args.track_len],
                   obs_xy=scene["obs_xy"][:m * args.track_len])
        sub["cam_params"] = tc.pad_params([scene["cam_params"][0]])
        t0 = time.perf_counter()
        ref = tc.reference(sub)
        dt = time.perf_counter() - t0
        same = bool(np.array_equal(ref["status"], status[:m]) and np.array_equal(ref["n_inliers"], n_inl[:m]))
        result["numpy"] = {"tracks": m, "seconds": dt, "tracks_per_second": m / dt, "agrees_with_gpu": same}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
