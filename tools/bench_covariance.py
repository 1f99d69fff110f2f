#!/usr/bin/env python3
"""BA covariance at the direct solver's largest scene: 1000 images (n_c ~ 6000 camera-side columns), ~1M observations on the
synthetic scene of tools/bench_geometric.py; geometric records.

    python tools/bench_covariance.py --out profiles/ba_covariance_bench.json

Reports the stages of pxr_ba_covariance as the call itself times them (host clock between stream synchronisations: set-up +
linearisation + Schur complement, factor + inverse, point propagation + scatter), the dense inverse on its own between HIP
events with its share of the fp64 matrix pipe's measured rate (44 TFLOP/s, profiles/r4_mfma_f64_rate.txt; n^3 flop: n^3 / 3
each for the factor, the triangular inverse and the product), and torch.linalg.cholesky + torch.cholesky_inverse on the same
device and the same matrix size for scale.  An untimed warm-up call first; medians and the spread of --repeats calls."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pixel-perfect-sfm_amd"))

FP64_MATRIX_TFLOPS = 44.0


def stats(values):
    v = sorted(float(x) for x in values)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cams", type=int, default=1000)
    ap.add_argument("--points", type=int, default=200_000)
    ap.add_argument("--obs-per-point", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--keypoint-noise", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from pixsfm_amd import synthetic_gpu
    from pixsfm_amd.engine import Context, GeometricBAProblem, dense_spd_inverse, make_loss
    ctx = Context(0, torch.cuda.current_stream().cuda_stream)
    prob, _ = synthetic_gpu.make_ba_problem_gpu("cuda:0", n_cams=args.cams, n_points=args.points, obs_per_point=args.obs_per_point,
                                                patch_size=2, channels=8)
    n_obs = len(prob["obs_image"])
    rng = np.random.default_rng(12345)
    prob["obs_xy"] = prob["centers"] + rng.normal(0.0, args.keypoint_noise, prob["centers"].shape)
    geo = GeometricBAProblem(ctx, prob)
    n_img, n_cam = len(prob["image_camera"]), len(prob["cam_model"])
    pose_const = np.zeros(n_img, np.uint8); pose_const[0] = 1
    tmask = np.zeros(n_img, np.uint8); tmask[1] = 1
    gauge = (pose_const, tmask, np.full(n_cam, 0xfff, np.uint16), np.zeros(args.points, np.uint8))     # intrinsics constant
    loss = make_loss("cauchy", [0.25])
    geo.eval(residuals=False)
    geo.covariance(loss, *gauge)                                                                       # warm-up
    stages = {"ms_linearise": [], "ms_factor_inverse": [], "ms_points": []}
    summary = None
    for _ in range(args.repeats):
        summary = geo.covariance(loss, *gauge)["summary"]
        for k in stages:
            stages[k].append(summary[k])
    n_c = summary["num_camera_unknowns"]
    out = {"scene": {"images": args.cams, "points": args.points, "observations": n_obs, "n_c": n_c,
                     "singular_points": summary["num_singular_points"], "info": summary["info"]},
           "method": "stages: the call's own host clock between stream synchronisations; dense inverse and torch: device events; "
                     "one untimed warm-up, median (min .. max) of %d calls" % args.repeats,
           "pxr_ba_covariance_ms": {k: stats(v) for k, v in stages.items()}}

    # ---- the dense inverse on its own, and torch on the same size ---------------------------------------------------------------
    g = torch.Generator(device="cuda").manual_seed(1)
    M = torch.randn((n_c, n_c + 8), dtype=torch.float64, device="cuda", generator=g)
    A = M @ M.T + 1e-3 * n_c * torch.eye(n_c, dtype=torch.float64, device="cuda")
    host = A.cpu().numpy()
    d = ctx.to_device(host)
    dense_spd_inverse(ctx, d)                                                                          # warm-up
    ms = []
    for _ in range(args.repeats):
        d.upload(host)
        ctx.sync()
        ctx.timer_start()
        info, _ = dense_spd_inverse(ctx, d)
        ms.append(ctx.timer_stop())
        assert info == 0
    st = stats(ms)
    tflops = 1e-9 * float(n_c) ** 3 / st["median"]
    out["pxr_dense_spd_inverse"] = {"n": n_c, "ms": st, "TFLOPs": tflops, "fraction_of_fp64_matrix_rate": tflops / FP64_MATRIX_TFLOPS,
                                    "fp64_matrix_rate_TFLOPs": FP64_MATRIX_TFLOPS}
    X = d.download()
    out["pxr_dense_spd_inverse"]["max_abs_XA_minus_I"] = float(np.abs(X[:256] @ host - np.eye(n_c)[:256]).max())
    torch.cholesky_inverse(torch.linalg.cholesky(A))                                                   # warm-up
    tms = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cholesky_inverse(torch.linalg.cholesky(A))
        e1.record()
        torch.cuda.synchronize()
        tms.append(e0.elapsed_time(e1))
    out["torch_cholesky_plus_cholesky_inverse"] = {"n": n_c, "ms": stats(tms)}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
