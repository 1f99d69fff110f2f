#!/usr/bin/env python3
"""Geometric BA on the flagship scene: the evaluation kernel on its own, and ms per LM iteration of pxr_ba_solve_geometric
next to pxr_ba_solve on the SAME scene in the same process.

    python tools/bench_geometric.py --out profiles/geom_ba_bench.json

Scene: BASELINE configs[2] from synthetic_gpu.make_ba_problem_gpu (200 cameras, 200k points, 1M observations); the observed
keypoints of the geometric problem are its true projections (`centers`) plus seeded Gaussian noise.  Timing: HIP events on the
context's stream around work that ends in a synchronisation; an untimed warm-up solve of each kind first; the two variants
alternated --repeats times; medians and the spread (min, max) of the repeats are reported.  bench.py is the project's
yardstick and is not touched: this tool only adds the geometric figures."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pixel-perfect-sfm_amd"))


def stats(values):
    v = sorted(float(x) for x in values)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "all": [round(x, 5) for x in values]}


def gauge(n_img, n_pts):
    pose_const = np.zeros(n_img, np.uint8); pose_const[0] = 1
    tmask = np.zeros(n_img, np.uint8); tmask[1] = 1
    return pose_const, tmask, np.full(n_img, 0b0110, np.uint16), np.zeros(n_pts, np.uint8)      # SIMPLE_RADIAL: f and k refined


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cams", type=int, default=200)
    ap.add_argument("--points", type=int, default=200_000)
    ap.add_argument("--obs-per-point", type=int, default=5)
    ap.add_argument("--lm-iters", type=int, default=10)
    ap.add_argument("--eval-launches", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--keypoint-noise", type=float, default=0.5)
    ap.add_argument("--no-featuremetric", action="store_true", help="geometric figures only (no patch arena is rendered)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from pixsfm_amd import synthetic_gpu
    from pixsfm_amd.engine import BAProblem, Context, GeometricBAProblem, PatchArena, interp_cfg, lm_options, make_loss
    stream = torch.cuda.current_stream().cuda_stream
    ctx = Context(0, stream)
    prob, patches = synthetic_gpu.make_ba_problem_gpu("cuda:0", n_cams=args.cams, n_points=args.points,
                                                      obs_per_point=args.obs_per_point,
                                                      patch_size=2 if args.no_featuremetric else 16,
                                                      channels=8 if args.no_featuremetric else 128)
    n_obs = len(prob["obs_image"])
    rng = np.random.default_rng(12345)
    prob["obs_xy"] = prob["centers"] + rng.normal(0.0, args.keypoint_noise, prob["centers"].shape)
    geo = GeometricBAProblem(ctx, prob)
    feat = None
    if not args.no_featuremetric:
        arena = PatchArena(ctx, n_obs, 16, 16, 128, np.float16, device_ptr=patches.data_ptr())
        arena.upload(0, None, prob["corners"], prob["scales"])
        feat = BAProblem(ctx, arena, prob)
    g = gauge(args.cams, args.points)
    loss = make_loss("cauchy", [0.25])
    cfg = interp_cfg()

    def reset(ba):
        for name in ("qvec", "tvec", "xyz"):
            ba.d[name].upload(prob[name])
        ba.d["cam_params"].upload(prob["cam_params"])

    out = {"scene": {"cameras": args.cams, "points": args.points, "observations": n_obs, "keypoint_noise_px": args.keypoint_noise},
           "method": "HIP events on the context's stream; untimed warm-up first; variants alternated %d times; median and spread" % args.repeats}

    # ---- geom_eval_kernel on its own ---------------------------------------------------------------------------------------------
    streamed = 4 + 4 + 16                 # obs_image, obs_point, obs_xy
    written = 64                          # the record
    gathered = 4 + 32 + 24 + 24 + 4 + 96  # image_camera, q, t, X, model, k: 200 images / 200k points -- L2 resident
    for _ in range(5):
        geo.eval(residuals=False)
    ctx.sync()
    ms = []
    for _ in range(args.repeats):
        ctx.timer_start()
        for _ in range(args.eval_launches):
            geo.eval(residuals=False)
        ms.append(ctx.timer_stop() / args.eval_launches)
    st = stats(ms)
    out["geom_eval_kernel"] = {"ms_per_launch": st, "launches_per_sample": args.eval_launches,
                               "bytes_per_observation": {"streamed_reads": streamed, "written": written, "gathered_reads": gathered},
                               "GBps_streamed_plus_written": 1e-6 * n_obs * (streamed + written) / st["median"],
                               "GBps_with_gathers": 1e-6 * n_obs * (streamed + written + gathered) / st["median"]}
    print("geom_eval_kernel: %.4f ms per launch (%.4f .. %.4f), %.0f GB/s streamed + written" % (
        st["median"], st["min"], st["max"], out["geom_eval_kernel"]["GBps_streamed_plus_written"]), file=sys.stderr)

    # ---- ms per LM iteration, geometric next to featuremetric ----------------------------------------------------------------------
    def solve(ba, inner, iters):
        reset(ba)
        opts = lm_options(max_iterations=iters, use_inner_iterations=inner)
        ctx.sync()
        ctx.timer_start()
        s = ba.solve(loss, *g, options=opts) if ba is geo else ba.solve(cfg, loss, *g, options=opts)
        wall = ctx.timer_stop()
        return s, wall

    variants = [("geometric", geo)] + ([("featuremetric", feat)] if feat is not None else [])
    for _, ba in variants:                # untimed warm-up: code objects, work-buffer arena, the Gram-matrix cache
        solve(ba, True, 2)
    lm = {}
    for key, inner in (("lm", True), ("lm_no_inner", False)):
        per = {name: {"ms_per_iteration": [], "event_ms_per_iteration": [], "iterations": [], "final_cost": []} for name, _ in variants}
        for _ in range(args.repeats):
            for name, ba in variants:
                s, wall = solve(ba, inner, args.lm_iters)
                it = max(1, s["iterations"])
                # total_ms: the solver's own clock from the initial evaluation to the end of the loop (what bench.py's lm figures use)
                per[name]["ms_per_iteration"].append(s["total_ms"] / it)
                per[name]["event_ms_per_iteration"].append(wall / it)      # + set-up, between HIP events
                per[name]["iterations"].append(s["iterations"])
                per[name]["final_cost"].append(s["final_cost"])
        lm[key] = {}
        for name, _ in variants:
            lm[key][name] = {"ms_per_iteration": stats(per[name]["ms_per_iteration"]),
                             "event_ms_per_iteration_with_setup": stats(per[name]["event_ms_per_iteration"]),
                             "iterations": per[name]["iterations"], "final_cost": per[name]["final_cost"][0],
                             "same_bits_every_repeat": len(set(per[name]["final_cost"])) == 1}
            print("%s %s: %.3f ms per iteration (%.3f .. %.3f)" % (key, name, lm[key][name]["ms_per_iteration"]["median"],
                  lm[key][name]["ms_per_iteration"]["min"], lm[key][name]["ms_per_iteration"]["max"]), file=sys.stderr)
        if feat is not None:
            a, b = lm[key]["geometric"]["ms_per_iteration"], lm[key]["featuremetric"]["ms_per_iteration"]
            lm[key]["geometric_not_slower"] = bool(a["median"] <= b["median"] or a["min"] <= b["max"])
    out["lm_iteration"] = lm
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
