#!/usr/bin/env python3
"""Guided descriptor matching (pxr_match_guided) on the batch of tools/bench_matching.py: 64 images of 4096 descriptors, D = 128,
256 image pairs, conf "NN-ratio" -- plus synthetic keypoints in [-1, 1]^2 and one random epipolar model per pair, with the pair's
threshold chosen (on a sample of its entries) so that about one candidate in fifty is admissible.

    python tools/bench_guided_matching.py --out profiles/guided_matching_bench.json

Reports the HIP-event time of every kernel, guided next to unguided in the same process (the two alternate launch by launch;
medians and spread over --repeats launches each after a warm-up), what the gate costs (guided tiles / unguided tiles), the guided
tile kernel as a fraction of the f32-input MFMA rate at the shader clock sampled while the kernels run, and pairs per second.
Nobody fixed a target for any of this.  bench.py is the project's yardstick and is not touched (only its telemetry sampler is
imported)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pixel-perfect-sfm_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_matching import make_images, stats  # noqa: E402


def epipolar_batch(n_images, n_desc, pairs, fraction, seed=2, sample=512):
    """Keypoints per image, and per pair a random rank-2 model and the threshold under which about `fraction` of the entries pass
    (the Sampson error of a sample x sample block of the pair, in plain numpy)."""
    rng = np.random.default_rng(seed)
    xy = [rng.uniform(-1, 1, (n_desc, 2)) for _ in range(n_images)]
    models, thrs = [], []
    for a, b in pairs:
        U, s, Vt = np.linalg.svd(rng.standard_normal((3, 3)))
        M = (U * np.array([s[0], s[1], 0.0])) @ Vt
        xa, xb = np.c_[xy[a][:sample], np.ones(min(sample, n_desc))], np.c_[xy[b][:sample], np.ones(min(sample, n_desc))]
        la, lb = xa @ M.T, xb @ M
        err = (xb @ la.T).T ** 2 / ((la[:, 0] ** 2 + la[:, 1] ** 2)[:, None] + (lb[:, 0] ** 2 + lb[:, 1] ** 2)[None, :])
        models.append(M)
        thrs.append(float(np.sqrt(np.quantile(err, fraction))))
    return xy, np.array(models), np.array(thrs)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--descriptors", type=int, default=4096)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--conf", default="NN-ratio")
    ap.add_argument("--fraction", type=float, default=0.02, help="share of the candidates that the gate admits")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from pixsfm_amd._lib import GUIDE_EPIPOLAR
    from pixsfm_amd.engine import MATCH_CONFS, Context, MatchProblem
    descs = make_images(args.images, args.descriptors, args.dim)
    rng = np.random.default_rng(1)
    all_pairs = [(i, j) for i in range(args.images) for j in range(i + 1, args.images)]
    pairs = np.array([all_pairs[k] for k in rng.permutation(len(all_pairs))[:args.pairs]], dtype=np.int32)
    xy, models, thrs = epipolar_batch(args.images, args.descriptors, pairs, args.fraction)
    kinds = np.full(len(pairs), GUIDE_EPIPOLAR, np.int32)
    options = MATCH_CONFS[args.conf]

    ctx = Context(0)
    prob = MatchProblem(ctx, descs, pairs, keypoints=xy)
    out_u = prob.run(**options)                                          # warm-up (allocates the workspace)
    out_g = prob.run_guided(kinds, models, thrs, **options)
    ctx.sync()
    kernels, wall = {"unguided": {}, "guided": {}}, {"unguided": [], "guided": []}

    def loop():
        for _ in range(args.repeats):
            for which in ("unguided", "guided"):
                t0 = time.perf_counter()
                if which == "guided":
                    prob.run_guided(kinds, models, thrs, timed=True, out=out_g, **options)
                else:
                    prob.run(timed=True, out=out_u, **options)
                ctx.sync()
                wall[which].append(1e3 * (time.perf_counter() - t0))
                for name, ms in prob.kernel_ms.items():
                    kernels[which].setdefault(name, []).append(ms)

    try:
        import bench
        telemetry = bench.GpuTelemetry(0).sample_while(loop, interval=0.002)
    except Exception as e:  # noqa: BLE001
        telemetry = {"note": "no telemetry: %r" % (e,)}
        if not wall["guided"]:
            loop()
    n_u, n_g = out_u[2].download(), out_g[2].download()
    total = {w: sum(stats(v)["median"] for v in kernels[w].values()) for w in kernels}
    tiles = {w: stats(kernels[w]["tiles"])["median"] for w in kernels}
    flop = 2.0 * args.dim * float(sum(len(descs[a]) * len(descs[b]) for a, b in pairs))
    sclk = ((telemetry or {}).get("sclk_mhz") or {}).get("mean")
    cus = 256
    try:
        import torch
        cus = torch.cuda.get_device_properties(0).multi_processor_count
    except Exception:  # noqa: BLE001
        pass
    result = {
        "scene": {"images": args.images, "descriptors_per_image": args.descriptors, "dim": args.dim, "pairs": int(len(pairs)), "conf": args.conf,
                  "kind": "epipolar", "admissible_fraction_target": args.fraction},
        "kernel_ms": {w: {name: stats(v) for name, v in kernels[w].items()} for w in kernels},
        "kernels_total_ms": total, "call_wall_ms": {w: stats(v) for w, v in wall.items()},
        "guided_over_unguided_tiles": tiles["guided"] / tiles["unguided"],
        "guided_over_unguided_total": total["guided"] / total["unguided"],
        "pairs_per_second_kernels": {w: len(pairs) / (total[w] * 1e-3) for w in total},
        "similarity_flop": flop, "tiles_tflops": {w: flop / (tiles[w] * 1e-3) * 1e-12 for w in tiles},
        "matches_per_pair_mean": {"unguided": float(n_u.mean()), "guided": float(n_g.mean())},
        "telemetry": telemetry, "compute_units": cus,
    }
    if sclk:
        peak = cus * 4 * 64.0 * sclk * 1e6                               # FLOP/s: 4096 FLOP per 64 cycles per SIMD
        result["f32_mfma_peak_tflops_at_sampled_clock"] = peak * 1e-12
        result["tiles_fraction_of_f32_mfma_peak"] = {w: flop / (tiles[w] * 1e-3) / peak for w in tiles}
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
