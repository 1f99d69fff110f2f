#!/usr/bin/env python3
"""Batched descriptor matching (pxr_match_descriptors) at the size of a small reconstruction: 64 images of 4096 descriptors,
D = 128, 256 image pairs, conf "NN-ratio".

    python tools/bench_matching.py --out profiles/matching_bench.json

Reports the HIP-event time of every kernel (medians and spread over --repeats launches after a warm-up), pairs per second, and the
similarity's FLOP/s (2 n_a n_b D per pair, against the tiles kernel's time) as a fraction of the f32-input MFMA rate: one
v_mfma_f32_32x32x2_f32 (4096 FLOP) per 64 cycles per SIMD, 4 SIMDs per CU, times the shader clock sampled while the kernels run.
For scale the same pairs go through torch on the same GPU (a @ b.T, topk(2) both ways, the same tests), timed with torch events;
its matches are compared with ours (they may differ where float32 GEMM rounding flips a near-tie; the count is reported).  Nobody
fixed a target for any of this.  bench.py is the project's yardstick and is not touched (only its telemetry sampler is imported)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pixel-perfect-sfm_amd"))
sys.path.insert(0, ROOT)


def stats(values):
    v = sorted(float(x) for x in values)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "all": [round(x, 5) for x in values]}


def make_images(n_images, n_desc, dim, seed=0, shared=0.5, noise=0.05):
    """Images that share half of their descriptors with a common pool (noisy, renormalised): the ratio test keeps some, drops some."""
    rng = np.random.default_rng(seed)
    pool = rng.standard_normal((2 * n_desc, dim))
    pool /= np.linalg.norm(pool, axis=1, keepdims=True)
    out = []
    for _ in range(n_images):
        k = int(shared * n_desc)
        d = np.concatenate([pool[rng.permutation(len(pool))[:k]] + noise * rng.standard_normal((k, dim)) / np.sqrt(dim),
                            rng.standard_normal((n_desc - k, dim))])
        d = d[rng.permutation(n_desc)]
        out.append((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32))
    return out


def torch_match(descs, pairs, ratio, repeats):
    import torch
    dev = torch.device("cuda:0")
    t = [torch.from_numpy(d).to(dev) for d in descs]
    r2 = torch.tensor(ratio * ratio, dtype=torch.float32, device=dev)

    def nn(sim):
        top, idx = sim.topk(2, dim=1)
        if ratio <= 0:
            return idx[:, 0]
        d = 2 * (1 - top)
        return torch.where(d[:, 0] <= r2 * d[:, 1], idx[:, 0], torch.full_like(idx[:, 0], -1))

    def run():
        out = []
        for a, b in pairs:
            sim = t[a] @ t[b].T
            m0, m1 = nn(sim), nn(sim.T)
            rows = torch.arange(len(m0), device=dev)
            back = m1[torch.where(m0 >= 0, m0, torch.zeros_like(m0))]
            out.append(torch.where((m0 >= 0) & (back == rows), m0, torch.full_like(m0, -1)))
        return out

    run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = run()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms, torch.cat(out).cpu().numpy().astype(np.int32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--descriptors", type=int, default=4096)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--conf", default="NN-ratio")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from pixsfm_amd.engine import MATCH_CONFS, Context, MatchProblem
    descs = make_images(args.images, args.descriptors, args.dim)
    rng = np.random.default_rng(1)
    all_pairs = [(i, j) for i in range(args.images) for j in range(i + 1, args.images)]
    pairs = np.array([all_pairs[k] for k in rng.permutation(len(all_pairs))[:args.pairs]], dtype=np.int32)
    options = MATCH_CONFS[args.conf]

    ctx = Context(0)
    prob = MatchProblem(ctx, descs, pairs)
    out = prob.run(**options)                                            # warm-up (allocates the workspace)
    ctx.sync()
    kernels, wall = {}, []

    def loop():
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            prob.run(timed=True, out=out, **options)
            ctx.sync()
            wall.append(1e3 * (time.perf_counter() - t0))
            for name, ms in prob.kernel_ms.items():
                kernels.setdefault(name, []).append(ms)

    telemetry = None
    try:
        import bench
        telemetry = bench.GpuTelemetry(0).sample_while(loop, interval=0.002)
    except Exception as e:  # noqa: BLE001
        telemetry = {"note": "no telemetry: %r" % (e,)}
        if not wall:
            loop()
    m, s, n = (a.download() for a in out)
    total_ms = sum(stats(v)["median"] for v in kernels.values())
    tiles_ms = stats(kernels["tiles"])["median"]
    flop = 2.0 * args.dim * float(sum(len(descs[a]) * len(descs[b]) for a, b in pairs))
    sclk = ((telemetry or {}).get("sclk_mhz") or {}).get("mean")
    props_cus = 256
    try:
        import torch
        props_cus = torch.cuda.get_device_properties(0).multi_processor_count
    except Exception:  # noqa: BLE001
        pass
    result = {
        "scene": {"images": args.images, "descriptors_per_image": args.descriptors, "dim": args.dim, "pairs": int(len(pairs)), "conf": args.conf},
        "kernel_ms": {name: stats(v) for name, v in kernels.items()},
        "kernels_total_ms": total_ms, "call_wall_ms": stats(wall),
        "pairs_per_second_kernels": len(pairs) / (total_ms * 1e-3),
        "similarity_flop": flop, "tiles_tflops": flop / (tiles_ms * 1e-3) * 1e-12,
        "matches_per_pair_mean": float(n.mean()), "telemetry": telemetry, "compute_units": props_cus,
    }
    if sclk:
        peak = props_cus * 4 * 64.0 * sclk * 1e6                        # FLOP/s: 4096 FLOP per 64 cycles per SIMD
        result["f32_mfma_peak_tflops_at_sampled_clock"] = peak * 1e-12
        result["tiles_fraction_of_f32_mfma_peak"] = flop / (tiles_ms * 1e-3) / peak
    if not args.no_torch:
        ms, tm = torch_match(descs, pairs, options["ratio_threshold"], max(3, args.repeats // 2))
        result["torch"] = {"ms": stats(ms), "pairs_per_second": len(pairs) / (stats(ms)["median"] * 1e-3),
                           "tflops_whole_loop": flop / (stats(ms)["median"] * 1e-3) * 1e-12,
                           "rows_differing_from_ours": int((tm != m).sum()), "rows": int(len(m))}
        result["torch_over_ours_time"] = stats(ms)["median"] / total_ms
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
