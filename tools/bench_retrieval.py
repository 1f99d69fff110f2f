#!/usr/bin/env python3
"""Image retrieval (pxr_vocab_train, pxr_vlad_aggregate, pxr_retrieval_topk) at the size of a large collection: 1000 images of 4096
descriptors, D = 128, a vocabulary of K = 64 learned from 262144 of them in 10 iterations, num_matched = 20.

    python tools/bench_retrieval.py --out profiles/retrieval_bench.json

Reports the HIP-event time of every kernel of the three entry points (medians and spread over --repeats calls after a warm-up;
training's are summed over its iterations), the assignment kernel's FLOP/s (2 n K D, against its time in the aggregation) as a
fraction of the f32-input MFMA rate -- one v_mfma_f32_32x32x2_f32 (4096 FLOP) per 64 cycles per SIMD, 4 SIMDs per CU, times the
shader clock sampled while the kernels run -- and the accumulation's bytes/s (the descriptors and assignments it reads, once per
block of centroids) against the 8 TB/s of HBM.  For scale the same steps run in torch on the same GPU (x @ c.T, argmax, index_add_,
topk), timed with torch events; its assignments and pairs are compared with ours (they may differ where float32 GEMM rounding
flips a near-tie; the counts are reported).  Nobody fixed a target for any of this.  bench.py is the project's yardstick and is
not touched (only its telemetry sampler is imported)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pixel-perfect-sfm_amd"))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_SECOND = 8.0e12


def stats(values):
    v = sorted(float(x) for x in values)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "all": [round(x, 5) for x in values]}


def make_descriptors(n_images, n_desc, dim, seed=0, words=512, noise=0.6):
    """(n_images * n_desc, dim) float32 unit rows: every image draws from its own window of a ring of `words` visual words, so that
    neighbouring images share words and the vocabulary has something to find."""
    rng = np.random.default_rng(seed)
    pool = rng.standard_normal((words, dim)).astype(np.float32)
    pool /= np.linalg.norm(pool, axis=1, keepdims=True)
    out = np.empty((n_images * n_desc, dim), np.float32)
    for m in range(n_images):
        first = m * words // n_images
        idx = (first + rng.integers(0, max(words // 8, 1), n_desc)) % words
        x = pool[idx] + (noise / np.sqrt(dim)) * rng.standard_normal((n_desc, dim), dtype=np.float32)
        out[m * n_desc:(m + 1) * n_desc] = x / np.linalg.norm(x, axis=1, keepdims=True)
    return out


def torch_steps(desc, n_images, centroids, train_rows, iterations, num_matched, repeats):
    """The same steps in torch: ({step: [ms]}, assign, top_index)."""
    import torch
    dev = torch.device("cuda:0")
    x = torch.from_numpy(desc).to(dev)
    c0 = torch.from_numpy(centroids).to(dev)
    K, D = c0.shape
    rows = torch.from_numpy(train_rows).to(dev)
    image = torch.arange(len(desc), device=dev) // (len(desc) // n_images)

    def train():
        t, c = x[rows], c0.clone()
        start = t[(torch.arange(K, device=dev) * len(t)) // K]
        c.copy_(start)
        for _ in range(iterations):
            a = (t @ c.T).argmax(1)
            s = torch.zeros_like(c).index_add_(0, a, t)
            n = torch.linalg.norm(s, dim=1, keepdim=True)
            c = torch.where(n > 0, s / n.clamp_min(1e-30), c)
        return c

    def aggregate():
        a = (x @ c0.T).argmax(1)
        slot = image * K + a
        s = torch.zeros((n_images * K, D), device=dev).index_add_(0, slot, x)
        cnt = torch.zeros(n_images * K, device=dev).index_add_(0, slot, torch.ones(len(x), device=dev))
        v = s - cnt[:, None] * c0.repeat(n_images, 1)
        n = torch.linalg.norm(v, dim=1, keepdim=True)
        v = torch.where(n > 0, v / n.clamp_min(1e-30), v).reshape(n_images, K * D)
        nne = (n.reshape(n_images, K) > 0).sum(1, keepdim=True).clamp_min(1)
        return a, v / nne.sqrt()

    def select(g):
        sim = g @ g.T
        sim.fill_diagonal_(-float("inf"))
        return sim.topk(num_matched, dim=1).indices

    def timed(fn, *args):
        fn(*args)
        torch.cuda.synchronize()
        ms, out = [], None
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*args)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms, out

    t_train, _ = timed(train)
    t_agg, (a, g) = timed(aggregate)
    t_sel, top = timed(select, g)
    return {"train": t_train, "aggregate": t_agg, "topk": t_sel}, a.cpu().numpy().astype(np.int32), top.cpu().numpy().astype(np.int32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--descriptors", type=int, default=4096)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--clusters", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--max-train", type=int, default=262144)
    ap.add_argument("--num-matched", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from pixsfm_amd.engine import Context, VladVocabulary, retrieval_topk
    desc = make_descriptors(args.images, args.descriptors, args.dim)
    n_total = len(desc)
    offsets = np.arange(args.images + 1, dtype=np.int64) * args.descriptors
    ctx = Context(0)
    d_desc = ctx.to_device(desc, np.float32)
    train = lambda timed: VladVocabulary.train(ctx, d_desc, args.clusters, args.iterations, args.max_train, timed=timed)   # noqa: E731
    voc = train(False)                                                   # warm-up (allocates the workspace)
    g = voc.aggregate(d_desc, offsets)
    self_ = np.arange(args.images, dtype=np.int32)
    retrieval_topk(ctx, g, g, args.num_matched, query_self=self_)
    ctx.sync()
    kernels, wall = {}, {"train": [], "aggregate": [], "topk": []}

    def record(step, t0, ms):
        ctx.sync()
        wall[step].append(1e3 * (time.perf_counter() - t0))
        for name, v in ms.items():
            kernels.setdefault(step + "." + name, []).append(v)

    def loop():
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            record("train", t0, train(True).kernel_ms)
            t0 = time.perf_counter()
            voc.aggregate(d_desc, offsets, timed=True)
            record("aggregate", t0, voc.kernel_ms)
            t0 = time.perf_counter()
            record("topk", t0, retrieval_topk(ctx, g, g, args.num_matched, query_self=self_, timed=True)[3])

    telemetry = None
    try:
        import bench
        telemetry = bench.GpuTelemetry(0).sample_while(loop, interval=0.002)
    except Exception as e:  # noqa: BLE001
        telemetry = {"note": "no telemetry: %r" % (e,)}
        if not wall["train"]:
            loop()
    _, d_assign, d_counts = voc.aggregate(d_desc, offsets, details=True)
    assign, counts = d_assign.download(), d_counts.download()
    top, _, found = (a.download() for a in retrieval_topk(ctx, g, g, args.num_matched, query_self=self_))

    med = {name: stats(v)["median"] for name, v in kernels.items()}
    K, D = args.clusters, args.dim
    assign_flop = 2.0 * n_total * K * D
    n_cblocks = -(-K // min(K, 8192 // D))
    acc_bytes = float(n_total) * (D * 4 + 8) * n_cblocks                  # the rows and their assignments (read twice), per block of centroids
    sim_flop = 2.0 * args.images * args.images * K * D
    props_cus = 256
    try:
        import torch
        props_cus = torch.cuda.get_device_properties(0).multi_processor_count
    except Exception:  # noqa: BLE001
        pass
    sclk = ((telemetry or {}).get("sclk_mhz") or {}).get("mean")
    n_pairs = int(found.sum())
    result = {
        "scene": {"images": args.images, "descriptors_per_image": args.descriptors, "dim": D, "n_clusters": K, "n_iterations": args.iterations,
                  "max_train": args.max_train, "num_matched": args.num_matched, "global_dim": K * D},
        "kernel_ms": {name: stats(v) for name, v in kernels.items()},
        "kernels_total_ms": {step: sum(v for n, v in med.items() if n.startswith(step + ".")) for step in wall},
        "call_wall_ms": {step: stats(v) for step, v in wall.items()},
        "n_empty_clusters": voc.n_empty, "rows_unassigned": int((assign < 0).sum()), "rows_counted": int(counts.sum()),
        "pairs_retrieved": n_pairs, "pairs_exhaustive": args.images * (args.images - 1) // 2,
        "assign_flop": assign_flop, "assign_tflops": assign_flop / (med["aggregate.assign"] * 1e-3) * 1e-12,
        "accumulate_bytes": acc_bytes, "accumulate_centroid_blocks": n_cblocks,
        "accumulate_bytes_per_second": acc_bytes / (med["aggregate.accumulate"] * 1e-3),
        "accumulate_fraction_of_hbm": acc_bytes / (med["aggregate.accumulate"] * 1e-3) / HBM_BYTES_PER_SECOND,
        "similarity_tflops": sim_flop / (med["topk.similarity"] * 1e-3) * 1e-12,
        "telemetry": telemetry, "compute_units": props_cus,
    }
    if sclk:
        peak = props_cus * 4 * 64.0 * sclk * 1e6                        # FLOP/s: 4096 FLOP per 64 cycles per SIMD
        result["f32_mfma_peak_tflops_at_sampled_clock"] = peak * 1e-12
        result["assign_fraction_of_f32_mfma_peak"] = assign_flop / (med["aggregate.assign"] * 1e-3) / peak
        result["similarity_fraction_of_f32_mfma_peak"] = sim_flop / (med["topk.similarity"] * 1e-3) / peak
    if not args.no_torch:
        n_train = min(n_total, args.max_train)
        rows = np.arange(n_train, dtype=np.int64) * n_total // n_train
        ms, t_assign, t_top = torch_steps(desc, args.images, voc.centroids, rows, args.iterations,
                                          args.num_matched, max(3, args.repeats // 2))
        ours = {(i, int(j)) for i in range(len(top)) for j in top[i] if j >= 0}
        theirs = {(i, int(j)) for i in range(len(t_top)) for j in t_top[i]}
        result["torch"] = {"ms": {k: stats(v) for k, v in ms.items()},
                           "assignments_differing_from_ours": int((t_assign != assign).sum()), "rows": int(n_total),
                           "pairs_not_in_ours": len(theirs - ours), "pairs": len(theirs)}
        result["torch_over_ours_time"] = {k: stats(v)["median"] / result["kernels_total_ms"][k] for k, v in ms.items()}
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
