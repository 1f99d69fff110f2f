#!/usr/bin/env python3
"""The batched query bundle adjustment at localization sizes (csrc/pxr_query_ba.hip).

    python tools/bench_query_ba.py --out profiles/query_ba_bench.json

Part 1 (the kernel): --queries 256 queries x --blocks 200 residual blocks, 128 channels, fp16 patches of 16 x 16, poses perturbed as
in the tests (0.3 degrees, 0.02).  The queries are --images 32 synthetic images, each under queries / images different perturbed
poses: the queries of one image read the same patches.  pxr_query_ba_solve_timed: one warm-up, then the median of --repeats 5
HIP-event times, every run from the same start poses.  Reported: ms per launch, queries / s, LM iterations / s, and the stencil
bytes the evaluations read per second next to the HBM rate the microarchitecture guide calls achievable -- the 200 stencils of a
query (0.8 MB) stay in L2 across its iterations, so that ratio says how far the launch is from being bound by moving texels
at all, not how much HBM traffic there was.
Next to it the unchanged per-query path: QueryBundleOptimizer.run in a loop on --baseline 16 of the same queries in the same
process (wall time, one warm-up query), EXTRAPOLATED to all queries; and QueryBundleOptimizer.run_batch on all of them (wall
time: the observation lists, one arena upload, the launch).
Part 2 (end to end): QueryLocalizer.localize_batch against the localize() loop on the three queries of the test scene
(tests/test_query_ba_gpu.py), wall time split by stage.
One process.  Nobody has fixed a target for these numbers: this writes down what is measured."""
import argparse
import json
import os
import sys
import time
from copy import deepcopy

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("", "tests", "oracle", "pixel-perfect-sfm_amd"):
    sys.path.insert(0, os.path.join(ROOT, p))

HBM_ACHIEVABLE_GBS = 6300.0     # of the 8 TB/s peak, what a streaming copy reaches on an MI355X


def stats(values):
    v = sorted(float(x) for x in values)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def perturbed(rng, q, t, rot_deg=0.3, trans=0.02):
    ax = rng.normal(0, 1, 3)
    ax /= np.linalg.norm(ax)
    ang = np.deg2rad(rot_deg) * rng.uniform(0.5, 1.0)
    w0, v0, w1, v1 = np.cos(ang / 2), np.sin(ang / 2) * ax, q[0], q[1:]
    return np.concatenate([[w0 * w1 - v0 @ v1], w0 * v1 + w1 * v0 + np.cross(v0, v1)]), t + rng.normal(0, trans, 3)


def kernel_part(ctx, args):
    from pixsfm_amd import synthetic
    from pixsfm_amd.api import QueryBundleOptimizer, features
    from pixsfm_amd.api.reconstruction import Camera
    from pixsfm_amd.engine import PatchArena, QueryBAProblem, interp_cfg, lm_options, make_loss
    n_img, per = args.images, args.queries // args.images
    assert per * n_img == args.queries
    full = synthetic.make_ba_problem(n_cams=n_img, n_points=int(args.blocks * n_img * 1.3 / 4), obs_per_point=4, seed=3, model=2,
                                     perturb=False)
    rng = np.random.default_rng(4)
    sels = []
    for im in range(n_img):
        sel = np.flatnonzero(full["obs_image"] == im)[:args.blocks]
        assert len(sel) == args.blocks, "image %d has only %d observations" % (im, len(sel))
        sels.append(sel)
    poses = [[perturbed(rng, full["gt_qvec"][im], full["gt_tvec"][im]) for _ in range(per)] for im in range(n_img)]
    order = [(im, k) for k in range(per) for im in range(n_img)]                                  # neighbours in the batch are different images
    T, B, C = args.queries, args.blocks, full["refs"].shape[1]
    prob = dict(query_offsets=np.arange(T + 1, dtype=np.int64) * B, obs_patch=np.concatenate([sels[im] for im, _ in order]),
                xyz=np.concatenate([full["gt_xyz"][full["obs_point"][sels[im]]] for im, _ in order]),
                refs=np.concatenate([full["refs"][full["obs_point"][sels[im]]] for im, _ in order]),
                qvec=np.array([poses[im][k][0] for im, k in order]), tvec=np.array([poses[im][k][1] for im, k in order]),
                query_camera=np.array([full["image_camera"][im] for im, _ in order], np.int32), cam_model=full["cam_model"],
                cam_params=full["cam_params"])
    arena = PatchArena.from_numpy(ctx, full["patches"], full["corners"], full["scales"])
    cfg, loss, opt = interp_cfg(), make_loss("cauchy", [0.25]), lm_options()
    ms, per_query = [], None
    for run in range(args.repeats + 1):                                                           # the first one is the warm-up
        qba = QueryBAProblem(ctx, arena, prob)
        per_query = qba.solve(cfg, loss, opt, timed=True)
        if run:
            ms.append(qba.kernel_ms["solve"])
    launch = stats(ms)
    iters = sum(s["iterations"] for s in per_query)
    evaluations = sum(s["iterations"] + 1 for s in per_query)                                    # at most: an invalid step evaluates nothing
    stencil_bytes = evaluations * B * 16 * C * full["patches"].dtype.itemsize
    sec = launch["median"] * 1e-3
    out = dict(queries=T, blocks=B, channels=C, dtype=str(full["patches"].dtype), images=n_img, launch_ms=launch,
               queries_per_s=T / sec, lm_iterations=iters, lm_iterations_per_s=iters / sec,
               terminations={str(k): sum(s["termination"] == k for s in per_query) for k in (0, 1, 2)},
               iterations_per_query=stats([s["iterations"] for s in per_query]),
               stencil_gbytes_per_s=stencil_bytes / sec * 1e-9, hbm_achievable_gbytes_per_s=HBM_ACHIEVABLE_GBS,
               stencil_rate_over_hbm=stencil_bytes / sec * 1e-9 / HBM_ACHIEVABLE_GBS,
               cost_ratio=stats([s["final_cost"] / s["initial_cost"] for s in per_query]))

    # the unchanged per-query path and the batched Python path on the same queries
    fmaps = [features.FeatureMap.from_arrays(full["patches"][sel], np.arange(B), full["corners"][sel], (1.0, 1.0)) for sel in sels]
    cams = [Camera(1, 2, 1000, 1000, full["cam_params"][full["image_camera"][im], :4].copy()) for im in range(n_img)]

    def query(im, k):
        pts = full["obs_point"][sels[im]]
        return (poses[im][k][0].copy(), poses[im][k][1].copy(), deepcopy(cams[im]), [full["gt_xyz"][p] for p in pts], fmaps[im],
                [full["refs"][p] for p in pts])
    solver = QueryBundleOptimizer(ctx=ctx)
    solver.run(*query(*order[0]))                                                                 # warm-up
    walls, base_iters = [], 0
    for im, k in order[:args.baseline]:
        q = query(im, k)
        t0 = time.perf_counter()
        solver.run(*q)
        ctx.sync()
        walls.append(1e3 * (time.perf_counter() - t0))
        base_iters += solver.last_summary["iterations"]
    out["per_query_path"] = dict(measured_queries=len(walls), ms_per_query=stats(walls), lm_iterations=base_iters,
                                 extrapolated_ms_for_all=float(np.mean(walls)) * T, extrapolated=True)
    batch = [query(im, k) for im, k in order]
    solver.run_batch(batch[:2])                                                                   # warm-up
    batch = [query(im, k) for im, k in order]
    t0 = time.perf_counter()
    solver.run_batch(batch)
    ctx.sync()
    out["run_batch_wall_ms"] = 1e3 * (time.perf_counter() - t0)
    out["run_batch_path"] = solver.last_batch_path
    out["speedup_launch_over_extrapolated_loop"] = out["per_query_path"]["extrapolated_ms_for_all"] / launch["median"]
    out["speedup_run_batch_over_extrapolated_loop"] = out["per_query_path"]["extrapolated_ms_for_all"] / out["run_batch_wall_ms"]
    arena.close()
    return out


class Stages:
    """Wall time per stage: the named callables of the objects are wrapped for the duration of a `with`."""

    def __init__(self, ctx, targets):
        self.ctx, self.targets, self.ms = ctx, targets, {}

    def __enter__(self):
        self.saved = []
        for stage, obj, name in self.targets:
            fn = getattr(obj, name)
            self.saved.append((obj, name, fn))
            setattr(obj, name, self._timed(stage, fn))
        return self

    def _timed(self, stage, fn):
        def call(*a, **k):
            t0 = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                self.ctx.sync()
                self.ms[stage] = self.ms.get(stage, 0.0) + 1e3 * (time.perf_counter() - t0)
        return call

    def __exit__(self, *exc):
        for obj, name, fn in self.saved:
            setattr(obj, name, fn)


def end_to_end_part(ctx, args):
    import test_query_ba_gpu as tq
    from pixsfm_amd.api import localization
    s = tq.make_scene(ctx)
    loc, qs = s["localizer"], s["queries"]
    as_dict = lambda q: tq._as_dict(s, q)                                                         # noqa: E731

    def loop():
        return [loc.localize(q["keypoints"].copy(), q["kp_idx"], q["p3d_id"], deepcopy(s["camera"]), query_fmaps=[q["fmap"]]) for q in qs]

    def batch():
        return loc.localize_batch([as_dict(q) for q in qs])
    out = {}
    for name, run, targets in (
            ("localize_loop", loop, [("references", loc, "get_query_references"), ("qka", loc.query_keypoint_adjuster, "refine_multilevel"),
                                     ("pnp", localization, "absolute_pose_estimation"), ("qba", loc.query_bundle_adjuster, "refine_multilevel")]),
            ("localize_batch", batch, [("references", loc, "get_query_references"), ("qka", loc.query_keypoint_adjuster, "refine_batch"),
                                       ("pnp", localization, "absolute_pose_estimation_batch"),
                                       ("qba", loc.query_bundle_adjuster, "refine_multilevel_batch")])):
        run()                                                                                     # warm-up
        rows = []
        for _ in range(args.repeats):
            with Stages(ctx, targets) as st:
                t0 = time.perf_counter()
                res = run()
                ctx.sync()
                rows.append(dict(st.ms, wall=1e3 * (time.perf_counter() - t0)))
            assert all(r["success"] for r in res)
        out[name] = {k: stats([r[k] for r in rows]) for k in rows[0]}
    out["queries"] = len(qs)
    out["pairs_per_query"] = [len(q["kp_idx"]) for q in qs]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=200)
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--baseline", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pixsfm_amd.engine import Context
    ctx = Context(0)
    result = {"kernel": kernel_part(ctx, args), "end_to_end": end_to_end_part(ctx, args)}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
