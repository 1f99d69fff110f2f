#!/usr/bin/env python
"""bench.py -- featuremetric residual+Jacobian throughput on the synthetic 1M-observation BA
problem (BASELINE.json config 3: 200 cams / 200k points / 1M obs, 128-ch fp16 16x16 patches).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A plain run measures the headline only: it builds the scene, settles the clocks, runs the W warm-up steps, times the K steps,
writes the last step's records if --dump-outputs is given, and prints the line.  --full adds everything else this script
measures after the headline (clocks / power, k_jac, the Gram-matrix evaluation, LM iterations/s and the 8-GPU model, cost maps,
the CPU baselines, keypoint adjustment, the drop-in API calls, the per-rank table) and writes bench_detail.json.

--dump-outputs DIR: after the timed steps, the records of the last step (the n_obs x 8 float64 array pxr_ba_eval hands its
caller, include/pixsfm_hip.h) go to DIR as .npy files: a fixed, seeded sample of 2^18 rows (`records_sample.npy`) with its
row indices (`records_sample_index.npy`) and the column sums over every row (`records_column_sum.npy`), all float64.  The
scene is seeded, so the same arguments give the same inputs in every run.  With several ranks each rank writes its own
shard's files, suffixed `.rank<r>`.

A "step" = one fused residual+Jacobian evaluation (pxr_ba_eval, with_jacobian=1) of every
observation owned by the rank: projection, bicubic interpolation of the patch stencil,
L2-normalisation with analytic gradient, reference subtraction and the six-scalar reduction
that stands in for the 128 x (10+K) Jacobian block.  Inputs are resident in HBM when the
timed region starts.  N > 1: points (with all their observations and patches) are
partitioned over the ranks, no data-path collective in the evaluation.  Default = STRONG scaling
(the target of BASELINE.json: the 1M-observation problem is sharded over the N ranks; the scene is bit for bit the
one-rank scene); --scaling weak lets every rank own --points points instead (N x 1M observations, cameras shared).
The LM loop's collective is the native RCCL all-reduce of the engine (pxr_comm_init; falls back to the
torch.distributed callback if the communicator cannot be created).

Launching: under torch.distributed.run (RANK / WORLD_SIZE in the environment) every process is one rank.  A PLAIN
`python bench.py --gpus N` (no RANK in the environment) spawns its N ranks itself -- one subprocess per GPU with
RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR=127.0.0.1 / MASTER_PORT set -- re-prints rank 0's JSON line last and
exits non-zero if any rank failed (the others are stopped: a rank left alone in a collective would hang).

Rank 0 prints ONE JSON line; see DESIGN.md section "Measurement" for the roofline and
cpu_baseline definitions.  With --full it carries, besides the contract's fields, `lm` / `lm_no_inner` (LM iterations/s
on the same problem), `ka` (BASELINE configs[1]) and `costmap` (the reference's low-memory strategy on the
same scene: cost-map extraction + cost-map BA).
"""
import argparse
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "pixel-perfect-sfm_amd"))

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec


def algorithmic_bytes_per_obs(C, K=4, elem=2):
    """stencil 16*C*sizeof(dtype) + reference C*8 + params 8*(10+K) + 4 indices."""
    return 16 * C * elem + C * 8 + 8 * (10 + K) + 16


# ---------------------------------------------------------------------------------------------------------------------
# launching: a plain `python bench.py --gpus N` is its own launcher
# ---------------------------------------------------------------------------------------------------------------------
def self_launch(argv, n_ranks):
    """Spawn `n_ranks` copies of this script (rank r on GPU r), wait, re-print rank 0's JSON line last.
    Returns the exit code: 0 only if every rank exited 0 and rank 0 printed its line."""
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out0 = tempfile.TemporaryFile(mode="w+")
    procs = []
    for r in range(n_ranks):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n_ranks), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), LOCAL_WORLD_SIZE=str(n_ranks))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # the host driver only supports dmabuf IPC (RCCL needs it)
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env,
                                      stdout=out0 if r == 0 else sys.stderr, stderr=sys.stderr))
    limit = float(os.environ.get("PXR_BENCH_LAUNCH_TIMEOUT", "3600"))
    t0, failed = time.time(), None
    while True:
        codes = [p.poll() for p in procs]
        bad = [(r, c) for r, c in enumerate(codes) if c not in (None, 0)]
        if bad:
            failed = bad[0]
            break
        if all(c == 0 for c in codes):
            break
        if time.time() - t0 > limit:
            failed = (-1, 124)
            break
        time.sleep(0.1)
    if failed is not None:
        for p in procs:                      # exactly the processes started here, by handle
            if p.poll() is None:
                p.terminate()
        deadline = time.time() + 10
        for p in procs:
            try:
                p.wait(timeout=max(0.1, deadline - time.time()))
            except subprocess.TimeoutExpired:
                p.kill()
                p.wait()
        print("bench.py launcher: %s -- the other ranks were stopped" %
              ("timed out after %.0f s" % limit if failed[0] < 0 else "rank %d exited with code %d" % failed), file=sys.stderr)
        return failed[1] if 0 < failed[1] < 256 else 1
    out0.seek(0)
    lines = out0.read().splitlines()
    last = max((i for i, l in enumerate(lines) if l.startswith("{") and l.rstrip().endswith("}")), default=None)
    for i, l in enumerate(lines):
        if i != last:
            print(l, file=sys.stderr)
    if last is None:
        print("bench.py launcher: rank 0 printed no JSON line", file=sys.stderr)
        return 1
    sys.stderr.flush()
    print(lines[last], flush=True)
    return 0


def _selftest_hooks(rank):
    """PXR_BENCH_SELFTEST="fail:R" / "hang:R" / "ok:R" / "watchdog:R" (comma separated): rank R exits with code 3 / sleeps / prints a
    line and exits 0 / arms the Watchdog and then sleeps, before any GPU work.
    Lets tests/ exercise the launcher's failure path on a box without a GPU."""
    for item in filter(None, os.environ.get("PXR_BENCH_SELFTEST", "").split(",")):
        what, _, who = item.partition(":")
        if who != "" and int(who) == rank:
            if what == "fail":
                raise SystemExit(3)
            if what == "hang":
                time.sleep(600)
            if what == "ok":
                print(json.dumps({"selftest": True, "rank": rank}))
                raise SystemExit(0)
            if what == "watchdog":        # a leg that never returns: the timer prints rank 0's line and ends the rank with code 0
                Watchdog(0.5, rank, lambda: print(json.dumps({"selftest": True, "watchdog": True, "rank": rank}), flush=True))
                time.sleep(600)


# ---------------------------------------------------------------------------------------------------------------------
# clocks / power: what tells a slower box from a regression
# ---------------------------------------------------------------------------------------------------------------------
class GpuTelemetry:
    """Samples the shader clock and the package power of one GPU from sysfs while a loop runs (amdgpu: pp_dpm_sclk marks
    the current level with '*', hwmon power1_average / power1_input are microwatts).  Everything is best effort: a field
    that cannot be read is reported as null."""

    def __init__(self, device_index):
        self.sclk_path = self.power_path = self.mclk_path = None
        self.note = None
        try:
            import torch
            bus = torch.cuda.get_device_properties(device_index).pci_bus_id
            dom = getattr(torch.cuda.get_device_properties(device_index), "pci_domain_id", 0)
            dev = getattr(torch.cuda.get_device_properties(device_index), "pci_device_id", 0)
            want = "%04x:%02x:%02x" % (dom, bus, dev)
        except Exception:  # noqa: BLE001
            want = None
        cards = sorted(glob.glob("/sys/class/drm/card[0-9]*/device"))
        pick = None
        for c in cards:
            if not os.path.exists(os.path.join(c, "pp_dpm_sclk")):
                continue
            real = os.path.realpath(c)
            if want and want in real:
                pick = c
                break
            if pick is None:
                pick = c
        if pick is None:
            self.note = "no amdgpu sysfs node with pp_dpm_sclk"
            return
        self.sclk_path = os.path.join(pick, "pp_dpm_sclk")
        if os.path.exists(os.path.join(pick, "pp_dpm_mclk")):
            self.mclk_path = os.path.join(pick, "pp_dpm_mclk")
        for name in ("power1_average", "power1_input"):
            hits = glob.glob(os.path.join(pick, "hwmon", "hwmon*", name))
            if hits:
                self.power_path = hits[0]
                break
        self.sysfs = pick

    @staticmethod
    def _current_mhz(path):
        try:
            with open(path) as fh:
                for line in fh:
                    if "*" in line:
                        m = re.search(r"(\d+)\s*[Mm][Hh]z", line)
                        if m:
                            return float(m.group(1))
        except OSError:
            pass
        return None

    def read(self):
        w = None
        if self.power_path:
            try:
                with open(self.power_path) as fh:
                    w = float(fh.read().strip()) * 1e-6
            except (OSError, ValueError):
                pass
        return (self._current_mhz(self.sclk_path) if self.sclk_path else None,
                self._current_mhz(self.mclk_path) if self.mclk_path else None, w)

    def sample_while(self, fn, interval=0.01):
        """Runs fn() while a thread samples; returns the summary dict."""
        rows, stop = [], threading.Event()

        def loop():
            while not stop.is_set():
                rows.append(self.read())
                time.sleep(interval)
        th = threading.Thread(target=loop, daemon=True)
        th.start()
        try:
            fn()
        finally:
            stop.set()
            th.join()

        def stats(k):
            v = [r[k] for r in rows if r[k] is not None]
            return None if not v else {"min": min(v), "mean": sum(v) / len(v), "max": max(v)}
        return {"samples": len(rows), "sclk_mhz": stats(0), "mclk_mhz": stats(1), "power_w": stats(2),
                "source": getattr(self, "sysfs", None), "note": self.note}


# ---------------------------------------------------------------------------------------------------------------------
# CPU legs (rank 0, one GPU): the oracle / the reference's own code on the host cores, timed inside C
# ---------------------------------------------------------------------------------------------------------------------
def cpu_baseline(prob, patches, n_sample, lm_gauge=None):
    """The CPU legs on a bounded sample of the same workload (whole points: the first n_sample observations' points with
    all their observations; every camera), each timed INSIDE C by the persistent-thread harness of
    oracle/pxo_bench_harness.h over {cores/4, cores/2, cores, 2 x cores} threads (best reported, with the single-thread
    rate, the scaling efficiency and the harness_limited guard):
      cpu_baseline          kind "port": the oracle's C restatement (AVX2 / F16C spline, analytic 128 x (10+K) Jacobians
                            materialised like ceres::AutoDiffCostFunction hands them over, + loss), threaded over blocks
                            like Ceres (bundle_adjustment_options.h:58).  The reference's own C++ cannot be built in this
                            image (no Eigen / Ceres / COLMAP), so there is no kind "reference" leg;
      cpu_baseline_lm_projected  one LM iteration of the oracle's Schur path (oracle/pxo_lm_bench.c, OpenMP), the
                            per-observation stages scaled to the full problem, the Cholesky not."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import pxo
    import pxo_cpubench
    n_obs = len(prob["obs_image"])
    n_pts_s = int(prob["obs_point"][min(n_sample, n_obs) - 1]) + 1          # whole points (observations are point-sorted)
    n_sample = int(np.searchsorted(prob["obs_point"], n_pts_s, side="left")) if n_pts_s < len(prob["xyz"]) else n_obs
    sub = dict(prob)
    for k in ("obs_image", "obs_point", "obs_patch", "corners", "scales"):
        sub[k] = prob[k][:n_sample]
    sub["xyz"], sub["refs"] = prob["xyz"][:n_pts_s], prob["refs"][:n_pts_s]
    sub["patches"] = patches[:n_sample].cpu().numpy()
    host = np.zeros((len(prob["cam_model"]), 12)); host[:, :prob["cam_params"].shape[1]] = prob["cam_params"]
    sub["cam_params"] = host
    touched_mb = n_sample * (16 * 128 * 2 + 128 * 8 / 5) / 1e6
    cfg, ls = pxo.cfg(), pxo.loss("cauchy", 0.25)
    what = ("first %d observations (%d whole points, all %d cameras) of the same workload; every thread works on its own "
            "first-touched copy of its share; touched working set %.0f MB of stencils + references"
            % (n_sample, n_pts_s, len(prob["image_camera"]), touched_mb))
    out = {"cpu_host": pxo_cpubench.host_probe()}
    port = pxo_cpubench.ba_eval_port(sub, cfg, ls)
    port["sample"] = what + "; oracle C restatement: analytic 128x(10+K) Jacobians materialised + Cauchy loss"
    out["cpu_baseline"] = port
    # ---- one LM iteration on the host cores (OpenMP; the thread count that won the evaluation sweep) -----------------
    if lm_gauge is not None:
        pose_const, tmask, cmask = lm_gauge
        threads = int(out["cpu_baseline"]["cores"])
        best = None
        t0 = time.perf_counter()
        for _ in range(3):
            r = pxo.ba_lm_iteration_schur(sub, cfg, ls, pose_const, tmask, cmask, np.zeros(n_pts_s, np.uint8), radius=1e4,
                                          n_threads=threads, want_step=False)
            if best is None or r["total_ms"] < best["total_ms"]:
                best = r
            if time.perf_counter() - t0 > 10.0:
                break
        scale = n_obs / n_sample
        per_obs_ms = best["jacobian_eval_ms"] + best["schur_ms"] + best["backsub_ms"] + best["cost_eval_ms"]
        full_ms = per_obs_ms * scale + best["cholesky_ms"]
        out["cpu_baseline_lm_projected"] = {
            "value": 1e3 / full_ms, "unit": "LM iterations/s (PROJECTED from the sample, see `sample`)", "cores": threads, "kind": "port",
            "ms_per_iteration_projected": full_ms, "rc": best["rc"], "reduced_system": best["n_c"],
            "measured_on_sample_ms": {k: best[k] for k in ("jacobian_eval_ms", "schur_ms", "cholesky_ms", "backsub_ms",
                                                           "cost_eval_ms", "total_ms")},
            "sample": "one LM iteration (best of <= 3, stage times taken inside C) on the first %d observations (%d whole points, "
                      "all %d cameras) of the same workload, oracle C restatement with OpenMP over observations / points "
                      "(%d threads; Schur elimination with <= 32 private copies of S, blocked Cholesky); projected to the full "
                      "problem: per-observation stages x %.1f, Cholesky of the same %d x %d system unchanged; no inner iterations"
                      % (n_sample, n_pts_s, len(prob["image_camera"]), threads, scale, best["n_c"], best["n_c"])}
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the GPU legs
# ---------------------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cams", type=int, default=200)
    ap.add_argument("--points", type=int, default=200_000)
    ap.add_argument("--obs-per-point", type=int, default=5)
    ap.add_argument("--float-simd", action="store_true", help="InterpolationConfig.use_float_simd")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-sample", type=int, default=131072,
                    help="observations of the CPU legs' sample (131072 -> 8.6 GB of patches, 0.5 GB touched: beyond the L3 of the box)")
    ap.add_argument("--lm-iters", type=int, default=10, help="LM iterations for the iters/s figure (0 = skip)")
    ap.add_argument("--no-ka", action="store_true", help="skip the keypoint-adjustment half of the metric (BASELINE configs[1])")
    ap.add_argument("--no-ka-points", action="store_true", help="skip the keypoint adjustment's other operating points (1000 per group, one problem, low_memory.yaml)")
    ap.add_argument("--no-costmap", action="store_true", help="skip the cost-map extraction / cost-map BA figures")
    ap.add_argument("--scaling", choices=("weak", "strong"), default="strong",
                    help="strong (default, BASELINE.json's target): --points points in total, sharded over the ranks; "
                         "weak: every rank owns --points points (N x the observations, cameras shared)")
    ap.add_argument("--patch-size", type=int, default=16, help="side of the square fp16 patches (16: pixsfm's default; 8: low_memory.yaml)")
    ap.add_argument("--preset", choices=("aachen",), default=None,
                    help="aachen: BASELINE.json configs[4]-shaped scene on ONE GPU -- 4000 cameras, 1M points, 5M observations, 8 x 8 "
                         "fp16 patches (82 GB; the reference runs Aachen with configs/low_memory.yaml: patch_size 8), iterative "
                         "solver by image count, cost-map strategy beside it; KA / CPU legs / API timing are skipped")
    ap.add_argument("--no-api-e2e", action="store_true",
                    help="skip the end-to-end timing of the drop-in API calls on host-resident inputs (tools/bench_api_e2e.py)")
    ap.add_argument("--no-telemetry", action="store_true", help="skip the clock / power sampling loop")
    ap.add_argument("--detail-out", default=os.path.join(ROOT, "bench_detail.json"),
                    help="where the full result goes (sweeps, cgroup dumps, phase tables); the printed line is its compact form")
    ap.add_argument("--linear-solver", default="auto", help="auto (by image count, bundle_optimizer.h:180-191) | direct | iterative")
    ap.add_argument("--watchdog-s", type=float, default=float(os.environ.get("PXR_BENCH_WATCHDOG_S", "420")),
                    help="several ranks only: if the legs after the headline measurement (LM, KA) do not finish within this many seconds "
                         "-- a collective that never returns -- rank 0 prints the line with what it has and every rank exits 0; 0 disables")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, run every other leg (telemetry, k_jac, Gram-matrix evaluation, LM, scaling model, cost maps, "
                         "CPU baselines, KA, drop-in API calls) and write --detail-out; a plain run measures the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's records to DIR as .npy (a seeded sample of rows, their indices, column sums)")
    args = ap.parse_args(argv)
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.preset == "aachen":
        args.cams, args.points, args.obs_per_point, args.patch_size = 4000, 1_000_000, 5, 8
        args.no_ka = args.no_api_e2e = args.no_cpu_baseline = True
    return args


class Job:
    """One rank's view of the run: process group, device, context."""

    def __init__(self, args):
        import torch
        self.args = args
        self.rank = int(os.environ.get("RANK", "0"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        if self.world != args.gpus:
            raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, self.world))
        # PXR_BENCH_ONE_DEVICE=1 + PXR_BENCH_BACKEND=gloo: several ranks on ONE GPU, used to validate the
        # multi-process flow (sharding, barriers, max-over-ranks timing, all-reduce callback) on a 1-GPU box
        if os.environ.get("PXR_BENCH_ONE_DEVICE") == "1":
            self.local_rank = 0
        torch.cuda.set_device(self.local_rank)
        self.dev = "cuda:%d" % self.local_rank
        # PXR_BENCH_FORCE_DIST=1 exercises the RCCL code path with a single rank
        self.dist_on = self.world > 1 or os.environ.get("PXR_BENCH_FORCE_DIST") == "1"
        self.backend = None
        if self.dist_on:
            import torch.distributed as dist
            if "MASTER_ADDR" not in os.environ:
                os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", "29531"
            self.backend = os.environ.get("PXR_BENCH_BACKEND", "nccl")          # "nccl" IS RCCL on ROCm
            if self.backend == "nccl":
                dist.init_process_group("nccl", rank=self.rank, world_size=self.world, device_id=torch.device(self.dev))
            else:
                dist.init_process_group(self.backend, rank=self.rank, world_size=self.world)
        from pixsfm_amd.engine import Context
        self.ctx = Context(self.local_rank, stream=torch.cuda.current_stream().cuda_stream)
        self.collective = "none"
        if self.dist_on:
            self._init_collective()

    def _init_collective(self):
        import numpy as np
        import torch
        import torch.distributed as dist
        from pixsfm_amd import parallel
        from pixsfm_amd.engine import Context
        ctx, rank, world = self.ctx, self.rank, self.world
        self.collective = "torch.distributed callback (%s)" % self.backend
        if self.backend == "nccl" and os.environ.get("PXR_BENCH_CALLBACK") != "1":
            ok = 1
            try:
                if world > 1:
                    parallel.init_native_comm(ctx)
                else:
                    ctx.comm_init(Context.comm_unique_id(), 0, 1)
                    ctx.comm_force(True)      # one rank: the solvers still run pack -> ncclAllReduce -> unpack (pxr_comm_force)
                probe = ctx.to_device(np.full(4, float(rank + 1)), np.float64)      # one real all-reduce before relying on it
                ctx.allreduce_sum(probe)
                ctx.sync()
                if not np.array_equal(probe.download(), np.full(4, world * (world + 1) / 2.0)):
                    raise RuntimeError("native all-reduce returned %r" % (probe.download(),))
            except Exception as e:  # noqa: BLE001 -- keep the bench alive on the callback path
                ok = 0
                print("rank %d: native communicator unavailable (%r)" % (rank, e), file=sys.stderr)
            # every rank must take the same path: one rank on the callback while the others wait in ncclAllReduce would hang
            flag = torch.tensor([ok], device=self.dev, dtype=torch.int32)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            if int(flag.item()) == 1:
                self.collective = "native ncclAllReduce on the engine's stream (pxr_comm_init)"
            else:
                if ok:
                    ctx.comm_destroy()
                if world > 1:
                    ctx.comm_set_rank(rank, world)
                if rank == 0:
                    print("using the torch.distributed callback on every rank", file=sys.stderr)
        elif world > 1:
            ctx.comm_set_rank(rank, world)

    @property
    def native(self):
        return self.collective.startswith("native")

    def barrier(self):
        import torch
        if self.dist_on:
            import torch.distributed as dist
            dist.barrier()
        torch.cuda.synchronize()

    def reduce(self, value, op="sum"):
        """A python float reduced over the ranks."""
        if not self.dist_on:
            return value
        import torch
        import torch.distributed as dist
        t = torch.tensor([value], dtype=torch.float64, device=self.dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX if op == "max" else dist.ReduceOp.SUM)
        return t.item()

    def solve_allreduce(self):
        """The callback BAProblem.solve needs on the non-native path (None: the engine's own communicator)."""
        if not self.dist_on or self.native:
            return None
        from pixsfm_amd.parallel import make_allreduce
        return make_allreduce()


def default_gauge(n_img, n_pts):
    """Default gauge (bundle_adjustment/main.py:12-18) and refine flags (bundle_adjustment_options.h:66-76)."""
    import numpy as np
    pose_const = np.zeros(n_img, np.uint8); pose_const[0] = 1
    tmask = np.zeros(n_img, np.uint8); tmask[1] = 1
    cmask = np.full(n_img, 0b0110, np.uint16)          # SIMPLE_RADIAL: refine f and k, keep cx, cy
    return pose_const, tmask, cmask, np.zeros(n_pts, np.uint8)


def reset_parameters(ba, prob):
    import numpy as np
    for name in ("qvec", "tvec", "xyz"):
        ba.d[name].upload(prob[name])
    host = np.zeros((len(prob["cam_model"]), 12)); host[:, :prob["cam_params"].shape[1]] = prob["cam_params"]
    ba.d["cam_params"].upload(host)


def run_eval(job, ba, cfg):
    """The headline: K timed evaluations between barriers; HIP events on the launch stream for the kernel time."""
    args, ctx = job.args, job.ctx
    # clock settle (untimed, BEFORE the W warm-up steps, disclosed as `settle_launches` in the line): the GPU comes out of the
    # host-side problem construction at idle clocks and needs ~0.1-0.2 s of load to reach its sustained state; W = 5 and K = 20
    # steps are 21 ms -- the driver's round-5 record read 0.871 ms in that window and 0.811 ms for the SAME kernel in the 0.4 s
    # telemetry loop of the same run.  PXR_BENCH_SETTLE_S=0 switches it off.
    settle_s = float(os.environ.get("PXR_BENCH_SETTLE_S", "0.25"))
    job.settle_launches = 0
    t_settle = time.perf_counter()
    while settle_s > 0 and time.perf_counter() - t_settle < settle_s:
        for _ in range(10):
            ba.eval(cfg, with_jacobian=True)
        ctx.sync()
        job.settle_launches += 10
    for _ in range(args.warmup):
        ba.eval(cfg, with_jacobian=True)
    job.barrier()
    t0 = time.perf_counter()
    ctx.timer_start()
    for _ in range(args.steps):
        ba.eval(cfg, with_jacobian=True)
    kernel_ms = ctx.timer_stop() / args.steps            # HIP events on the launch stream
    job.barrier()
    dt = job.reduce(time.perf_counter() - t0, "max")
    return dt, kernel_ms


def run_telemetry(job, ba, cfg):
    """~0.4 s of the same launches back to back while a thread samples the shader clock / power (the 44 ms timed region is
    too short to sample); the kernel time of THIS loop is reported beside the samples."""
    ctx = job.ctx
    tel = GpuTelemetry(job.local_rank)
    reps = 400
    box = {}

    def loop():
        ctx.timer_start()
        for _ in range(reps):
            ba.eval(cfg, with_jacobian=True)
        box["ms"] = ctx.timer_stop() / reps
    idle = tel.read()
    out = tel.sample_while(loop)
    out["kernel_ms_in_this_loop"] = box.get("ms")
    out["launches"] = reps
    out["idle_before"] = {"sclk_mhz": idle[0], "mclk_mhz": idle[1], "power_w": idle[2]}
    return out


def run_gram(job, ba, cfg):
    """The evaluation of the LM loop with the Gram-matrix cache on its own (pxr_ba_eval_gram): the build of every observation's
    16 x 16 Gram matrix (32 fp64 MFMAs per observation: bound by the matrix pipe) and the steady-state pass from the cache
    (1 408 + 64 B per observation: HBM-bound), with the shader clock / power sampled while the build loops."""
    ctx = job.ctx
    out = {}
    ba.eval_gram(cfg, reset=True)
    ctx.sync()
    reps = 5
    ctx.timer_start()
    for _ in range(reps):
        ba.eval_gram(cfg, reset=True, sync=False)
    out["build_and_evaluate_ms"] = ctx.timer_stop() / reps
    reps = 50
    ctx.timer_start()
    for _ in range(reps):
        ba.eval_gram(cfg, reset=False, sync=False)
    out["evaluate_from_cache_ms"] = ctx.timer_stop() / reps
    bytes_per_obs = 176 * 8 + 64
    out["evaluate_from_cache_GBps"] = bytes_per_obs * ba.n_obs / (out["evaluate_from_cache_ms"] * 1e-3) / 1e9
    out["cache_bytes_per_obs"] = 176 * 8
    out["roofline"] = {"bound": "hbm", "achieved": out["evaluate_from_cache_GBps"], "peak": 8000.0, "unit": "GB/s",
                       "frac": out["evaluate_from_cache_GBps"] / 8000.0, "kernel": "k_gram_eval",
                       "algorithmic_bytes_per_obs": bytes_per_obs,
                       "note": "1 408 B of cached Gram matrix + D, 64 B record; counter traffic of the kernel: profiles/r4_hot_kernels_pmc.json"}
    # the build: 32 v_mfma_f64_16x16x4 (2 048 flop each) per observation against the fp64 matrix rate this hardware sustains
    # (tools/micro/mfma_f64_rate.hip: 44 TFLOP/s; the data sheet's dense fp64 matrix peak is 78.6)
    build_ms = max(out["build_and_evaluate_ms"] - out["evaluate_from_cache_ms"], 1e-9)
    out["build_roofline"] = {"bound": "mfma", "achieved": 32 * 2048 * ba.n_obs / (build_ms * 1e-3) / 1e12, "peak": 78.6, "unit": "TFLOP/s",
                             "frac": 32 * 2048 * ba.n_obs / (build_ms * 1e-3) / 1e12 / 78.6, "kernel": "k_gram_build (+ the second evaluation pass)",
                             "sustained_rate_measured": 44.4}
    if job.rank == 0 and not job.args.no_telemetry:
        try:
            tel = GpuTelemetry(job.local_rank)

            def loop():
                for _ in range(60):
                    ba.eval_gram(cfg, reset=True, sync=False)
                ctx.sync()
            t = tel.sample_while(loop)
            out["build_loop_sclk_mhz"] = t["sclk_mhz"]
            out["build_loop_power_w"] = t["power_w"]
        except Exception as e:  # noqa: BLE001
            out["telemetry_error"] = repr(e)
    return out


def run_lm(job, ba, prob, cfg):
    """LM iterations / s on the same problem: "lm" = pixsfm's default configuration (use_inner_iterations = True,
    bundle_adjustment/main.py:43), "lm_no_inner" = the plain trust-region loop.  One iteration = linearise + Schur +
    Cholesky + back-substitution + evaluation at the trial point.  Same initial parameters for both."""
    import numpy as np
    from pixsfm_amd.engine import lm_options, make_loss
    args, ctx = job.args, job.ctx
    lm, extra = {}, {}
    if args.lm_iters <= 0:
        return lm, extra
    n_img = args.cams
    pose_const, tmask, cmask, ptc = default_gauge(n_img, len(prob["xyz"]))
    # untimed warm-up, like the W steps of the headline: the FIRST pxr_ba_solve of a process pays for loading ~40 kernels' code
    # objects, the 1.4 GB Gram-matrix cache and the pinned staging buffers (measured: 9.4 ms of set-up against 2.0 ms for every
    # later solve -- outside total_ms -- and 1.7 ms more inside it, tools/_lm_setup_probe.py) -- a two-iteration solve takes that,
    # its own time is reported as `first_solve_of_the_process`
    reset_parameters(ba, prob)
    job.barrier()
    first = ba.solve(cfg, make_loss("cauchy", [0.25]), pose_const, tmask, cmask, ptc,
                     options=lm_options(max_iterations=2, use_inner_iterations=True, linear_solver=args.linear_solver),
                     allreduce=job.solve_allreduce())
    extra["first_solve_of_the_process"] = {"iterations": first["iterations"], "total_ms": first["total_ms"], "setup_ms": first["setup_ms"],
                                           "note": "untimed warm-up before the lm / lm_no_inner solves"}
    for key, inner in (("lm", True), ("lm_no_inner", False)):
        reset_parameters(ba, prob)
        job.barrier()
        if job.dist_on and "allreduce_ms" not in extra:
            # the collective of the direct solver on its own: the packed upper triangle of [S | rhs], n_c (n_c + 3) / 2 doubles,
            # n_c = 8 per camera - 7 gauge columns (round 3 moved the full (n_c + 1)^2 square: twice the bytes)
            n_c = 8 * n_img - 7
            count = n_c * (n_c + 3) // 2
            buf = ctx.to_device(np.zeros(count), np.float64)
            cb = job.solve_allreduce()
            one = (lambda: ctx.allreduce_sum(buf)) if cb is None else (lambda: cb(buf.ptr.value, count))
            for _ in range(3):
                one()
            ctx.sync(); job.barrier()
            ctx.timer_start()
            for _ in range(10):
                one()
            extra["allreduce_ms"] = job.reduce(ctx.timer_stop() / 10, "max")
            extra["allreduce_bytes"] = int(count * 8)
            extra["allreduce_what"] = "packed upper triangle of [S | rhs] (n_c = %d), %s" % (n_c, job.collective)
            del buf
            job.barrier()
        if job.dist_on:
            ctx.comm_stats(reset=True)
        lm[key] = ba.solve(cfg, make_loss("cauchy", [0.25]), pose_const, tmask, cmask, ptc,
                           options=lm_options(max_iterations=args.lm_iters, use_inner_iterations=inner,
                                              linear_solver=args.linear_solver),
                           allreduce=job.solve_allreduce())
        if job.dist_on:      # what really went through the context's RCCL communicator during this solve
            calls, nbytes = ctx.comm_stats()
            lm[key]["native_collective_calls"], lm[key]["native_collective_bytes"] = int(calls), int(nbytes)
        job.barrier()
    # ---- what the defaults cost / buy: the same solves (a) once more -- the deterministic default must give the same bits --,
    # (b) with floating-point atomics (PXR_DETERMINISTIC=0), (c) with the evaluation from the texels instead of from the cached
    # Gram matrices (PXR_GRAM_CACHE=0: the exact-order kernel of the headline at every iteration)
    def solve(inner):
        reset_parameters(ba, prob)
        job.barrier()
        r = ba.solve(cfg, make_loss("cauchy", [0.25]), pose_const, tmask, cmask, ptc,
                     options=lm_options(max_iterations=args.lm_iters, use_inner_iterations=inner, linear_solver=args.linear_solver),
                     allreduce=job.solve_allreduce())
        job.barrier()
        return r

    def brief(r, ref):
        per = r["total_ms"] / max(1, r["iterations"])
        return {"ms_per_iter": per, "iterations": r["iterations"], "successful": r["num_successful"], "final_cost": r["final_cost"],
                "ratio_to_default": per / (ref["total_ms"] / max(1, ref["iterations"])),
                "final_cost_rel_diff": abs(r["final_cost"] - ref["final_cost"]) / max(ref["initial_cost"], 1e-300)}
    again = solve(True)
    extra["deterministic"] = {"on": bool(ctx.deterministic), "two_runs_bit_identical":
                              bool(again["final_cost"] == lm["lm"]["final_cost"] and again["num_successful"] == lm["lm"]["num_successful"])}
    was_det, was_gram = ctx.deterministic, ctx.gram_cache
    try:
        ctx.deterministic = False
        extra["nondeterministic"] = brief(solve(True), lm["lm"])
        ctx.deterministic = was_det
        ctx.gram_cache = False
        extra["texel_evaluation"] = brief(solve(True), lm["lm"])
        extra["no_inner_texel_evaluation"] = brief(solve(False), lm["lm_no_inner"])
    finally:
        ctx.deterministic, ctx.gram_cache = was_det, was_gram
    return lm, extra


def run_scaling_model(job, prob, patches, lm, cfg, measured_call_ms=None, full_step_ms=None):
    """What an 8-GPU LM iteration would cost, MODELLED from this GPU (no multi-GPU box is reachable from
    the build container): the same `lm` solve on the first eighth of the points (all cameras) -- the shard one of eight ranks
    would own -- gives T_shard; with T_1 the full solve, the part that does not shrink with the shard (the replicated reduced
    camera system: Cholesky, camera-side launches) is (8 T_shard - T_1) / 7.  The collective is ASSUMED, not measured: the packed
    [S | rhs] integers (n_c (n_c + 3) / 2 x 8 bytes) at an all-reduce bus bandwidth of 100 GB/s + 20 us."""
    import numpy as np
    from pixsfm_amd.engine import BAProblem, PatchArena, lm_options, make_loss
    args, ctx = job.args, job.ctx
    n_pts = len(prob["xyz"]) // 8
    n_obs = int(np.searchsorted(prob["obs_point"], n_pts, side="left"))
    sub = dict(prob)
    for k in ("obs_image", "obs_point", "obs_patch", "corners", "scales"):
        sub[k] = prob[k][:n_obs]
    sub["xyz"], sub["refs"] = prob["xyz"][:n_pts].copy(), prob["refs"][:n_pts].copy()
    arena = PatchArena(ctx, n_obs, args.patch_size, args.patch_size, 128, np.float16, device_ptr=patches.data_ptr())
    arena.upload(0, None, sub["corners"], sub["scales"])
    ba8 = BAProblem(ctx, arena, sub)
    pose_const, tmask, cmask, ptc = default_gauge(args.cams, n_pts)
    out = {}
    # metric 1 (`value`: no collective on that path) at 8 GPUs, strong scaling: the headline's step on the shard ONE of eight ranks
    # would own -- 1/8 of the points, every camera -- timed like the headline (K launches back to back, wall clock incl. the host's
    # launch loop, the GPU already at its sustained clocks): efficiency = (full step / 8) / shard step   
    if full_step_ms:
        for _ in range(20):
            ba8.eval(cfg, with_jacobian=True)
        ctx.sync()
        reps = 200
        t0 = time.perf_counter()
        ctx.timer_start()
        for _ in range(reps):
            ba8.eval(cfg, with_jacobian=True)
        k_ms = ctx.timer_stop() / reps
        w_ms = (time.perf_counter() - t0) * 1e3 / reps
        out["value"] = {"obs_per_gpu": int(n_obs), "full_step_ms": full_step_ms, "shard8_step_ms": w_ms, "shard8_kernel_ms": k_ms,
                        "efficiency_8gpu_modelled": full_step_ms / 8.0 / w_ms,
                        "note": "evaluation of the first 1/8 of the points on this GPU; no collective on this path, barriers not modelled"}
    for key, inner in (("lm", True), ("lm_no_inner", False)):
        best = None
        for _ in range(2):
            reset_parameters(ba8, sub)
            s = ba8.solve(cfg, make_loss("cauchy", [0.25]), pose_const, tmask, cmask, ptc,
                          options=lm_options(max_iterations=args.lm_iters, use_inner_iterations=inner, linear_solver=args.linear_solver))
            per = s["total_ms"] / max(1, s["iterations"])
            best = per if best is None else min(best, per)
        t1 = lm[key]["total_ms"] / max(1, lm[key]["iterations"])
        n_c = lm[key]["num_camera_unknowns"]
        # latency term: the ONE-rank ncclAllReduce of the same buffer measured through RCCL when the bench ran with
        # PXR_BENCH_FORCE_DIST=1 (launch + protocol overhead, no wire), else 20 us assumed; wire term: ring over 8 ranks at 100 GB/s
        # (a ONE-rank in-place ncclAllReduce is elided by RCCL -- ~1 us, no kernel --, so the measured call is only a floor: the
        #  20 us of a real multi-rank launch stay as the assumption unless the measurement is larger)
        lat_ms = max(measured_call_ms or 0.0, 0.02)
        coll_ms = n_c * (n_c + 3) / 2 * 8 * 2 * 7 / 8 / 100e9 * 1e3 + lat_ms
        out[key] = {"t1_ms": t1, "t_shard8_ms": best, "replicated_ms": max(0.0, (8 * best - t1) / 7), "allreduce_ms_assumed": coll_ms,
                    "allreduce_latency_ms": lat_ms, "one_rank_rccl_call_ms": measured_call_ms,
                    "efficiency_8gpu_modelled": t1 / (8 * (best + coll_ms))}
    out["note"] = ("modelled from one GPU: T_shard = the same solve on the first 1/8 of the points; collective = wire term assumed "
                   "(ring, 100 GB/s bus bandwidth) + 20 us call latency assumed (the one-rank RCCL call measured here is elided by RCCL: a floor only)")
    arena.close()
    return out


def run_costmap(job, ba, prob):
    """The reference's low-memory strategy on the same scene: cost-map extraction (one HBM-bound pass over
    the feature arena) and the cost-map BA (3-channel maps, no reference descriptor)."""
    import numpy as np
    from pixsfm_amd.engine import interp_cfg, lm_options, make_loss
    args, ctx = job.args, job.ctx
    C, PS = 128, args.patch_size
    n_obs_local = len(prob["obs_image"])
    reset_parameters(ba, prob)
    trivial = make_loss("trivial", [])
    cm = ba.extract_costmaps(trivial)                 # warm-up + the maps used below
    ctx.sync()
    reps = 20                                         # > 60 ms at 1M maps: the shader clock has settled (the kernel
    for _ in range(3):                                # runs at the package power limit)
        ba.extract_costmaps(trivial, out=cm)
    ctx.timer_start()
    for _ in range(reps):
        ba.extract_costmaps(trivial, out=cm)
    ex_ms = ctx.timer_stop() / reps
    ex_bytes = PS * PS * C * 2 + C * 8 + 3 * PS * PS * 2          # feature patch + reference in, 3-channel fp16 map out
    cba = ba.costmap_problem(cm)
    cfg_cm = interp_cfg(l2_normalize=False)                       # bundle_adjustment/main.py:270
    for _ in range(3):
        cba.eval(cfg_cm, with_jacobian=True)
    ctx.timer_start()
    for _ in range(20):
        cba.eval(cfg_cm, with_jacobian=True)
    ev_ms = ctx.timer_stop() / 20
    costmap = {"extract_ms": ex_ms, "maps_per_sec": n_obs_local / (ex_ms * 1e-3),
               "extract_GBps": ex_bytes * n_obs_local / (ex_ms * 1e-3) / 1e9,
               "extract_frac_of_peak": ex_bytes * n_obs_local / (ex_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
               "extract_bytes_per_map": ex_bytes, "kernel": "costmap_kernel_f16_split%s<f16> (%dx%dx128, gradients)" % ("8" if PS == 8 else "", PS, PS),
               "map_arena_GB": n_obs_local * PS * PS * 3 * 2 / 1e9,
               "extract_bound": "vector ALU at the package power limit: ~1800 4-cycle vector instructions per lane and map "
                                "(the reference's double accumulation and half -> double conversions), 1366 W / shader clock "
                                "2.10 GHz while it runs (profiles/r2_costmap_clock_power.txt, r2_costmap_split_pmc_sq.json)",
               "eval_ms": ev_ms, "eval_blocks_per_sec": n_obs_local / (ev_ms * 1e-3)}
    if args.lm_iters > 0:
        n_img = args.cams
        pose_const, tmask, cmask, ptc = default_gauge(n_img, len(prob["xyz"]))
        for key, inner in (("lm", True), ("lm_no_inner", False)):
            reset_parameters(ba, prob)
            s = cba.solve(cfg_cm, make_loss("cauchy", [0.25]), pose_const, tmask, cmask, ptc,
                          options=lm_options(max_iterations=args.lm_iters, use_inner_iterations=inner))
            costmap[key] = {"iters_per_sec": s["iterations"] / (s["total_ms"] * 1e-3), "iterations": s["iterations"],
                            "successful": s["num_successful"], "ms_per_iter": s["total_ms"] / max(1, s["iterations"]),
                            "initial_cost": s["initial_cost"], "final_cost": s["final_cost"], "inner_iterations": inner}
    return costmap


def committed_ka_traffic():
    """HBM bytes per pxr_ka_solve launch at configs[1] from the newest committed counter file (profiles/r*_ka_solve_traffic.json)."""
    best = None
    for path in glob.glob(os.path.join(ROOT, "profiles", "r*_ka_solve_traffic.json")):
        m = re.match(r"r(\d+)_ka_solve_traffic\.json$", os.path.basename(path))
        if m and (best is None or int(m.group(1)) > best[0]):
            best = (int(m.group(1)), path)
    if best is None:
        return None, None
    with open(best[1]) as fh:
        rec = json.load(fh)
    return rec.get("hbm_bytes_per_launch"), "committed profile profiles/%s (separate rocprofv3 --pmc passes; NOT measured in this run); measured at commit %s" % (
        os.path.basename(best[1]), rec.get("measured_at_commit", "unrecorded"))


def committed_traffic(world, n_obs_total, float_simd):
    """HBM bytes per launch of the dominant kernel from the PMC counters: collected in separate rocprofv3 --pmc passes of this
    same command (gpurun refuses / forbids mixing passes) and committed under profiles/ -- the NEWEST round's file."""
    if world != 1 or n_obs_total != 1_000_000 or float_simd:
        return None, None
    best = None
    for path in glob.glob(os.path.join(ROOT, "profiles", "r*_ba_eval_pmc.json")):
        m = re.match(r"r(\d+)_ba_eval_pmc\.json$", os.path.basename(path))
        if m and (best is None or int(m.group(1)) > best[0]):
            best = (int(m.group(1)), path)
    if best is None:
        return None, None
    with open(best[1]) as fh:
        rec = json.load(fh)
    src = ("committed profile profiles/%s (separate rocprofv3 --pmc passes of this command; NOT measured in this run); "
           "measured at commit %s" % (os.path.basename(best[1]), rec.get("measured_at_commit", "unrecorded")))
    return rec.get("hbm_bytes_per_launch"), src


# ---------------------------------------------------------------------------------------------------------------------
# the printed line: compact (the driver keeps a few KB of tail), everything else goes to bench_detail.json
# ---------------------------------------------------------------------------------------------------------------------
LINE_BUDGET_BYTES = 6000


def _r(x, sig=5):
    """Round floats to `sig` significant digits (None / ints / strings pass through)."""
    if isinstance(x, bool) or not isinstance(x, float):
        return x
    if x == 0.0 or x != x or x in (float("inf"), float("-inf")):
        return x
    return float("%.*g" % (sig, x))


def _pick(d, keys):
    return {k: _r(d[k]) for k in keys if isinstance(d, dict) and k in d}


def _mean(stats):
    return _r(stats["mean"], 4) if isinstance(stats, dict) and stats.get("mean") is not None else None


def compact_line(full):
    """The ONE line rank 0 prints, cut down from the full result `full` (written to bench_detail.json): the contract's
    fields, roofline, cpu_baseline, then one short object per secondary figure, and -- LAST, so that the tail the driver
    keeps always carries metric 2 -- `telemetry`, `lm_no_inner` and `lm`.  Stays under LINE_BUDGET_BYTES (tests/)."""
    out = {k: full[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "settle_launches", "ms_per_step", "higher_is_better",
                                "scaling", "vs_baseline", "dtype", "data") if k in full}
    for k in ("value", "ms_per_step"):
        out[k] = _r(out.get(k), 7)
    cfg = dict(full.get("config", {}))
    cfg["arena_GB"] = _r(cfg.get("arena_GB"))
    out["config"] = cfg
    ro = full.get("roofline", {})
    out["roofline"] = _pick(ro, ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "kernel_ms",
                                 "algorithmic_bytes_per_obs"))
    if ro.get("traffic_source"):
        m = re.search(r"profiles/\S+", ro["traffic_source"])
        out["roofline"]["traffic_source"] = (m.group(0) if m else "committed profile") + ", separate --pmc passes, not this run"
    cb = full.get("cpu_baseline")
    if cb:
        out["cpu_baseline"] = _pick(cb, ("value", "unit", "cores", "kind", "single_thread", "harness_limited"))
        host = full.get("cpu_host", {})
        out["cpu_baseline"]["cgroup_cpu_quota"] = host.get("cgroup_cpu_quota")
        out["cpu_baseline"]["physical_cores"] = host.get("physical_cores")
        out["cpu_baseline"]["sample"] = (cb.get("sample") or "")[:150]
        out["gpu_over_cpu"] = _r(full["value"] / cb["value"], 4) if cb.get("value") else None
    if "like_for_like" in full:
        out["like_for_like"] = full["like_for_like"]
    if full.get("initial_cost") is not None:
        out["initial_cost"] = _r(full["initial_cost"], 10)
    if "collective" in full:
        out["collective"] = full["collective"][:60]
    if "ranks" in full:
        out["ranks"] = {k: ([_r(x, 4) for x in v] if isinstance(v, list) else v) for k, v in full["ranks"].items()}
    cpl = full.get("cpu_baseline_lm_projected")
    if cpl:
        out["cpu_lm_projected"] = _pick(cpl, ("value", "cores", "kind", "ms_per_iteration_projected"))
    ge = full.get("gram_evaluation")
    if ge:
        out["gram_evaluation"] = {"from_cache_ms": _r(ge.get("evaluate_from_cache_ms")), "build_and_evaluate_ms": _r(ge.get("build_and_evaluate_ms")),
                                  "from_cache_frac_of_hbm": _r((ge.get("roofline") or {}).get("frac"), 3)}
    cm = full.get("costmap")
    if cm:
        out["costmap"] = _pick(cm, ("extract_ms", "extract_GBps", "extract_frac_of_peak", "extract_bytes_per_map", "eval_ms"))
        for k in ("lm", "lm_no_inner"):
            if k in cm:
                out["costmap"][k + "_ms_per_iter"] = _r(cm[k]["ms_per_iter"])
    ka = full.get("ka")
    if ka:
        sol, rf = ka.get("solve", {}), ka.get("roofline", {})
        out["ka"] = {"workload": "configs[1]: 10k tracks / 100k keypoints / %s sub-problems" % (ka.get("workload", "").split(" edges, ")[-1].split(" sub-")[0]),
                     "edge_eval_ms": _r(ka.get("edge_eval", {}).get("kernel_ms")),
                     "edges_per_s": _r(ka.get("edge_eval", {}).get("edges_per_s")),
                     "solve": _pick(sol, ("kernel_ms", "kernel_ms_min", "kernel_ms_first", "solves_timed", "wall_ms", "lm_iterations_max",
                                          "successful_steps", "initial_cost", "final_cost")),
                     "roofline": _pick(rf, ("bound", "achieved", "peak", "frac", "kernel", "kernel_ms", "algorithmic_bytes", "traffic", "traffic_source")),
                     "accuracy_px": {k: _r(v, 3) for k, v in ka.get("accuracy_px", {}).items()}}
        if ka.get("operating_points"):
            out["ka"]["operating_points_kernel_ms"] = {k: _r(v.get("kernel_ms")) for k, v in ka["operating_points"].items()}
        t = ka.get("telemetry")
        if t:
            out["ka"]["telemetry"] = {"sclk_mhz_mean": _mean(t.get("sclk_mhz")), "power_w_mean": _mean(t.get("power_w")),
                                      "samples": t.get("samples")}
        if ka.get("cpu_baseline"):
            out["ka"]["cpu_baseline"] = _pick(ka["cpu_baseline"], ("value", "unit", "cores", "kind", "projected_full_solve_ms"))
            out["ka"]["gpu_over_cpu_solve"] = _r(ka.get("gpu_over_cpu_solve"), 4)
    ae = full.get("api_e2e")
    if ae:
        out["api_e2e"] = {}
        for k in ("ba_host", "ba_host_two_levels", "ka_host"):
            if k in ae:
                ph = ae[k].get("phases_s", {})
                top = sorted(ph.items(), key=lambda kv: -kv[1])[:4]
                out["api_e2e"][k] = {"wall_s": _r(ae[k].get("wall_s"), 4), "phases_s": {a: _r(b, 3) for a, b in top}}
    if full.get("detail_file") is not None:
        out["detail"] = full["detail_file"]
    if "watchdog" in full:
        out["watchdog"] = full["watchdog"]
    # ---- the tail: clocks, then both LM figures (metric 2) ----
    t = full.get("telemetry")
    if t:
        out["telemetry"] = {"sclk_mhz": {k: _r(v, 5) for k, v in (t.get("sclk_mhz") or {}).items()} or None,
                            "mclk_mhz_mean": _mean(t.get("mclk_mhz")),
                            "power_w": {k: _r(v, 4) for k, v in (t.get("power_w") or {}).items()} or None,
                            "kernel_ms_in_this_loop": _r(t.get("kernel_ms_in_this_loop")), "samples": t.get("samples"),
                            "error": t.get("error")}
    for key in ("lm_no_inner", "lm"):
        v = full.get(key)
        if not v:
            continue
        o = _pick(v, ("iters_per_sec", "ms_per_iter", "ms_per_iter_after_initial", "initial_ms", "iterations", "successful", "setup_ms", "reduced_system",
                      "linear_iterations", "inner_iterations", "collective_KiB_per_solve", "native_collective_calls",
                      "native_collective_bytes"))
        o["mode"] = "defaults: deterministic (integer sums), evaluation from cached Gram matrices"
        o["initial_cost"], o["final_cost"] = _r(v.get("initial_cost"), 10), _r(v.get("final_cost"), 10)
        o["linear_solver"] = "direct: Schur + dense Cholesky" if str(v.get("linear_solver", "")).startswith("point") else "iterative: implicit Schur PCG"
        for sub in ("texel_evaluation", "nondeterministic", "deterministic", "first_solve_of_the_process"):
            if isinstance(v.get(sub), dict):
                o[sub] = {a: _r(b) for a, b in v[sub].items() if not isinstance(b, (dict, list))}
        for sub in ("allreduce_ms", "allreduce_bytes"):
            if sub in v:
                o[sub] = _r(v[sub])
        sm = (full.get("lm") or {}).get("scaling_model")
        if isinstance(sm, dict) and isinstance(sm.get("value"), dict) and "value_scaling_model_8gpu" not in out:
            out["value_scaling_model_8gpu"] = {a: _r(b, 4) for a, b in sm["value"].items() if a != "note"}
        if isinstance(sm, dict) and isinstance(sm.get(key), dict):
            o["scaling_model_8gpu"] = {a: _r(b, 4) for a, b in sm[key].items()}
        elif isinstance(sm, dict) and key == "lm" and "error" in sm:
            o["scaling_model_8gpu"] = sm
        out[key] = o
    return out


def write_detail(full, path):
    """Everything the line no longer carries (sweeps, cgroup dumps, phase tables): bench_detail.json."""
    try:
        with open(path, "w") as fh:
            json.dump(full, fh, indent=1, default=str)
        return path
    except OSError as e:
        print("bench.py: could not write %s (%r)" % (path, e), file=sys.stderr)
        return None


DUMP_SAMPLE_ROWS = 1 << 18          # 2^18 records x 64 B = 16.8 MB: the dump stays far below 64 MB at any scene size
DUMP_SAMPLE_SEED = 20240917


def dump_outputs(job, ba, out_dir):
    """--dump-outputs: what the timed path handed its caller in the last step -- the n_obs x 8 float64 records of pxr_ba_eval
    (still in ba.rec: nothing runs on it after the timed loop) -- as a fixed, seeded sample of rows, their indices, and the column
    sums over all rows.  Every rank writes its own shard's files (suffix .rank<r> when there are several)."""
    import numpy as np
    job.ctx.sync()
    rec = ba.rec.download()
    n = rec.shape[0]
    if n > DUMP_SAMPLE_ROWS:
        idx = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(n, DUMP_SAMPLE_ROWS, replace=False))
    else:
        idx = np.arange(n)
    suffix = ".rank%d" % job.rank if job.world > 1 else ""
    os.makedirs(out_dir, exist_ok=True)
    for name, arr in (("records_sample", rec[idx]), ("records_sample_index", idx.astype(np.float64)),
                      ("records_column_sum", rec.sum(axis=0))):
        np.save(os.path.join(out_dir, name + suffix + ".npy"), np.ascontiguousarray(arr, dtype=np.float64))


def make_scene(job):
    """This rank's share of the synthetic scene, resident in HBM: points (with their observations, patches and references)
    are the sharded unit; cameras and poses are replicated.  weak: the scene grows with the ranks, strong: split."""
    import numpy as np
    from pixsfm_amd import synthetic_gpu
    from pixsfm_amd.engine import BAProblem, PatchArena
    args, rank, world = job.args, job.rank, job.world
    C, PS = 128, args.patch_size
    total_points = args.points * world if args.scaling == "weak" else args.points
    per = (total_points + world - 1) // world
    lo, hi = rank * per, min(total_points, (rank + 1) * per)
    prob, patches = synthetic_gpu.make_ba_problem_gpu(job.dev, n_cams=args.cams, n_points=total_points,
                                                      obs_per_point=args.obs_per_point, channels=C,
                                                      patch_size=PS, seed=2, point_range=(lo, hi),
                                                      # 8 x 8 patches leave +-2 px around the stencil: ~1 px initial errors
                                                      **(dict(rot_deg=0.04, trans=0.003, pt_sigma=0.003) if PS < 16 else {}))
    arena = PatchArena(job.ctx, len(prob["obs_image"]), PS, PS, C, np.float16, device_ptr=patches.data_ptr())
    arena.upload(0, None, prob["corners"], prob["scales"])
    return prob, patches, arena, BAProblem(job.ctx, arena, prob), total_points


def gather_ranks(job, n_obs_local, kernel_ms):
    """What makes a multi-GPU run self-verifying: every rank's share and kernel time, the ranks the native communicator
    really joined."""
    if not job.dist_on:
        return None
    import torch
    import torch.distributed as dist
    mine = torch.tensor([float(job.rank), float(n_obs_local), kernel_ms, float(job.local_rank)], dtype=torch.float64, device=job.dev)
    every = [torch.zeros_like(mine) for _ in range(job.world)]
    dist.all_gather(every, mine)
    every = torch.stack(every).cpu().numpy()
    _, comm_n = job.ctx.comm_rank()
    seen = job.reduce(1.0 if job.native and comm_n == job.world else 0.0)
    return {"obs_per_gpu": [int(v) for v in every[:, 1]], "kernel_ms": [float(v) for v in every[:, 2]],
            "kernel_ms_min": float(every[:, 2].min()), "kernel_ms_max": float(every[:, 2].max()),
            "devices": [int(v) for v in every[:, 3]], "nranks_seen": int(comm_n), "ranks_in_native_communicator": int(seen)}


def run_projection_jacobian(job, ba):
    """k_jac alone (pxr_ba_projection_jacobian): the 2 x (10+K) projection Jacobian P of J = G P that the fused headline kernel
    does not write.  evaluation + this = the like-for-like unit next to a CPU leg that materialises 128 x (10+K) Jacobians."""
    ctx = job.ctx
    P = ba.projection_jacobian()
    ctx.sync()
    reps = 20
    ctx.timer_start()
    for _ in range(reps):
        ba.projection_jacobian(out=P)
    ms = ctx.timer_stop() / reps
    P.free()
    return ms


def lm_entry(v, key, job):
    return {"iters_per_sec": v["iterations"] / (v["total_ms"] * 1e-3), "iterations": v["iterations"],
            "successful": v["num_successful"], "ms_per_iter": v["total_ms"] / max(1, v["iterations"]),
            "setup_ms": v["setup_ms"], "initial_cost": v["initial_cost"], "final_cost": v["final_cost"],
            "reduced_system": v["num_camera_unknowns"],
            # total_ms also holds the evaluation at the initial point and the two linearisations behind the Jacobi scaling: per
            # iteration WITHOUT them (what another 90 iterations of pixsfm's default 100 would cost each)
            "ms_per_iter_after_initial": (v["total_ms"] - v.get("initial_us", 0) * 1e-3) / max(1, v["iterations"]),
            "initial_ms": v.get("initial_us", 0) * 1e-3,
            "linear_solver": "point Schur complement (LDS-privatised) + hand-written blocked dense Cholesky"
                             if v["linear_solver"] == 1 else
                             "implicit Schur complement, block-Jacobi preconditioned CG (ITERATIVE_SCHUR regime)",
            "linear_iterations": v["linear_iterations"], "collective": job.collective,
            "collective_KiB_per_solve": v.get("collective_kib", 0),
            "native_collective_calls": v.get("native_collective_calls"), "native_collective_bytes": v.get("native_collective_bytes"),
            "inner_iterations": key == "lm"}


def secondary_legs(job, total_points):
    """KA (BASELINE configs[1]) and the drop-in calls end to end; both need the BA scene's HBM back first."""
    import torch
    args, rank, world = job.args, job.rank, job.world
    ka_result = api_e2e = None
    if not args.no_ka:
        # one KA edge (A7): per-edge residual+Jacobian rate and the whole bounded LM; with several ranks the sub-problems are
        # dealt to them (every rank takes part, rank 0 reports)
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import bench_ka
        ka_result = bench_ka.run(device_index=job.local_rank, ctx=job.ctx, rank=rank, world=world,
                                 cpu_legs=(rank == 0 and world == 1 and not args.no_cpu_baseline),
                                 telemetry=None if args.no_telemetry else GpuTelemetry(job.local_rank))
        if ka_result is not None and world == 1 and ka_result.get("roofline", {}).get("traffic") is None:
            t, src = committed_ka_traffic()
            if t is not None:
                ka_result["roofline"]["traffic"], ka_result["roofline"]["traffic_source"] = t, src
        # the reference's OTHER shipped operating points of this path (VERDICT r5 missing-3): configs/low_memory.yaml:13-24 -- label
        # groups of 1000 keypoints, 8 x 8 patches, bound 2, topological_reference (examples/sfm+loc_aachen.py:124-125) -- and ONE
        # problem (split_in_subproblems = false, keypoint_adjustment/main.py:197-202).  A large label group runs on as many
        # workgroups as it has chunks of whole tracks, with the decisions of one Ceres problem (pxr_ka_view.d_prob_group).
        if rank == 0 and world == 1 and ka_result is not None and not args.no_ka_points:
            pts = {}
            for name, kw in (("max_kps_1000", dict(max_kps_per_problem=1000)),
                             ("one_problem", dict(max_kps_per_problem=0)),
                             ("low_memory_yaml", dict(max_kps_per_problem=1000, patch_size=8, bound=2.0, strategy="topological_reference")),
                             ("low_memory_yaml_50_per_problem", dict(max_kps_per_problem=50, patch_size=8, bound=2.0, strategy="topological_reference"))):
                try:
                    torch.cuda.empty_cache()
                    r = bench_ka.run(steps=2, device_index=job.local_rank, ctx=job.ctx, solves=3, **kw)
                    pts[name] = {"options": r["options"], "kernel_ms": r["solve"]["kernel_ms"], "kernel_ms_min": r["solve"]["kernel_ms_min"],
                                 "lm_iterations_max": r["solve"]["lm_iterations_max"], "successful_steps": r["solve"]["successful_steps"],
                                 "final_cost": r["solve"]["final_cost"], "median_error_px_after": r["accuracy_px"]["median_after"]}
                except Exception as e:  # noqa: BLE001 -- a secondary figure never fails the bench
                    pts[name] = {"error": repr(e)}
            ka_result["operating_points"] = pts
    if rank == 0 and world == 1 and not args.no_api_e2e:
        torch.cuda.empty_cache()
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import bench_api_e2e
        api_e2e = {"host_cores": os.cpu_count(),
                   "ba_host": bench_api_e2e.run_ba(job.dev, job.ctx, args.cams, total_points, args.obs_per_point, max(1, args.lm_iters), False)}
        if not args.no_ka:
            api_e2e["ka_host"] = bench_api_e2e.run_ka(job.dev, job.ctx, 10_000, 10, False)
        api_e2e["note"] = ("wall time of BundleAdjuster.create(conf).refine_multilevel(reconstruction, feature_manager) / "
                           "KeypointAdjuster...refine_multilevel(keypoints, feature_manager, graph) on host FeaturePatch objects "
                           "and Python scene objects, phases from pixsfm_amd.api._timing; building the inputs is not timed")
    return ka_result, api_e2e


class Watchdog:
    """Several ranks only.  The multi-rank legs after the headline measurement (the LM loop's all-reduce, the KA gather) have never met
    a second GPU in development: if one of them never returns, a rank cannot be interrupted out of the collective -- so a timer
    thread lets rank 0 print the line with what has been measured (the headline is complete by then) plus a `watchdog` note, and
    ends every rank with code 0 instead of leaving the driver to kill a silent job."""

    def __init__(self, seconds, rank, emit):
        import threading
        self.rank, self.emit, self.seconds = rank, emit, seconds
        self.timer = threading.Timer(seconds, self._fire) if seconds > 0 else None
        if self.timer is not None:
            self.timer.daemon = True
            self.timer.start()

    def _fire(self):
        try:
            print("bench.py rank %d: the legs after the headline did not finish in %.0f s -- giving up on them" % (self.rank, self.seconds),
                  file=sys.stderr, flush=True)
            if self.rank == 0:
                self.emit()
        finally:
            os._exit(0)

    def cancel(self):
        if self.timer is not None:
            self.timer.cancel()


def headline(job, args, dt, kernel_ms, n_obs_total, n_obs_local, total_points, cost, jac_ms):
    """The contract's fields + roofline of the one line (rank 0): complete as soon as the evaluation loop has been timed."""
    C, PS, world = 128, args.patch_size, job.world
    bpo = algorithmic_bytes_per_obs(C)
    traffic, traffic_source = committed_traffic(world, n_obs_total, args.float_simd)
    achieved = bpo * n_obs_local / (kernel_ms * 1e-3) / 1e9
    out = {
        "metric": "featuremetric residuals+Jacobians evaluated/sec (1M obs)",
        "value": n_obs_total * args.steps / dt,
        "unit": "residual_blocks/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        # untimed launches BEFORE the W warm-up steps that bring the GPU from idle to its sustained clocks (run_eval)
        "settle_launches": int(getattr(job, "settle_launches", 0)),
        "ms_per_step": dt / args.steps * 1e3,
        "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
        "dtype": "f32 horizontal / f64 vertical+normalisation on f16 patches"
                 if not args.float_simd else "f32 splines / f64 normalisation on f16 patches",
        "data": "synthetic",
        "config": {"workload": "BASELINE.json %s: synthetic %d cams / %d points / %d obs "
                               "featuremetric BA residual+Jacobian evaluation, %d-ch fp16 %dx%d patches, "
                               "SIMPLE_RADIAL, fused six-scalar Jacobian reduction"
                               % ("configs[4] shape (Aachen scale) on one GPU" if args.preset == "aachen" else "configs[2]",
                                  args.cams, total_points, n_obs_total, C, PS, PS),
                   "n_obs": n_obs_total, "channels": C, "patch": PS,
                   "arena_GB": n_obs_total * PS * PS * C * 2 / 1e9,
                   "obs_per_gpu": n_obs_local,
                   "partition": "points sharded, cameras replicated" if world > 1 else "none"},
        "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
                     "traffic_note": "bytes/launch, rocprofv3 FETCH_SIZE x2 (gfx950 correction) + WRITE_SIZE",
                     "traffic_source": traffic_source,
                     "kernel": "ba_eval_kernel<f16,128,jac>", "kernel_ms": kernel_ms,
                     "algorithmic_bytes_per_obs": bpo},
        "initial_cost": cost,
    }
    if jac_ms is not None:
        # the reference's unit materialises the Jacobian; the fused record + the projection Jacobian P (k_jac) is its equivalent
        out["like_for_like"] = {"what": "evaluation + k_jac (2x(10+K) projection Jacobian P of J = G P, which the fused record kernel omits)",
                                "k_jac_ms": _r(jac_ms), "ms": _r(dt / args.steps * 1e3 + jac_ms),
                                "value_with_projection_jacobian": _r(n_obs_total / ((dt / args.steps + jac_ms * 1e-3)), 7)}
    return out


def main():
    args = parse_args()
    if args.gpus > 1 and "RANK" not in os.environ:          # the plain command: be the launcher
        sys.exit(self_launch(sys.argv[1:], args.gpus))
    _selftest_hooks(int(os.environ.get("RANK", "0")))

    import torch
    job = Job(args)
    rank, world, ctx = job.rank, job.world, job.ctx
    from pixsfm_amd.engine import interp_cfg, make_loss
    C, PS = 128, args.patch_size
    prob, patches, arena, ba, total_points = make_scene(job)
    n_obs_local = len(prob["obs_image"])
    cfg = interp_cfg(use_float_simd=args.float_simd)

    dt, kernel_ms = run_eval(job, ba, cfg)
    n_obs_total = int(job.reduce(float(n_obs_local)))
    if args.dump_outputs:
        dump_outputs(job, ba, args.dump_outputs)
    if not args.full:
        result_line = None
        if rank == 0:
            line = compact_line(headline(job, args, dt, kernel_ms, n_obs_total, n_obs_local, total_points, None, None))
            result_line = json.dumps(line, separators=(",", ":"))
        finish(job, result_line)
        return
    per_rank = gather_ranks(job, n_obs_local, kernel_ms)
    cost = job.reduce(ba.cost(make_loss("cauchy", [0.25])))         # cost of the whole (sharded) problem
    per_rank_now = per_rank

    def emit_partial():         # the watchdog's line: the headline as measured, nothing of the legs that did not come back
        part = headline(job, args, dt, kernel_ms, n_obs_total, n_obs_local, total_points, cost, None)
        part["collective"] = job.collective
        if per_rank_now is not None:
            part["ranks"] = per_rank_now
        part["watchdog"] = ("the legs after the headline measurement (LM loop / KA over %d ranks) did not finish within %.0f s; "
                            "`value` and `roofline` are complete" % (world, args.watchdog_s))
        import ctypes
        ctypes.CDLL(None).fflush(None)
        sys.stdout.flush()
        print(json.dumps(compact_line(part), separators=(",", ":")), flush=True)
    watchdog = Watchdog(args.watchdog_s if world > 1 else 0.0, rank, emit_partial)
    telemetry = None
    if rank == 0 and not args.no_telemetry:
        try:
            telemetry = run_telemetry(job, ba, cfg)
        except Exception as e:  # noqa: BLE001 -- never let the sampling break the bench
            telemetry = {"error": repr(e)}
    job.barrier()
    jac_ms = job.reduce(run_projection_jacobian(job, ba), "max")
    gram_eval = run_gram(job, ba, cfg)
    job.barrier()
    lm, lm_extra = run_lm(job, ba, prob, cfg)
    if rank == 0 and world == 1 and lm and args.preset is None and args.linear_solver != "iterative":
        try:
            lm_extra["scaling_model"] = run_scaling_model(job, prob, patches, lm, cfg, measured_call_ms=lm_extra.get("allreduce_ms"),
                                                               full_step_ms=dt / args.steps * 1e3)
        except Exception as e:  # noqa: BLE001 -- a model, never the reason for a failed bench
            lm_extra["scaling_model"] = {"error": repr(e)}
    costmap = run_costmap(job, ba, prob) if (not args.no_costmap and world == 1) else None
    cpu_base = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu_base = cpu_baseline(prob, patches, args.cpu_sample, lm_gauge=default_gauge(args.cams, 0)[:3])
    del ba
    arena.close()
    del arena, patches
    torch.cuda.empty_cache()
    ka_result, api_e2e = secondary_legs(job, total_points)

    watchdog.cancel()
    result_line = None
    if rank == 0:
        out = headline(job, args, dt, kernel_ms, n_obs_total, n_obs_local, total_points, cost, jac_ms)
        if telemetry is not None:
            out["telemetry"] = telemetry
        for key, v in lm.items():
            out[key] = lm_entry(v, key, job)
        if cpu_base is not None:
            out.update(cpu_base)
        if ka_result is not None:
            out["ka"] = ka_result
        out["gram_evaluation"] = gram_eval
        if costmap is not None:
            out["costmap"] = costmap
        if api_e2e is not None:
            out["api_e2e"] = api_e2e
        out["collective"] = job.collective
        if per_rank is not None:
            out["ranks"] = per_rank
        if "lm" in out:
            if "no_inner_texel_evaluation" in lm_extra:
                out["lm_no_inner"]["texel_evaluation"] = lm_extra.pop("no_inner_texel_evaluation")
            out["lm"].update(lm_extra)
        out["detail_file"] = write_detail(out, args.detail_out)
        line = compact_line(out)
        result_line = json.dumps(line, separators=(",", ":"))
        if len(result_line) > LINE_BUDGET_BYTES:            # never let the line outgrow the driver's tail: drop the least important objects
            for k in ("api_e2e", "gram_evaluation", "cpu_lm_projected", "costmap", "ranks"):
                line.pop(k, None)
                result_line = json.dumps(line, separators=(",", ":"))
                if len(result_line) <= LINE_BUDGET_BYTES:
                    break
    finish(job, result_line)


def finish(job, result_line):
    """The JSON line must be the last thing on stdout: native libraries (RCCL's version banner, ...) write to the C
    stdio buffer of every rank, which would otherwise be flushed at exit -- after the line.  Flush it now, wait for
    all ranks, tear the process group down, then print."""
    import ctypes
    libc = ctypes.CDLL(None)
    libc.fflush(None)
    sys.stdout.flush()
    if job.dist_on:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
        libc.fflush(None)
    if result_line is not None:
        print(result_line, flush=True)


if __name__ == "__main__":
    main()
