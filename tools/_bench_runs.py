"""What the bench_*.py tools of the batched estimators share: the statistics of a list of times and the warm-up / repeat loop."""
import time


def stats(values, keep_all=True):
    v = sorted(float(x) for x in values)
    out = {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}
    if keep_all:
        out["all"] = [round(x, 5) for x in values]
    return out


def timed_runs(ctx, run, repeats):
    """run: the bound method that launches the kernels (estimate, triangulate) and, with timed=True, leaves their HIP-event times
    in its problem's kernel_ms.  One untimed warm-up call, then `repeats` timed ones.  Returns (the last call's outputs,
    {kernel: [ms per call]}, [wall ms per call, device synchronisation included])."""
    run()                                                                # warm-up
    ctx.sync()
    kernels, wall = {}, []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = run(timed=True)
        ctx.sync()
        wall.append(1e3 * (time.perf_counter() - t0))
        for name, ms in run.__self__.kernel_ms.items():
            kernels.setdefault(name, []).append(ms)
    return out, kernels, wall
