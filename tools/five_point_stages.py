"""Where the five-point solver loses its digits: the numpy restatement of tests/twoview_cases.py is run
as it is and with exact input for one more stage at a time -- the null space, the 10 x 20 constraint rows, the polynomial
det B(z), each from the mpmath reference of tests/minimal_solver_ref.py rounded to double -- and every run is held against the
reference's solutions.  Prints, per family, the solutions beyond 1e4 kappa u and the largest err / (kappa u).  CPU only.

    python tools/five_point_stages.py [--samples 16] [--polish 0] [family ...]

--polish: the Gauss-Newton steps that tv.five_point takes per hypothesis (0: the elimination alone, as the table was made)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "pixel-perfect-sfm_amd"), ROOT]

import minimal_solver_ref as ms          # noqa: E402
import twoview_cases as tv               # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--polish", type=int, default=0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("families", nargs="*", default=["generic", "parallax 1e-1", "parallax 1e-2", "parallax 1e-3", "parallax 1e-4", "planar scene"])
    a = ap.parse_args()
    tv.POLISH = a.polish
    for name in a.families:
        rec, _ = tv.hard_family(name, a.seed, a.samples)
        ratios = {k: [] for k in ("as is", "exact null space", "+ exact rows", "+ exact det B(z)")}
        for b in range(len(rec)):
            sols, st = ms.five_point(rec[b], nister=tv.NISTER)
            exact, runs = {}, {"as is": tv.five_point(rec[b:b + 1])}
            for key, stage in (("exact null space", "basis"), ("+ exact rows", "rows"), ("+ exact det B(z)", "c")):
                exact[stage] = st[stage][None]
                runs[key] = tv.five_point(rec[b:b + 1], exact=dict(exact))
            for s in sols:
                if not np.isfinite(s["kappa"]):
                    continue
                for key, (E, valid) in runs.items():
                    err = min([ms.projective_distance(E[0, r], s["E"]) for r in range(10) if valid[0, r]] or [np.inf])
                    ratios[key].append(err / (s["kappa"] * ms.U))
        print(name + ": " + " | ".join("%s %d / %d beyond 1e4 kappa u, max %.2g" % (k, sum(x > 1e4 for x in v), len(v), max(v)) for k, v in ratios.items()), flush=True)


if __name__ == "__main__":
    main()
