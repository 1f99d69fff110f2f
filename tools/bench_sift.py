"""SIFT throughput (csrc/pxr_sift.hip).  One JSON line on stdout; --out FILE also writes it.

    python tools/bench_sift.py [--out FILE] [--commit HASH] [--quick]

One grey uint8 image of 2000 x 1500 (the golden photograph tile repeated to that size, so the density of keypoints is that of
a photograph), both first_octave values, defaults otherwise.  Per stage the HIP-event time of its kernels (the *_timed entry
points) after a warm-up, the median of `--repeats` runs with the image resident on the device: pyramid, detect (count, scan,
write, orient, emit) and describe; features per second over their sum.  --quick: 500 x 375.
There is no earlier implementation to compare with; anything that was not run is recorded as "not measured".
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pixel-perfect-sfm_amd"))

import numpy as np  # noqa: E402


def photograph(h, w):
    tiles = np.load(os.path.join(ROOT, "tests", "golden", "real_image_tiles.npz"))["tiles"]
    grey = np.round(tiles[0].astype(np.float64).mean(-1)).astype(np.uint8)
    reps = (-(-h // grey.shape[0]), -(-w // grey.shape[1]))
    return np.ascontiguousarray(np.tile(grey, reps)[:h, :w])


def commit(given):
    if given:
        return given
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL, text=True).strip()
    except Exception:
        return "not recorded"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--commit", help="the commit the working tree stands on (the GPU machine has no .git)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    import torch
    from pixsfm_amd.engine import Context, SiftPyramid
    h, w = (375, 500) if args.quick else (1500, 2000)
    ctx = Context(0)
    image = torch.from_numpy(photograph(h, w)).to("cuda:0")
    torch.cuda.synchronize()
    res = {"tool": "tools/bench_sift.py", "commit": commit(args.commit), "image": [h, w], "dtype": "uint8", "repeats": args.repeats,
           "quick": bool(args.quick), "cpu_reference_or_other_library": "not measured (none is installed)"}
    for first in (-1, 0):
        runs = []
        for rep in range(args.repeats + 1):                         # the first run is the warm-up (it also grows the workspace)
            pyr = SiftPyramid(ctx, image, timed=True, first_octave=first)
            kp, _, _, found = pyr.detect(timed=True)
            pyr.describe(kp, timed=True)
            if rep:
                runs.append(dict(pyr.kernel_ms))
        ms = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
        detect = sum(ms[k] for k in ("count", "scan", "write", "orient", "emit"))
        total = ms["pyramid"] + detect + ms["describe"]
        res["first_octave_%d" % first] = {
            "features": int(found), "octaves": int(pyr.n_octaves), "pyramid_MB": round(pyr.d_pyramid.nbytes / 1e6, 1),
            "ms": {k: round(v, 4) for k, v in ms.items()}, "ms_pyramid": round(ms["pyramid"], 4), "ms_detect": round(detect, 4),
            "ms_describe": round(ms["describe"], 4), "ms_total": round(total, 4), "features_per_s": round(found / total * 1e3, 1)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
