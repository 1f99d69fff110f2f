"""GPU: the record of an observation does not depend on where it sits in the observation list.

The BA residual kernel walks a few consecutive observations per lane group and keeps the reference descriptor of the point it
holds, reloading it only when the next observation belongs to another point.  Every record (and, in materialise mode, every
residual / gradient row) must come out bit-identical whatever the order: point-sorted with ragged tracks of 1-7 observations,
a random order, an order in which the point changes at every observation, reversed -- and whatever the number of observations
a lane group walks (PXR_BA_EVAL_OPR, read once per process: every value runs in a subprocess of its own).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (arena dtype, channels, use_float_simd, materialise, with_jacobian)
CASES = [
    ("f16", 128, False, False, True),
    ("f16", 128, True, False, True),
    ("f16", 128, False, True, True),
    ("f16", 128, False, False, False),
    ("f32", 128, False, False, True),
    ("f64", 128, False, True, True),
    ("f16", 64, False, False, True),
    ("f32", 64, True, True, True),
]
DTYPES = {"f16": np.float16, "f32": np.float32, "f64": np.float64}


def _ragged(prob, rng):
    """Keep 1..7 observations of every point (tracks stay point-sorted); obs_patch keeps pointing into the full arena."""
    keep = []
    opp = int(np.bincount(prob["obs_point"]).max())
    for p in range(len(prob["xyz"])):
        k = int(rng.integers(1, opp + 1))
        keep.extend(range(p * opp, p * opp + k))
    keep = np.asarray(keep)
    out = dict(prob)
    for name in ("obs_image", "obs_point", "obs_patch"):
        out[name] = np.ascontiguousarray(prob[name][keep])
    return out


def _orders(obs_point, rng):
    n = len(obs_point)
    rank = np.zeros(n, np.int64)          # position of each observation inside its track
    for i in range(1, n):
        rank[i] = rank[i - 1] + 1 if obs_point[i] == obs_point[i - 1] else 0
    return {
        "sorted": np.arange(n),
        "random": rng.permutation(n),
        "point_changes_every_obs": np.lexsort((obs_point, rank)),   # round robin over the points
        "reversed": np.arange(n)[::-1].copy(),
    }


def _worker(out_path):
    """Evaluates every case in every order; writes the records (and materialised rows) back in the sorted order."""
    from pixsfm_amd import synthetic
    from pixsfm_amd.engine import BAProblem, Context, PatchArena, interp_cfg
    ctx = Context(0)
    res = {}
    for ci, (dt, C, fs, mat, wj) in enumerate(CASES):
        rng = np.random.default_rng(100 + ci)
        full = synthetic.make_ba_problem(n_cams=8, n_points=97, obs_per_point=7, channels=C, seed=30 + ci, dtype=DTYPES[dt])
        prob = _ragged(full, rng)
        arena = PatchArena.from_numpy(ctx, full["patches"], full["corners"], full["scales"])
        for name, perm in _orders(prob["obs_point"], rng).items():
            p = dict(prob)
            for k in ("obs_image", "obs_point", "obs_patch"):
                p[k] = np.ascontiguousarray(prob[k][perm])
            ba = BAProblem(ctx, arena, p)
            rec, r, gx, gy = ba.eval(interp_cfg(use_float_simd=fs), with_jacobian=wj, materialize=mat)
            inv = np.empty_like(perm)
            inv[perm] = np.arange(len(perm))
            arrs = [rec.download()] + ([r.download()] if mat else []) + ([gx.download(), gy.download()] if mat and wj else [])
            for ai, a in enumerate(arrs):
                res["%d_%s_%d" % (ci, name, ai)] = np.ascontiguousarray(a[inv])
    np.savez(out_path, **res)
    print(json.dumps({"cases": len(CASES), "arrays": len(res)}))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope="module")
def by_opr(tmp_path_factory):
    d = tmp_path_factory.mktemp("ba_eval_order")
    out = {}
    for opr in (1, 4, 16):
        path = str(d / ("opr%d.npz" % opr))
        env = dict(os.environ, PXR_BA_EVAL_OPR=str(opr))
        proc = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, cwd=ROOT,
                              capture_output=True, text=True, timeout=900)
        assert proc.returncode == 0, "worker (PXR_BA_EVAL_OPR=%d) failed:\n%s\n%s" % (opr, proc.stdout[-4000:], proc.stderr[-4000:])
        out[opr] = dict(np.load(path))
    return out


pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("opr", [1, 4, 16])
def test_records_do_not_depend_on_observation_order(by_opr, opr):
    res = by_opr[opr]
    n_checked = 0
    for key, a in res.items():
        if "_sorted_" in key:
            continue
        ref = res[key.replace("_random_", "_sorted_").replace("_point_changes_every_obs_", "_sorted_").replace("_reversed_", "_sorted_")]
        assert a.shape == ref.shape, key
        assert np.array_equal(_bits(a), _bits(ref)), "%s differs from the point-sorted order (PXR_BA_EVAL_OPR=%d)" % (key, opr)
        n_checked += 1
    assert n_checked == 3 * sum(1 + (1 if m else 0) + (2 if m and wj else 0) for _, _, _, m, wj in CASES)


def test_records_do_not_depend_on_observations_per_lane_group(by_opr):
    base = by_opr[1]          # one observation per lane group: the reference is always loaded for the observation itself
    for opr in (4, 16):
        assert sorted(by_opr[opr]) == sorted(base)
        for key, a in by_opr[opr].items():
            assert np.array_equal(_bits(a), _bits(base[key])), "%s: PXR_BA_EVAL_OPR=%d differs from 1" % (key, opr)


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "pixel-perfect-sfm_amd"))
    _worker(sys.argv[1])
