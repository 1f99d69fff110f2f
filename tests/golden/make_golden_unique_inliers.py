"""Generates tests/golden/unique_inliers_ref.npz by running the REFERENCE's own `find_unique_inliers` and
`find_unique_min_by_group` (pixsfm/localization/main.py:38-62) on seeded inputs, ties and pre_inliers included.  The module
itself cannot be imported here (omegaconf / pycolmap / the pybind module are absent), so the two functions are cut out of the
file with `ast` at generation time and executed on their own -- nothing of them is copied into the repository.  Inputs and
outputs are both stored, so the test needs the file alone.

Run where a checkout of the reference is at hand:  python tests/golden/make_golden_unique_inliers.py <path to pixel-perfect-sfm>
"""
import ast
import os
import sys
from collections import defaultdict

import numpy as np


def load_reference_functions(src):
    tree = ast.parse(open(src).read())
    names = ("find_unique_inliers", "find_unique_min_by_group")
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    ns = {"np": np, "defaultdict": defaultdict}
    exec(compile(ast.Module(body=fns, type_ignores=[]), src, "exec"), ns)
    return [ns[n] for n in names]


def cases():
    """(name, idxs, errors, pre_inliers | None), seeded."""
    rng = np.random.default_rng(20261018)
    out = []
    for i in range(24):
        n = int(rng.integers(1, 120))
        idxs = rng.integers(0, max(1, n // int(rng.choice([1, 2, 5]))), n) + int(rng.choice([0, 1000]))
        errors = rng.uniform(0, 20, n)
        if i % 2 == 0:
            errors = np.round(errors)                      # ties within a group: the first of equals wins
        pre = None if i % 3 == 0 else rng.random(n) < 0.7
        out.append(("case%02d" % i, idxs.astype(np.int64), errors, pre))
    out.append(("all_out", np.array([4, 4, 5], np.int64), np.array([1.0, 2.0, 3.0]), np.zeros(3, bool)))
    out.append(("one_group", np.zeros(9, np.int64), np.array([3.0, 1.0, 1.0, 2.0, 1.0, 5.0, 0.5, 0.5, 4.0]), None))
    return out


if __name__ == "__main__":
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("PIXSFM_REFERENCE", "")
    unique, min_by_group = load_reference_functions(os.path.join(root, "pixsfm", "localization", "main.py"))
    store = {}
    for name, idxs, errors, pre in cases():
        store[name + "_idxs"], store[name + "_errors"] = idxs, errors
        store[name + "_pre"] = np.zeros(0, bool) if pre is None else pre          # (empty: None)
        pre_l = None if pre is None else [bool(x) for x in pre]
        store[name + "_unique"] = np.asarray(unique([int(v) for v in idxs], pre_inliers=pre_l), dtype=bool)
        store[name + "_min"] = np.asarray(min_by_group([float(e) for e in errors], [int(v) for v in idxs], pre_inliers=pre_l), dtype=bool)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "unique_inliers_ref.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, len(store), "arrays")
