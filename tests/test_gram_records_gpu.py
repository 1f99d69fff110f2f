"""GPU: the records of the Gram-matrix cache (pxr_ba_eval_gram: k_gram_eval, k_gram_build, k_gram_eval_dirty) held to the
long-double reference and the DERIVED bound of tests/gram_cases.py -- four to five orders tighter than the comparison with the
exact-order kernel in tests/test_gram_cache_gpu.py, which cannot see below the fp32 pass's rounding.  Patches are 7 x 9, at most
200 observations per problem.  The reference is evaluated at the (x, y) the device wrote into record entries 6 and 7."""
import numpy as np
import pytest

import gram_cases as gc

pytestmark = pytest.mark.gpu

_NAMES = [g["name"] for g in gc.groups()]
_REFERENCES = {}


def _group(name):
    return gc.groups()[_NAMES.index(name)]


def _reference(g, xy, idx=None):
    """Reference records and bounds of observations idx (default: all) at pixel positions xy[idx]; kept per (group, positions),
    read-only."""
    idx = np.arange(len(xy)) if idx is None else np.asarray(idx, dtype=np.int64)
    key = (g["name"], idx.tobytes(), np.ascontiguousarray(xy[idx]).tobytes())
    if key not in _REFERENCES:
        p = g["prob"]
        out = []
        for o in idx:
            k = int(p["obs_patch"][o])
            rec, q = gc.reference_record(p["patches"][k], p["refs"][p["obs_point"][o]], xy[o], p["scales"][k], p["corners"][k], g["l2"])
            out.append((rec, gc.bound(q, p["scales"][k], g["l2"], g["C"])))
        ref = np.stack([r for r, _ in out]) if out else np.empty((0, 6), gc.LD)
        bnd = np.stack([b for _, b in out]) if out else np.empty((0, 6), gc.LD)
        ref.setflags(write=False), bnd.setflags(write=False)
        _REFERENCES[key] = (ref, bnd)
    return _REFERENCES[key]


def _ratio(g, rec, idx=None):
    """error / bound of the six entries of rec[idx] against the reference at rec[idx, 6:8]: (len(idx), 6)."""
    ref, bnd = _reference(g, rec[:, 6:8], idx)
    got = rec[:, :6] if idx is None else rec[np.asarray(idx, dtype=np.int64), :6]
    assert np.isfinite(got).all()
    return (np.abs(got.astype(gc.LD) - ref) / bnd).astype(np.float64)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _open(ctx, prob):
    from pixsfm_amd.engine import BAProblem, PatchArena
    arena = PatchArena.from_numpy(ctx, prob["patches"], prob["corners"], prob["scales"])
    return arena, BAProblem(ctx, arena, prob)


@pytest.mark.parametrize("name", _NAMES)
def test_records_are_within_the_derived_bound_of_the_reference(ctx, name):
    from pixsfm_amd.engine import interp_cfg
    g = _group(name)
    p = g["prob"]
    arena, ba = _open(ctx, p)
    cfg = interp_cfg(l2_normalize=g["l2"])
    exact = ba.eval(cfg)[0].download().copy()
    rec, built = ba.eval_gram(cfg, reset=True)
    rec = rec.download().copy()
    arena.close()
    assert built == ba.n_obs == len(p["obs_image"])
    assert np.array_equal(_bits(rec[:, 6:]), _bits(exact[:, 6:]))                       # the projection is the same code
    if g["planned"] is not None:                                                        # ... and exact where it was placed
        assert np.array_equal(_bits(rec[:, 6:8]), _bits(g["planned"]))
    ratio = _ratio(g, rec)
    o, e = np.unravel_index(ratio.argmax(), ratio.shape)
    print("%-32s worst error / bound %.4f (%.1f x 2^-53 scale) at observation %d entry %d"
          % (name, ratio.max(), ratio.max() * gc.K(g["C"], g["l2"]), o, e))
    assert ratio.max() <= 1.0, (name, int(o), int(e), float(ratio.max()))
    assert (rec[:, 0] >= 0.0).all()                                                     # the clamp of |r|^2 (case i: ~ 0)
    if name.startswith("placed"):
        n_uv = n_d = 0
        ref, bnd = _reference(g, rec[:, 6:8])
        for o, tag in enumerate(g["tags"]):
            k = int(p["obs_patch"][o])
            if tag == "a:uv":      # on a texel: the closed form of that texel and its neighbours
                row, col, *_ = gc.stencil(rec[o, 6:8], p["scales"][k], p["corners"][k])
                want = gc.closed_form_on_a_texel(p["patches"][k], p["refs"][p["obs_point"][o]], row, col, p["scales"][k], g["l2"])
                assert (np.abs(rec[o, :6].astype(gc.LD) - want) <= bnd[o]).all(), (name, o)
                n_uv += 1
            if tag == "d":         # 50 texels outside: the cell index is limited, the fraction is the same: the same record
                assert np.array_equal(_bits(rec[o, :6]), _bits(rec[o + 1, :6])), (name, o)
                n_d += 1
        assert n_uv == 3 * len(gc.PATCH_FRAMES) and n_d == 4 * len(gc.PATCH_FRAMES)


@pytest.mark.parametrize("name", ["smooth-C128-float16-l2-n200", "noise-C64-float32-l2-n65", "placed-C64-float16-raw-n195"])
def test_two_runs_give_the_same_bytes(ctx, name):
    from pixsfm_amd.engine import interp_cfg
    g = _group(name)
    cfg = interp_cfg(l2_normalize=g["l2"])
    runs = []
    for _ in range(2):
        arena, ba = _open(ctx, g["prob"])
        rec, built = ba.eval_gram(cfg, reset=True)
        runs.append(rec.download().tobytes())
        assert built == ba.n_obs
        arena.close()
    assert runs[0] == runs[1]


def _interior_problem(C, dtype, n, seed, noise):
    """n placed observations in cells 1 .. n - 3 with fractions in [1/8, 5/8]: a quarter texel stays in the cell, a whole texel
    changes the cell and keeps the stencil inside the patch."""
    rng = np.random.default_rng(seed)
    uv = np.column_stack([rng.integers(1, gc.W - 3, n) + rng.integers(128, 641, n) / 1024.0,
                          rng.integers(1, gc.H - 3, n) + rng.integers(128, 641, n) / 1024.0])
    feats = (gc.noise_features if noise else gc.smooth_features)(rng, n, C).astype(dtype)
    prob, xy = gc.placed_problem(uv, gc.PATCH_FRAMES, feats, rng=rng)
    return prob, xy


def _texel(prob):
    """(n, 2): one texel in pixels, per observation."""
    return 1.0 / prob["scales"][prob["obs_patch"]]


COMBOS_MOVED = [(128, np.float16, True, False), (64, np.float32, False, True), (128, np.float32, False, False), (64, np.float16, True, True)]


@pytest.mark.parametrize("C,dtype,l2,noise", COMBOS_MOVED)
def test_a_move_inside_the_cell_reuses_the_matrices_at_full_accuracy(ctx, C, dtype, l2, noise):
    """The case the cache exists for: every projection moves by a quarter texel, no cell changes, nothing is built -- the old G
    with new weights is as close to the reference at the NEW positions as a fresh build."""
    from pixsfm_amd.engine import interp_cfg
    prob, xy = _interior_problem(C, dtype, 65, 11, noise)
    g = dict(name="inside-%d-%s-%d-%d" % (C, np.dtype(dtype).name, l2, noise), C=C, l2=l2, prob=prob)
    arena, ba = _open(ctx, prob)
    cfg = interp_cfg(l2_normalize=l2)
    rec, built = ba.eval_gram(cfg, reset=True)
    first = rec.download().copy()
    assert built == ba.n_obs and _ratio(g, first).max() <= 1.0
    moved = xy + 0.25 * _texel(prob)
    ba.d["xyz"].upload(np.column_stack([moved, np.ones(len(moved))]))
    rec, built = ba.eval_gram(cfg, reset=False)
    rec = rec.download().copy()
    arena.close()
    assert built == 0
    assert np.array_equal(_bits(rec[:, 6:8]), _bits(moved))
    assert (rec[:, :6] != first[:, :6]).any(axis=1).all()                                # every record is a new one
    ratio = _ratio(g, rec)
    print("%-32s moved inside the cell: worst error / bound %.4f (%.1f x 2^-53 scale)" % (g["name"], ratio.max(), ratio.max() * gc.K(C, l2)))
    assert ratio.max() <= 1.0


FLAG_SETS = [[], [0], list(range(0, 130, 8)), list(range(64)), [63, 64], [129], list(range(8, 17)), list(range(130))]


@pytest.mark.parametrize("C,dtype,l2,noise", COMBOS_MOVED[:2])
def test_exactly_the_flagged_observations_are_rebuilt_and_the_others_keep_their_bits(ctx, C, dtype, l2, noise):
    """130 observations = two full 64-blocks and two: index sets with 0, 1, 8, 9, 17, 64, 130 flagged observations (1, 8, 9 and 64
    inside one 64-block of the second pass, a pair across the block boundary, the last observation alone) move by one texel."""
    from pixsfm_amd.engine import interp_cfg
    n = 130
    prob, xy = _interior_problem(C, dtype, n, 13, noise)
    g = dict(name="flags-%d-%s-%d-%d" % (C, np.dtype(dtype).name, l2, noise), C=C, l2=l2, prob=prob)
    arena, ba = _open(ctx, prob)
    cfg = interp_cfg(l2_normalize=l2)
    rec, built = ba.eval_gram(cfg, reset=True)
    first = rec.download().copy()
    assert built == n and _ratio(g, first).max() <= 1.0
    home = np.column_stack([xy, np.ones(n)])
    worst = 0.0
    for idx in FLAG_SETS:
        idx = np.array(idx, dtype=np.int64)
        away = home.copy()
        away[idx, 0] += _texel(prob)[idx, 0]
        ba.d["xyz"].upload(away)
        rec, built = ba.eval_gram(cfg, reset=False)
        rec = rec.download().copy()
        assert built == len(idx), (idx.tolist(), built)
        keep = np.setdiff1d(np.arange(n), idx)
        assert np.array_equal(_bits(rec[keep]), _bits(first[keep])), idx.tolist()              # unmoved: the previous call's bits
        assert np.array_equal(_bits(rec[idx, 6:8]), _bits(away[idx, :2]))
        if len(idx):
            assert (rec[idx, :6] != first[idx, :6]).any(axis=1).all()
            ratio = _ratio(g, rec, idx)
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= 1.0, (idx.tolist(), float(ratio.max()))
        ba.d["xyz"].upload(home)
        rec, built = ba.eval_gram(cfg, reset=False)
        assert built == len(idx), (idx.tolist(), built)
        assert np.array_equal(_bits(rec.download()), _bits(first)), idx.tolist()                # and back: the first call's bits
    arena.close()
    print("%-32s flagged rebuilds: worst error / bound %.4f (%.1f x 2^-53 scale)" % (g["name"], worst, worst * gc.K(C, l2)))
