"""The reference, the float64 restatement and the bound of tests/gram_cases.py, checked against each other and the oracle
before tests/test_gram_records_gpu.py holds the device to them.  No GPU."""
import numpy as np
import pytest

import gram_cases as gc
from conftest import FP32_PASS_RECORD_ATOL


def _xy(g):
    return g["planned"] if g["planned"] is not None else gc.host_xy(g["prob"])


@pytest.fixture(scope="module")
def references():
    """name -> (group, xy, reference records, bounds): computed once, read by every test, never written."""
    out = {}
    for g in gc.groups():
        xy = _xy(g)
        ref, bnd = gc.reference_and_bound(g, xy)
        ref.setflags(write=False), bnd.setflags(write=False)
        out[g["name"]] = (g, xy, ref, bnd)
    return out


def test_the_restatement_is_within_the_derived_bound_of_the_reference(references):
    """The reference alone stays inside the bound: the algebra on G in float64 -- the device's grouping, numpy's order inside the
    C-term contractions -- against the per-channel long-double statement, every group, every entry."""
    worst_ratio, worst_units = 0.0, 0.0
    for name, (g, xy, ref, bnd) in references.items():
        got = np.stack(gc.evaluate(g, xy, gc.restated_record))
        assert np.isfinite(got).all(), name
        ratio = np.abs(got.astype(gc.LD) - ref) / bnd
        print("%-32s worst error / bound %.4f  (%.1f x 2^-53 scale)" % (name, ratio.max(), ratio.max() * gc.K(g["C"], g["l2"])))
        assert ratio.max() <= 1.0, (name, np.unravel_index(ratio.argmax(), ratio.shape), float(ratio.max()))
        worst_ratio = max(worst_ratio, float(ratio.max()))
        worst_units = max(worst_units, float(ratio.max()) * gc.K(g["C"], g["l2"]))
    print("worst: %.4f of the bound, %.1f x 2^-53 scale" % (worst_ratio, worst_units))


def test_the_bound_is_four_orders_below_the_fp32_pass_tolerance_on_unit_norm_features(references):
    """What the derived bound buys: on smooth unit-norm features in a frame of scale 1 it is below 1e-4 * FP32_PASS_RECORD_ATOL
    for every entry of every position (a)-(d)."""
    for name, (g, xy, ref, bnd) in references.items():
        if not name.startswith("placed"):
            continue
        p = g["prob"]
        unit = np.array([tuple(p["scales"][int(k)]) == (1.0, 1.0) for k in p["obs_patch"]])
        assert unit.sum() == len(gc.planned_positions())
        assert bnd[unit].max() < 1e-4 * FP32_PASS_RECORD_ATOL, (name, float(bnd[unit].max()))


# the content whose entries are in the range FP32_PASS_RECORD_ATOL is stated for (tests/conftest.py: "entries of magnitude
# 1e-2 .. 1"): texels and references of norm ~1.  The other groups scale the features (x300, x1e-3) or plant +-65504 / 1e5 among
# them; an absolute 2e-7 says nothing there.
UNIT_CONTENT = ("placed", "smooth", "noise", "selfref")
SMOOTH_UNIT_NORM = ("placed", "smooth")          # entries up to ~1: the constant as it stands


def test_the_reference_agrees_with_the_oracle_to_the_fp32_pass(references):
    """The long-double reference against the oracle's PatchInterpolator (pxo.patch_eval: the reference implementation's fp32
    horizontal pass restated), the six entries formed from its f, df/dx, df/dy in the same way.
    * Smooth unit-norm features (every placed position (a)-(e) and the shared-patch group): entries up to ~1, what
      FP32_PASS_RECORD_ATOL = 2e-7 is stated for.  Asserted as it stands, absolute.
    * White noise and the self-reference groups: same texel norms, but Gram entries of 10 .. 100 (neighbouring texels are
      unrelated, the derivatives are as large as the features).  The fp32 pass rounds every TERM of an entry at 6e-8 relative and
      the terms reach  m = max(1, scale)  with the scale of gram_cases.bound ((B tau)^2 s_a s_b for a Gram entry, ...), so there
      the assertion is  |difference| <= FP32_PASS_RECORD_ATOL * m.
    Measured here, the justification of the constant: smooth unit-norm 6.5e-8 absolute (C = 64, fp32 storage, l2 off; fp16
    storage stays at 6e-9); white noise 1.8e-6 absolute = 1.6e-7 of m (C = 64, fp16, l2 off)."""
    worst = {True: (0.0, ""), False: (0.0, "")}
    for name, (g, xy, ref, bnd) in references.items():
        if not name.startswith(UNIT_CONTENT):
            continue
        got = np.stack(gc.evaluate(g, xy, gc.oracle_record))
        diff = np.abs(got.astype(gc.LD) - ref).astype(np.float64)
        plain = name.startswith(SMOOTH_UNIT_NORM)
        m = 1.0 if plain else np.maximum(1.0, (bnd / (gc.K(g["C"], g["l2"]) * gc.U)).astype(np.float64))
        print("%-32s worst |oracle - reference| %.2e absolute, %.2e of %s" % (name, diff.max(), (diff / m).max(), "1" if plain else "m"))
        assert (diff <= FP32_PASS_RECORD_ATOL * m).all(), (name, float((diff / m).max()))
        worst[plain] = max(worst[plain], (float((diff / m).max()), name))
    print("worst distance to the oracle: smooth unit-norm %.2e absolute (%s); white noise %.2e of m (%s)" % (worst[True] + worst[False]))


def test_closed_forms_where_the_projection_is_on_a_texel(references):
    """(a) Fraction 0 in u and v: the record is the texel's own -- f the texel, the derivatives central differences.  Fraction 0 in
    one direction: the taps of the other three columns (rows) carry weight exactly 0."""
    n_uv = 0
    for name, (g, xy, ref, bnd) in references.items():
        if not name.startswith("placed"):
            continue
        p = g["prob"]
        for o, tag in enumerate(g["tags"]):
            if not tag.startswith("a:"):
                continue
            k = int(p["obs_patch"][o])
            row, col, fu, fv, _, _ = gc.stencil(xy[o], p["scales"][k], p["corners"][k])
            assert (fu == 0.0) == ("u" in tag[2:]) and (fv == 0.0) == ("v" in tag[2:])
            wu, _ = gc.catmull_rom(fu, gc.LD)
            wv, _ = gc.catmull_rom(fv, gc.LD)
            if fu == 0.0:
                assert np.array_equal(wu, [0, 1, 0, 0])
            if fv == 0.0:
                assert np.array_equal(wv, [0, 1, 0, 0])
            if tag == "a:uv":
                want = gc.closed_form_on_a_texel(p["patches"][k], p["refs"][p["obs_point"][o]], row, col, p["scales"][k], g["l2"])
                # both are long-double evaluations of the same numbers: a few hundred of ITS roundings, 1e-3 of the bound
                assert (np.abs(want - ref[o]) <= 1e-3 * bnd[o]).all(), (name, o)
                n_uv += 1
    assert n_uv == 3 * len(gc.PATCH_FRAMES) * len(gc.COMBOS)


def test_positions_far_outside_equal_the_clamp_limit(references):
    """(d) 50 texels outside on each side: the cell index is limited, every tap clamps onto the border: the same record as at
    the limit with the same fraction."""
    n = 0
    for name, (g, xy, ref, bnd) in references.items():
        if not name.startswith("placed"):
            continue
        for o, tag in enumerate(g["tags"]):
            if tag == "d":
                assert g["tags"][o + 1] == "d=" and np.array_equal(ref[o], ref[o + 1])
                n += 1
    assert n == 4 * len(gc.PATCH_FRAMES) * len(gc.COMBOS)


def test_the_weight_norms_and_roundings_the_derivation_uses():
    """|w|_1 <= 1.5625 and |wc|_1, |wr|_1 <= 3.75 in two dimensions (1.25 and 3 in one), A >= 1 and B >= 1, and the float64
    weights are within 27 u / 39 u (1-norm over the taps) of the long-double ones."""
    xs = np.concatenate([np.linspace(0.0, 1.0, 4001)[:-1], 1.0 - 2.0 ** -np.arange(1, 54), 2.0 ** -np.arange(1, 60)])
    a1 = d1 = 0.0
    dmin = np.inf
    ew = ed = 0.0
    for x in xs:
        w, dw = gc.catmull_rom(x, gc.LD)
        w64, dw64 = gc.catmull_rom(x, np.float64)
        a1, d1, dmin = max(a1, float(np.abs(w).sum())), max(d1, float(np.abs(dw).sum())), min(dmin, float(np.abs(dw).sum()))
        assert abs(float(w.sum()) - 1.0) < 1e-17 and abs(float(dw.sum())) < 1e-17
        ew, ed = max(ew, float(np.abs(w64 - w).sum()) / gc.U), max(ed, float(np.abs(dw64 - dw).sum()) / gc.U)
    print("1-D: |w|_1 <= %.6f, %.6f <= |w'|_1 <= %.6f; float64 weights off by %.2f u and %.2f u" % (a1, dmin, d1, ew, ed))
    assert a1 <= 1.25 and a1 ** 2 <= 1.5625
    assert d1 <= 3.0 and a1 * d1 <= 3.75 and dmin >= 1.0
    assert ew <= gc.E_W1 and ed <= gc.E_D1
    for g in gc.groups()[:2]:                       # ... and as the reference reports them
        res = gc.evaluate(g, _xy(g))
        assert all(1.0 <= q["A"] <= 1.5625 and 1.0 <= q["B"] <= 3.75 for _, q in res)


def test_the_cases_cover_what_they_claim():
    gs = gc.groups()
    assert {(g["C"], g["dtype"], g["l2"]) for g in gs if g["name"].startswith("placed")} == set(gc.COMBOS)
    assert all(g["prob"]["patches"].shape[1:3] == (gc.H, gc.W) == (7, 9) for g in gs)
    assert max(len(g["prob"]["obs_image"]) for g in gs) <= 200
    tags = gs[0]["tags"]
    clamped = set()
    for o, t in enumerate(tags[:len(gc.planned_positions())]):
        if t == "c":
            row, col, *_ = gc.stencil(gs[0]["planned"][o], (1.0, 1.0), (0, 0))
            nc = lambda i, n: sum(1 for k in range(4) if not 0 <= i - 1 + k <= n - 1)
            clamped.add((nc(row, gc.H), nc(col, gc.W)))
    assert clamped == {(a, b) for a in range(4) for b in range(4)}          # 0..3 taps clamped, each direction, every corner
    for g in gs:                                                            # several observations per point, shared patches
        p = g["prob"]
        if g["planned"] is None and len(p["obs_image"]) >= 7:
            assert len(set(p["obs_patch"])) < len(p["obs_patch"]) and np.bincount(p["obs_point"]).max() > 1
        assert np.all(np.log2(p["scales"]) % 1 == 0)                        # powers of two
        assert not np.array_equal(p["obs_patch"], np.arange(len(p["obs_patch"]))) or len(p["obs_patch"]) == 1
    edge = next(g for g in gs if g["name"].startswith("f16edge"))["prob"]["patches"]
    assert (edge == 65504).any() and (edge == -65504).any() and ((np.abs(edge) < 2.0 ** -14) & (edge != 0)).any()
