"""CPU: the minimal solvers against an independent reference (tests/minimal_solver_ref.py: mpmath at 60 digits, written from each
problem's definition), on hard families of noise-free samples (hard_family of tests/*_cases.py).  Two implementations of every
solver are held to the same bound: the numpy restatement of tests/*_cases.py, and the kernel's own device functions compiled as
host code (extern "C" wrappers in tests/lane_emulation/*_on_host.cpp).

The bound.  kappa is the 2-norm of d(model) / d(sample coordinates) at an mp solution, u = 2^-53.  Every real mp solution must
have a returned hypothesis within C kappa u, and no sample may return more hypotheses than mp has solutions.  C is 100 x the
largest err / (kappa u) that an attainable-level computation leaves on the generic family: three Newton steps in double on the
problem's defining equations from the mp solution rounded to double.  The factor 100 covers a direct solver's operation count
over a polished one.  A solution with C kappa u above 1e-7 (ms.CAP) is ill-conditioned by construction: counted, left out, and a
family's share of them is bounded from the mp reference alone (EXCLUDED_SHARE)."""
import ctypes as C
import functools

import numpy as np
import pytest

import abspose_cases as ac
import fundamental_cases as fc
import homography_cases as hc
import lanes
import minimal_solver_ref as ms
import twoview_cases as tv
from lanes import p as _p

# Measured on 64 samples of each solver's generic family (seed 1), printed by test_attainable_level:
ATTAINABLE_P3P = 25.0          # largest err / (kappa u) of the polished pose: 22.2
ATTAINABLE_SEVEN = 2.0         # of the polished F, over the three focal scales: 1.4
ATTAINABLE_FOUR = 0.6          # of the polished H: 0.53
ATTAINABLE_FIVE = 6.0          # of the polished E: 5.2
C_P3P, C_SEVEN, C_FOUR, C_FIVE = 100 * ATTAINABLE_P3P, 100 * ATTAINABLE_SEVEN, 100 * ATTAINABLE_FOUR, 100 * ATTAINABLE_FIVE

SEED = 1
CONSTRUCTED = 8                # samples of a family whose every member is found by a search (bisection onto a threshold)
EXCLUDED_SHARE = 0.05          # of a family's solutions may be ill-conditioned (bound above ms.CAP); the mp reference alone decides that


def _pose_distance(h, s):
    return ms.pose_error(h[0], h[1], s["R"], s["t"])


def _f_distance(h, s):
    return ms.projective_distance(h, s["F"])


def _h_distance(h, s):
    return hc.h_distance(h, s["H"])


# ---- the implementations under test: samples of a family -> the hypotheses of every sample -----------------------------------------
def _p3p_samples(name, B):
    uv, X, _, _ = ac.hard_family(name, SEED, B)
    return list(zip(uv, X))


def _p3p_restatement(samples):
    return [[(R, t) for _, R, t in ac.p3p(uv, X)] for uv, X in samples]


def _p3p_lanes(lib, samples):
    n = len(samples)
    rec = np.ascontiguousarray([np.concatenate([uv, X], 1) for uv, X in samples], np.float64)
    R, t, valid = np.full((n, 4, 9), np.nan), np.full((n, 4, 3), np.nan), np.zeros((n, 4), np.uint8)
    lib.emu_p3p(C.c_int(n), _p(rec), _p(R), _p(t), _p(valid))
    assert np.isfinite(R[valid == 1]).all() and np.isfinite(t[valid == 1]).all()
    return [[(R[b, r].reshape(3, 3), t[b, r]) for r in range(4) if valid[b, r]] for b in range(n)]


def _seven_restatement(samples):
    F, valid = fc.seven_point(np.array(samples))
    assert np.isfinite(F[valid]).all()
    return [[F[b, r] for r in range(3) if valid[b, r]] for b in range(len(samples))]


def _seven_lanes(lib, samples):
    n = len(samples)
    rec = np.ascontiguousarray(samples, np.float64)
    F, valid = np.full((n, 3, 9), np.nan), np.zeros((n, 3), np.uint8)
    lib.emu_seven_point(C.c_int(n), _p(rec), _p(F), _p(valid))
    assert np.isfinite(F[valid == 1]).all()
    return [[F[b, r] for r in range(3) if valid[b, r]] for b in range(n)]


def _e_distance(h, s):
    return ms.projective_distance(h, s["E"])


def _five_restatement(samples):
    E, valid = tv.five_point(np.array(samples))
    assert np.isfinite(E[valid]).all()
    return [[E[b, r] for r in range(10) if valid[b, r]] for b in range(len(samples))]


def _five_lanes(lib, samples):
    n = len(samples)
    rec = np.ascontiguousarray(samples, np.float64)
    E, valid = np.full((n, 10, 9), np.nan), np.zeros((n, 10), np.uint8)
    lib.emu_five_point(C.c_int(n), _p(rec), _p(E), _p(valid))
    assert np.isfinite(E[valid == 1]).all()
    return [[E[b, r] for r in range(10) if valid[b, r]] for b in range(n)]


def _four_restatement(samples):
    H, ok = hc.four_point(np.array(samples))
    assert np.isfinite(H[ok]).all()
    return [[H[b]] if ok[b] else [] for b in range(len(samples))]


def _four_lanes(lib, samples):
    n = len(samples)
    rec = np.ascontiguousarray(samples, np.float64)
    H, valid = np.full((n, 9), np.nan), np.zeros(n, np.uint8)
    lib.emu_four_point(C.c_int(n), _p(rec), _p(H), _p(valid))
    assert np.isfinite(H[valid == 1]).all()
    return [[H[b]] if valid[b] else [] for b in range(n)]


SOLVERS = {
    "P3P": dict(cases=ac, samples=_p3p_samples, mp=lambda s: ms.p3p(*s), restatement=_p3p_restatement, lanes=_p3p_lanes,
                source="abspose_on_host.cpp", distance=_pose_distance, C=C_P3P,
                constructed=("A4 above LEAD_TOL", "A4 below LEAD_TOL"), refused=()),
    "seven-point": dict(cases=fc, samples=lambda name, B: list(fc.hard_family(name, SEED, B)[0]), mp=ms.seven_point,
                        restatement=_seven_restatement, lanes=_seven_lanes, source="fundamental_on_host.cpp", distance=_f_distance, C=C_SEVEN,
                        constructed=("double root", "leading coefficient above LEAD_TOL", "leading coefficient below LEAD_TOL"),
                        refused=fc.REFUSED_FAMILIES),
    "five-point": dict(cases=tv, samples=lambda name, B: list(tv.hard_family(name, SEED, B)[0]), mp=lambda rec: ms.five_point(rec)[0],
                       restatement=_five_restatement, lanes=_five_lanes, source="twoview_on_host.cpp", distance=_e_distance, C=C_FIVE,
                       constructed=("double root", "leading coefficient above LEAD_TOL", "leading coefficient below LEAD_TOL"),
                       refused=tv.REFUSED_FAMILIES),
    "four-point": dict(cases=hc, samples=lambda name, B: list(hc.hard_family(name, SEED, B)[0]), mp=ms.four_point,
                       restatement=_four_restatement, lanes=_four_lanes, source="homography_on_host.cpp", distance=_h_distance, C=C_FOUR,
                       constructed=(), refused=()),
}
CASES = [(solver, name) for solver, S in SOLVERS.items() for name in S["cases"].HARD_FAMILIES]


@functools.lru_cache(maxsize=None)
def family(solver, name, B=64):
    """(samples, mp solutions of every sample), computed once per session."""
    S = SOLVERS[solver]
    samples = S["samples"](name, CONSTRUCTED if name in S["constructed"] else B)
    return samples, [S["mp"](s) for s in samples]


def bounded(solver, name):
    """Whether a family is held to the bound: all but the five-point families below tv.FIVE_POINT_MIN_PARALLAX.  Those are
    measured: everything valid is finite (asserted in the wrappers), the root stage of either implementation is held to its own
    polynomial (test_root_stage), and the count of solutions within the bound is printed."""
    return solver != "five-point" or tv.PARALLAX_FAMILIES.get(name, 1.0) >= tv.FIVE_POINT_MIN_PARALLAX


def check(solver, name, what, hypotheses, samples, solutions, refused=False):
    """Hold one implementation's hypotheses of a family to the bound; returns the worst err / (kappa u)."""
    S = SOLVERS[solver]
    n_mp, n_ret = sum(map(len, solutions)), sum(map(len, hypotheses))
    if refused:          # the solver's own rule gives no hypothesis here, though mp finds the problem solvable
        print("%s / %s, %s: refused by the solver's rule -- %d samples, mp %d solutions, returned %d" % (solver, name, what, len(samples), n_mp, n_ret))
        assert n_ret == 0 and n_mp > 0
        return 0.0
    worst, excluded, met, judged = 0.0, 0, 0, 0
    for hyp, sol in zip(hypotheses, solutions):
        ratios, ex = ms.judge(sol, hyp, S["distance"], S["C"])
        worst, excluded = max([worst] + ratios), excluded + ex
        met, judged = met + sum(r <= S["C"] for r in ratios), judged + len(ratios)
        assert not bounded(solver, name) or len(hyp) <= len(sol), "more hypotheses than real solutions"
    share = excluded / max(n_mp, 1)
    print("%s / %s, %s: %d samples, excluded share %.3f, %d of %d solutions within the bound, worst err / (kappa u) %.3g (C = %g), "
          "mp solutions %d, returned %d" % (solver, name, what, len(samples), share, met, judged, worst, S["C"], n_mp, n_ret))
    if bounded(solver, name):
        assert n_mp > 0 and share <= EXCLUDED_SHARE
        assert worst <= S["C"]
    return worst


@pytest.mark.parametrize("solver,name", CASES)
def test_restatement_against_the_mp_reference(solver, name):
    samples, solutions = family(solver, name)
    check(solver, name, "restatement", SOLVERS[solver]["restatement"](samples), samples, solutions, name in SOLVERS[solver]["refused"])


@pytest.mark.parametrize("solver,name", CASES)
def test_kernel_source_against_the_mp_reference(solver, name, tmp_path_factory):
    lib, _ = lanes.load(tmp_path_factory, SOLVERS[solver]["source"])
    samples, solutions = family(solver, name)
    check(solver, name, "kernel source", SOLVERS[solver]["lanes"](lib, samples), samples, solutions, name in SOLVERS[solver]["refused"])


@pytest.mark.parametrize("name", [n for n in tv.HARD_FAMILIES if not bounded("five-point", n)])
def test_five_point_outside_the_range_kernel_source_and_restatement_agree(name, tmp_path_factory):
    """Below tv.FIVE_POINT_MIN_PARALLAX no bound is asserted.  The kernel's source and the restatement still find the same number
    of hypotheses, sample by sample, and each finds the roots of its own polynomial (test_root_stage).  The hypotheses' values are
    printed, not compared, so the issue's "kernel and restatement agree" is met only that far: the elimination to det B(z)
    amplifies the two compilers' different roundings without limit as the parallax falls -- the largest difference between
    unit-norm matrices was measured at 2.3e-3 (parallax 1e-2), 3.3e-2 (1e-3) and 1.6 (1e-4), against 6e-13 inside the range --
    and no tolerance short of the matrices' own size could be derived for it."""
    lib, _ = lanes.load(tmp_path_factory, "twoview_on_host.cpp")
    samples, _ = family("five-point", name)
    worst = 0.0
    for a, b in zip(_five_restatement(samples), _five_lanes(lib, samples)):
        assert len(a) == len(b)
        for x in a:
            worst = max(worst, min(float(np.linalg.norm(x / np.linalg.norm(x) - y / np.linalg.norm(y))) for y in b))
    print("five-point / %s: largest difference between kernel source and restatement %.3g" % (name, worst))


def _stage(lib, fn, samples, deg):
    n = len(samples)
    c, nr, z = np.zeros((n, deg + 1)), np.zeros(n, np.int32), np.full((n, deg), np.nan)
    getattr(lib, fn)(C.c_int(n), _p(np.ascontiguousarray(samples, np.float64)), _p(c), _p(nr), _p(z))
    return c, nr, z


ROOT_CASES = [("five-point", n) for n in tv.HARD_FAMILIES if n not in tv.REFUSED_FAMILIES] + \
             [("seven-point", n) for n in fc.HARD_FAMILIES if n not in fc.REFUSED_FAMILIES]


@pytest.mark.parametrize("solver,name", ROOT_CASES)
def test_root_stage(solver, name, tmp_path_factory):
    """The Sturm chain, the bisection and the Newton steps, which the polish of the five-point hypotheses would otherwise hide: the
    roots that either implementation returns for its own polynomial (before any polish), against that polynomial's roots in mp.
    The count of real roots is equal, and every simple root is within the bound of ms.polynomial_roots -- what Horner's scheme
    in double lets a sign-based root finder resolve, 2 n u sum |c_k z^k| / |p'(z)| + u |z|, no constant of this test's own.
    Measured: at most 0.46 of that bound.  With NEWTON = 0 the restatement reaches 1.2 of it on the generic five-point family
    (red); with BISECT halved alone the Newton steps still converge (0.17, green: the two stages cover each other in that
    direction); with both 2e9.  On every family, the low-parallax ones included: this stage is not where those lose their roots."""
    five = solver == "five-point"
    samples, _ = family(solver, name)
    samples = samples[:16]
    det = (tv.five_point if five else fc.seven_point)(np.array(samples), details=True)[2]
    lib, _ = lanes.load(tmp_path_factory, "twoview_on_host.cpp" if five else "fundamental_on_host.cpp")
    kc, knr, kz = _stage(lib, "emu_five_point_roots" if five else "emu_seven_point_roots", samples, 10 if five else 3)
    worst = 0.0
    for what, c, nr, z in (("restatement", det["c_scaled"] if five else det["c"], np.where(det["ok"], det["n_roots"], -1), det["roots"]), ("kernel source", kc, knr, kz)):
        for b in range(len(samples)):
            if nr[b] < 0:
                continue
            ref = ms.polynomial_roots(c[b])
            assert len(ref) == nr[b], (what, b)
            for k, (zm, bound) in enumerate(ref):
                if np.isfinite(bound):
                    worst = max(worst, abs(z[b, k] - zm) / bound)
    assert (knr == np.where(det["ok"], det["n_roots"], -1)).all()
    print("%s / %s: root stage, worst |dz| / bound %.3g" % (solver, name, worst))
    assert worst <= 1.0


def test_attainable_level():
    """The constants C: the error that three Newton steps in double on the defining equations leave on the generic families,
    in units of kappa u.  The measured values are written next to ATTAINABLE_* above and in docs/NUMBERS_HISTORY.md."""
    worst = dict.fromkeys(("P3P", "five-point", "seven-point", "four-point"), 0.0)
    for rec, sols in zip(*family("five-point", "generic")):
        for s in sols:
            worst["five-point"] = max(worst["five-point"], _e_distance(ms.attainable_five_point(rec, s), s) / (s["kappa"] * ms.U))
    for (uv, X), sols in zip(*family("P3P", "generic")):
        for s in sols:
            R, t = ms.attainable_p3p(uv, X, s)
            worst["P3P"] = max(worst["P3P"], ms.pose_error(R, t, s["R"], s["t"]) / (s["kappa"] * ms.U))
    for name in ("generic, focal x 0.7", "generic, focal x 1", "generic, focal x 1.4"):
        for rec, sols in zip(*family("seven-point", name)):
            for s in sols:
                worst["seven-point"] = max(worst["seven-point"], fc.f_distance(fc.signed(ms.attainable_seven_point(rec, s)), s["F"]) / (s["kappa"] * ms.U))
    for rec, sols in zip(*family("four-point", "generic")):
        for s in sols:
            worst["four-point"] = max(worst["four-point"], hc.h_distance(ms.attainable_four_point(rec, s), s["H"]) / (s["kappa"] * ms.U))
    print("attainable err / (kappa u): P3P %.3g, five-point %.3g, seven-point %.3g, four-point %.3g"
          % (worst["P3P"], worst["five-point"], worst["seven-point"], worst["four-point"]))
    assert worst["five-point"] <= ATTAINABLE_FIVE
    assert worst["P3P"] <= ATTAINABLE_P3P and worst["seven-point"] <= ATTAINABLE_SEVEN and worst["four-point"] <= ATTAINABLE_FOUR


@pytest.mark.parametrize("solver,name", CASES)
def test_generating_model_is_among_the_mp_solutions(solver, name):
    """The reference against ground truth, on every family that has one: the model that generated a noise-free sample is one of
    its mp solutions, to the rounding of the sample's own coordinates (kappa u, with a factor 10 for the 15 to 28 coordinates
    rounded)."""
    S = SOLVERS[solver]
    samples, solutions = family(solver, name)
    truth = S["cases"].hard_family(name, SEED, len(samples))
    worst, n = 0.0, 0
    for b, sols in enumerate(solutions):
        if solver == "P3P":
            dist = [ms.pose_error(s["R"], s["t"], truth[2][b], truth[3][b]) / (s["kappa"] * ms.U) for s in sols]
        elif not np.isfinite(truth[1][b]).all():
            continue
        else:
            dist = [S["distance"](truth[1][b], s) / (s["kappa"] * ms.U) for s in sols]
        worst, n = max(worst, min(dist)), n + 1
    print("%s / %s: generating model among the mp solutions of %d samples, worst %.3g kappa u" % (solver, name, n, worst))
    assert worst <= 10.0


def test_degenerate_samples_give_no_hypothesis(tmp_path_factory):
    """Coincident points, collinear points, a pure rotation, a coordinate that is not a number: nothing valid from either
    implementation (what is valid is finite: asserted inside the wrappers)."""
    uv, X = ac.degenerate_samples()
    samples = list(zip(uv, X))
    assert not any(_p3p_restatement(samples)) and not any(_p3p_lanes(lanes.load(tmp_path_factory, "abspose_on_host.cpp")[0], samples))
    rec = list(fc.degenerate_samples())
    assert not any(_seven_restatement(rec)) and not any(_seven_lanes(lanes.load(tmp_path_factory, "fundamental_on_host.cpp")[0], rec))
    rec = list(tv.degenerate_samples())
    assert not any(_five_restatement(rec)) and not any(_five_lanes(lanes.load(tmp_path_factory, "twoview_on_host.cpp")[0], rec))
    rec = list(hc.degenerate_samples())
    assert not any(_four_restatement(rec)) and not any(_four_lanes(lanes.load(tmp_path_factory, "homography_on_host.cpp")[0], rec))
