"""GPU: one solver hypothesis per query or pair through the public entry points, held to the mp reference of
tests/minimal_solver_ref.py with the bound of tests/test_minimal_solvers_cpu.py (C kappa u) and to the numpy restatement's winner
with the existing tolerances of tests/*_cases.py.

With exactly the minimal sample every root fits its points to rounding, so which root an estimator returns is decided by sums of
1e-32: the returned model is judged against the mp solution nearest to it (left out where that one is ill-conditioned), and the
five-point estimator, whose ten roots the GPU and the restatement rank differently (rotations 3.1 rad apart), is compared with
the restatement in everything discrete and by its E against the restatement's hypotheses of the same sample.

A pair carries exactly the minimal sample (5, 7 or 4 matches); one trial, no local optimisation, no refinement: what comes back
is the solver's best hypothesis.  A query carries four correspondences, not three -- fewer than four is status 1 by the
estimator's contract: the hard triple sits where sample 0 of four draws its three indices, and the fourth is one more
noise-free correspondence of the same pose, which leaves the hypothesis itself untouched and only picks the root.

16 samples of every family (4 of the constructed ones) in one batch per solver, pinhole cameras.  The mp solutions are computed
from the normalised coordinates as the kernels form them, (x - cx) / fx in double."""
import numpy as np
import pytest

import abspose_cases as ac
import fundamental_cases as fc
import homography_cases as hc
import minimal_solver_ref as ms
import test_minimal_solvers_cpu as cpu
import triangulation_cases as tc
import twoview_cases as tv
from pixsfm_amd import synthetic

pytestmark = pytest.mark.gpu

B, B_CONSTRUCTED = 16, 4
K = np.array(tc.MODEL_PARAMS[1], dtype=np.float64)            # pinhole: fx, fy, cx, cy
ONE_TRIAL = dict(lo_rounds=0, refine_max_iterations=0, min_inlier_ratio=0.0, min_num_trials=1, max_num_trials=1, round_size=1)


def _pixels(x):
    return np.asarray(x) * K[:2] + K[2:]


def _normalised(xy):
    return (np.asarray(xy) - K[2:]) / K[:2]


def _families(solver):
    """[(name, samples)] of a solver, in the order of its HARD_FAMILIES."""
    S = cpu.SOLVERS[solver]
    return [(name, S["samples"](name, B_CONSTRUCTED if name in S["constructed"] else B)) for name in S["cases"].HARD_FAMILIES]


def _pair_batch(recs):
    """Pairs of exactly len(rec) matches each, every pair through pinhole camera 0.  Returns (batch, the normalised records as the kernels see them)."""
    n = len(recs[0])
    xy1, xy2 = _pixels(np.concatenate([r[:, :2] for r in recs])), _pixels(np.concatenate([r[:, 2:] for r in recs]))
    batch = dict(pair_offsets=np.arange(len(recs) + 1, dtype=np.int64) * n, xy1=xy1, xy2=xy2,
                 pair_camera=np.zeros((len(recs), 2), np.int32), cam_model=np.array([1], np.int32), cam_params=tc.pad_params([K]))
    seen = np.concatenate([_normalised(xy1), _normalised(xy2)], 1).reshape(len(recs), n, 4)
    return batch, seen


def _check_pairs(solver, fams, seen, models, status, bounded=lambda name: True):
    """models (T, 9) returned for the pairs of fams in order: status 0 and within C kappa u of an mp solution, family by family."""
    S, p = cpu.SOLVERS[solver], 0
    for name, samples in fams:
        worst, met, total = 0.0, 0, 0
        for _ in samples:
            if name in S["refused"]:
                assert status[p] == 2, (name, p, status[p])
            else:
                assert status[p] == 0 and np.isfinite(models[p]).all(), (name, p, status[p])
                near = min(S["mp"](seen[p]), key=lambda s: S["distance"](models[p], s))
                if S["C"] * near["kappa"] * ms.U <= ms.CAP:        # (an ill-conditioned solution is left out, as on the CPU)
                    ratio = S["distance"](models[p], near) / (near["kappa"] * ms.U)
                    worst, met, total = max(worst, ratio), met + (ratio <= S["C"]), total + 1
            p += 1
        print("%s / %s on the GPU: %d of %d samples within the bound, worst err / (kappa u) %.3g (C = %g)" % (solver, name, met, total, worst, S["C"]))
        if bounded(name):
            assert met == total, (solver, name)
    assert p == len(models)


def test_p3p(ctx):
    from pixsfm_amd.engine import AbsolutePoseProblem
    fams = _families("P3P")
    order = list(ac.sample(0, 0, 4))                           # where sample 0 of a query of four draws its triple
    extra = [i for i in range(4) if i not in order][0]
    rng = np.random.default_rng(5)
    xy, xyz, seen = [], [], []
    for name, samples in fams:
        _, _, R, t = ac.hard_family(name, cpu.SEED, len(samples))
        for b, (uv, X) in enumerate(samples):
            P4 = np.append(rng.uniform(-0.3, 0.3, 2), 1.0) * rng.uniform(2.0, 20.0)
            q_uv, q_X = np.zeros((4, 2)), np.zeros((4, 3))
            q_uv[order], q_X[order] = uv, X
            q_uv[extra], q_X[extra] = P4[:2] / P4[2], (P4 - t[b]) @ R[b]
            xy.append(_pixels(q_uv)); xyz.append(q_X)
            seen.append((_normalised(xy[-1])[order], X))
    T = len(xy)
    batch = dict(query_offsets=np.arange(T + 1, dtype=np.int64) * 4, xy=np.concatenate(xy), xyz=np.concatenate(xyz),
                 query_camera=np.zeros(T, np.int32), cam_model=np.array([1], np.int32), cam_params=tc.pad_params([K]))
    options = dict(ONE_TRIAL, min_num_inliers=3)
    out = AbsolutePoseProblem(ctx, batch).estimate(**options)
    got = {k: a.download() for k, a in zip(("qvec", "tvec", "status", "n_inliers", "n_trials", "inlier", "err"), out)}
    ac.compare(got, ac.reference(batch, **options), report="P3P, GPU vs restatement: ")
    p = 0
    for name, samples in fams:
        worst = 0.0
        for _ in samples:
            assert got["status"][p] == 0, (name, p)
            R = synthetic.qvec_to_rotmat(got["qvec"][p])
            ratios = [ms.pose_error(R, got["tvec"][p], s["R"], s["t"]) / (s["kappa"] * ms.U) for s in ms.p3p(*seen[p])
                      if cpu.C_P3P * s["kappa"] * ms.U <= ms.CAP]
            worst = max([worst] + ([min(ratios)] if ratios else []))
            p += 1
        print("P3P / %s on the GPU: worst err / (kappa u) %.3g (C = %g)" % (name, worst, cpu.C_P3P))
        assert worst <= cpu.C_P3P, name


def test_five_point(ctx):
    """Inside the accurate range (tv.FIVE_POINT_MIN_PARALLAX): the bound; status, inliers and
    trials equal the restatement's; the returned E is one of the restatement's hypotheses of that sample within fc.F_TOL (unit
    norm, sign fixed).  Outside it: status 0, finite models, and the count within the bound printed.  About a minute, nearly all
    of it the mp reference of the 204 samples on the CPU (0.3 s each at 60 digits, computed once here; the digits are kept)."""
    from pixsfm_amd.engine import TwoViewProblem
    inside = lambda name: tv.PARALLAX_FAMILIES.get(name, 1.0) >= tv.FIVE_POINT_MIN_PARALLAX
    options = dict(ONE_TRIAL, min_num_inliers=5)
    for bounded in (True, False):
        fams = [f for f in _families("five-point") if inside(f[0]) == bounded]
        batch, seen = _pair_batch([r for _, samples in fams for r in samples])
        got = {k: a.download() for k, a in zip(tv.NAMES, TwoViewProblem(ctx, batch).estimate(**options))}
        if bounded:
            ref = tv.reference(batch, **options)
            assert all(np.array_equal(got[k], ref[k]) for k in ("status", "n_inliers", "n_trials", "inlier"))
            E, valid = tv.five_point(seen)
            worst = 0.0
            for p in np.flatnonzero(got["status"] == 0):
                worst = max(worst, min(ms.projective_distance(got["E"][p], E[p, r]) for r in range(10) if valid[p, r]))
            print("five-point, GPU vs the restatement's hypotheses: max E difference %.3e" % worst)
            assert worst <= fc.F_TOL
        _check_pairs("five-point", fams, seen, got["E"], got["status"], bounded=lambda name: bounded)


def test_seven_point(ctx):
    from pixsfm_amd.engine import FundamentalProblem
    fams = _families("seven-point")
    batch, seen = _pair_batch([r for _, samples in fams for r in samples])
    options = dict(ONE_TRIAL, min_num_inliers=7)
    got = {k: a.download() for k, a in zip(fc.NAMES, FundamentalProblem(ctx, batch).estimate(**options))}
    fc.compare(got, fc.reference(batch, **options), report="seven-point, GPU vs restatement: ")
    _check_pairs("seven-point", fams, seen, got["F"], got["status"])


def test_four_point(ctx):
    from pixsfm_amd.engine import HomographyProblem
    fams = _families("four-point")
    batch, seen = _pair_batch([r for _, samples in fams for r in samples])
    options = dict(ONE_TRIAL, min_num_inliers=4)
    got = {k: a.download() for k, a in zip(hc.NAMES, HomographyProblem(ctx, batch).estimate(**options))}
    hc.compare(got, hc.reference(batch, **options), report="four-point, GPU vs restatement: ")
    _check_pairs("four-point", fams, seen, got["H"], got["status"])


def test_degenerate_samples_keep_their_sentinels(ctx):
    """No hypothesis is status 2; the rows of such pairs and queries keep what they held."""
    from pixsfm_amd.engine import AbsolutePoseProblem, FundamentalProblem, HomographyProblem, TwoViewProblem
    for Problem, recs, k, names, first in ((TwoViewProblem, tv.degenerate_samples(), 5, tv.NAMES, ("qvec", "tvec", "E")),
                                           (FundamentalProblem, fc.degenerate_samples(), 7, fc.NAMES, ("F",)),
                                           (HomographyProblem, hc.degenerate_samples(), 4, hc.NAMES, ("H", "rot_qvec"))):
        recs = [r for r in recs if np.isfinite(r).all()]        # (a coordinate that is not a number makes the pair too short: status 1)
        batch, _ = _pair_batch(recs)
        widths = dict(qvec=4, tvec=3, E=9, F=9, H=9, rot_qvec=4)
        start = {n: np.arange(len(recs) * widths[n], dtype=np.float64).reshape(len(recs), widths[n]) - 50.0 for n in first}
        out = Problem(ctx, batch).estimate(**start, **dict(ONE_TRIAL, min_num_inliers=k))
        got = {n: a.download() for n, a in zip(names, out)}
        assert (got["status"] == 2).all(), (Problem.__name__, got["status"])
        assert all(np.array_equal(got[n], start[n]) for n in first) and not got["inlier"].any() and np.isnan(got["err"]).all()
    uv, X = ac.degenerate_samples()
    keep = [b for b in range(len(uv)) if np.isfinite(X[b]).all()]
    order = list(ac.sample(0, 0, 4))
    extra = [i for i in range(4) if i not in order][0]
    xy, xyz = np.zeros((len(keep), 4, 2)), np.zeros((len(keep), 4, 3))
    for i, b in enumerate(keep):
        xy[i, order], xyz[i, order] = _pixels(uv[b]), X[b]
        xy[i, extra], xyz[i, extra] = xy[i, order[0]], xyz[i, order[0]]        # (a copy: whichever triple is drawn stays degenerate)
    batch = dict(query_offsets=np.arange(len(keep) + 1, dtype=np.int64) * 4, xy=xy.reshape(-1, 2), xyz=xyz.reshape(-1, 3),
                 query_camera=np.zeros(len(keep), np.int32), cam_model=np.array([1], np.int32), cam_params=tc.pad_params([K]))
    sq, st = np.arange(len(keep) * 4.0).reshape(-1, 4) - 50, np.arange(len(keep) * 3.0).reshape(-1, 3) - 70
    out = AbsolutePoseProblem(ctx, batch).estimate(qvec=sq, tvec=st, **dict(ONE_TRIAL, min_num_inliers=3))
    got = [a.download() for a in out]
    assert (got[2] == 2).all() and np.array_equal(got[0], sq) and np.array_equal(got[1], st)
