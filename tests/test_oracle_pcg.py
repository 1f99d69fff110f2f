"""CPU: the oracle's iterative reduced step (oracle/pxo_solve.c: pxo_ba_solve_iterative, pxo_ba_reduced_system) -- the reference the
GPU's inexact trajectories are compared with in tests/test_ba_pcg_precond_gpu.py -- and the condition of every scene used there.

The step is written from the specification (include/pixsfm_hip.h: pxr_lm_options; the header comment of csrc/pxr_ba_pcg.hip) on the
oracle's dense scaled normal equations; its model cost change is the direct branch's -d.g - d.H.d / 2 with the full step.  It is
pinned here by
  * tight options (eta = 0, r_tolerance = 1e-13) against the oracle's own dense Cholesky step (tolerances: tests/test_ba_pcg_gpu.py:44-47);
  * the first conjugate-gradient iterate on a scene with block-diagonal S against numpy's solve of the dense S;
  * the preconditioner blocks and S itself against a Schur complement formed in numpy from pxo.ba_eval_batch's Jacobians: equal to
    the block diagonal of S with one camera per image, different from it by exactly the dropped cross terms with a shared camera;
  * the default eta = 0.1 reaching the direct solve's optimum (the bar of tests/test_ba_pcg_gpu.py:62).
The last two tests are the CONDITION of the scenes as references: the measured tables are in tests/test_ba_pcg_precond_gpu.py."""
import numpy as np
import pytest

import geom_cases
import pcg_cases as pc
from test_ba_solve_gpu import _gauge

EPS = np.finfo(np.float64).eps


def _cfg_loss():
    import pxo
    return pxo.cfg(l2_normalize=False), pxo.loss(*pc.CAUCHY)


def _six(shared_camera):
    prob = geom_cases.make_case(n_cams=6, n_points=60, obs_per_point=4, shared_camera=shared_camera)
    return prob, _gauge(prob)


# ---- 1. tight conjugate gradients take the dense Cholesky step -------------------------------------------------------------------------
@pytest.mark.parametrize("shared_camera", [False, True])
def test_tight_options_reproduce_the_direct_solve(shared_camera):
    prob, gauge = _six(shared_camera)
    for iters in (1, 4, 7):
        sd, pd = geom_cases.oracle_solve(prob, pc.CAUCHY, gauge, max_iterations=iters)
        si, tr, pi = pc.oracle_iterative(prob, gauge, iters, cap=2000, eta=0.0, r_tolerance=1e-13)
        print("shared %d, %d iterations: cost %.2e of the initial, parameters %.2e, cg %s" % (
            shared_camera, iters, abs(si["final_cost"] - sd["final_cost"]) / sd["initial_cost"], pc.relative_gap(pi, pd),
            [e["cg_iterations"] for e in tr]))
        assert si["iterations"] == sd["iterations"] and si["num_successful"] == sd["num_successful"]
        assert si["termination"] == sd["termination"] and si["initial_cost"] == sd["initial_cost"]
        assert [e["step_is_successful"] for e in tr].count(1) == sd["num_successful"] and len(tr) == sd["iterations"]
        assert abs(si["final_cost"] - sd["final_cost"]) < 1e-8 * sd["initial_cost"]
        for a, b in zip(pi, pd):
            assert np.abs(a - b).max() < 1e-7 * max(1.0, np.abs(b).max())
        assert si["final_radius"] == pytest.approx(sd["final_radius"], rel=1e-6) and tr[-1]["radius"] == si["final_radius"]
        assert all(e["cg_iterations"] > 0 and e["step_is_valid"] for e in tr)


# ---- 2. block-diagonal S: the first iterate is the solution -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pc.DECOUPLED))
def test_first_cg_iterate_solves_a_block_diagonal_system(name):
    import pxo
    prob, gauge = pc.decoupled(name, ramp=True)
    rs = pxo.ba_reduced_system(prob, *_cfg_loss(), *gauge, pxo.lm_options(), pxo.linear_options(1, 0.1))
    S, b, x, grp = rs["S"], rs["rhs"], rs["x"], rs["col_group"]
    assert rs["n_c"] == sum(pc.DECOUPLED[name]["rows"]) and rs["cg_iterations"] == 1
    # the premise: S is block diagonal over exactly the preconditioner's blocks, one per variable image, of the expected rows
    assert np.array_equal(S != 0.0, grp[:, None] == grp[None, :])
    assert sorted(np.bincount(grp).tolist()) == sorted(r for r in pc.DECOUPLED[name]["rows"] if r)
    assert np.array_equal(rs["M"] != 0.0, S != 0.0) and np.abs(rs["M"] - S).max() <= 4 * EPS * np.abs(S).max()
    want = np.linalg.solve(S, b)
    res = np.linalg.norm(S @ x - b) / np.linalg.norm(b)
    print("%s: n_c %d, |S x - b| / |b| %.2e (numpy's own %.2e), cond(S) %.1e" % (
        name, rs["n_c"], res, np.linalg.norm(S @ want - b) / np.linalg.norm(b), np.linalg.cond(S)))
    assert res <= 1e-12
    # ... so a solve ends in at most two iterations (the second on the Q test or on rho == 0), and one is enough for the direct step
    for iters in (1, 4):
        s, tr, p = pc.oracle_iterative(prob, gauge, iters)
        assert len(tr) == iters and all(1 <= e["cg_iterations"] <= 2 for e in tr)
        s1, tr1, p1 = pc.oracle_iterative(prob, gauge, iters, cap=1)
        sd, pd = geom_cases.oracle_solve(prob, pc.CAUCHY, gauge, max_iterations=iters)
        assert [e["cg_iterations"] for e in tr1] == [1] * iters and all(e["cg_stop"] == "max_iterations" for e in tr1)
        assert s1["iterations"] == sd["iterations"] and s1["num_successful"] == sd["num_successful"]
        assert abs(s1["final_cost"] - sd["final_cost"]) < 1e-8 * sd["initial_cost"]
        assert pc.relative_gap(p1, pd) < 1e-7


# ---- 3. the preconditioner against a Schur complement formed in numpy ---------------------------------------------------------------------
def _quat_plus_jacobian(q):
    """d(exp(delta) * q) / d delta at delta = 0 (4 x 3), q = (w, x, y, z) [upstream Ceres QuaternionManifold::PlusJacobian]"""
    w, x, y, z = q
    return np.array([[-x, -y, -z], [w, z, -y], [-z, w, x], [y, -x, w]])


def _numpy_reduced_system(prob, gauge, radius=1e4):
    """S, the per-observation blocks W_i (in S's columns) and T_p of the first LM iteration, from pxo.ba_eval_batch's raw residuals
    and ambient Jacobians: tangent columns, the loss's corrector, Jacobi scaling 1 / (1 + |column|), damping clamp(diag, 1e-6, 1e32)
    / radius, Schur complement -- all dense."""
    import pxo
    pose_const, tmask, cmask, ptc = gauge
    cfg, ls = _cfg_loss()
    _, r, J = pxo.ba_eval_batch(prob, cfg, ls, want_r=True, want_J=True)
    n_img, n_cam, n_pt = len(prob["image_camera"]), len(prob["cam_model"]), len(prob["xyz"])
    cols, off = {}, 0
    for i in range(n_img):                                           # pose columns: 3 rotation + the free translation components
        if not pose_const[i]:
            free_t = [a for a in range(3) if not (int(tmask[i]) >> a) & 1]
            cols["img", i] = (off, free_t); off += 3 + len(free_t)
    for c in range(n_cam):
        K = pxo.lib().pxo_camera_num_params(int(prob["cam_model"][c]))
        free_k = [a for a in range(K) if not (int(cmask[c]) >> a) & 1]
        if free_k:
            cols["cam", c] = (off, free_k); off += len(free_k)
    n_c = off
    for p in range(n_pt):
        if not ptc[p]:
            cols["pt", p] = (off, None); off += 3
    n, C = off, r.shape[1]
    Jd = np.zeros((len(r) * C, n)); rd = np.zeros(len(r) * C)
    for i, (im, pt) in enumerate(zip(prob["obs_image"], prob["obs_point"])):
        im, pt = int(im), int(pt)
        cam = int(prob["image_camera"][im])
        idx, blocks = [], []
        if ("img", im) in cols:
            o, free_t = cols["img", im]
            blocks += [J[i][:, 0:4] @ _quat_plus_jacobian(prob["qvec"][im] / np.linalg.norm(prob["qvec"][im])), J[i][:, 4:7][:, free_t]]
            idx += list(range(o, o + 3 + len(free_t)))
        if ("cam", cam) in cols:
            o, free_k = cols["cam", cam]
            blocks.append(J[i][:, 10:][:, free_k]); idx += list(range(o, o + len(free_k)))
        if ("pt", pt) in cols:
            o = cols["pt", pt][0]
            blocks.append(J[i][:, 7:10]); idx += [o, o + 1, o + 2]
        Jl = np.hstack(blocks)
        sq = float(r[i] @ r[i])
        rc, Jc = pxo.corrector(sq, pxo.loss_eval(ls, sq), r[i], Jl)
        Jd[i * C:(i + 1) * C, idx] = Jc; rd[i * C:(i + 1) * C] = rc
    scale = 1.0 / (1.0 + np.sqrt((Jd * Jd).sum(0)))
    Js = Jd * scale
    H = Js.T @ Js
    A = H + np.diag(np.clip(np.diag(H), 1e-6, 1e32) / radius)
    S = A[:n_c, :n_c].copy()
    T, W, kappa = {}, [], 1.0
    for p in range(n_pt):
        if ("pt", p) in cols:
            o = cols["pt", p][0]
            T[p] = np.linalg.inv(A[o:o + 3, o:o + 3]); kappa = max(kappa, np.linalg.cond(A[o:o + 3, o:o + 3]))
            S -= A[:n_c, o:o + 3] @ T[p] @ A[o:o + 3, :n_c]
    for i, pt in enumerate(prob["obs_point"]):                       # W_i = (camera-side columns of the observation)^T (its point columns)
        Ji = Js[i * C:(i + 1) * C]
        W.append(Ji[:, :n_c].T @ Ji[:, cols["pt", int(pt)][0]:cols["pt", int(pt)][0] + 3] if ("pt", int(pt)) in cols else None)
    return S, W, T, cols, n_c, kappa


def _tolerance(S, kappa):
    """Both sides form entries of magnitude <= max|S| ~ 1 (scaled columns have norm < 1) from sums of a few hundred products and the
    inverse of the damped 3 x 3 point blocks, whose rounding is amplified by their condition number: 256 eps kappa max|S|."""
    return 256 * EPS * kappa * np.abs(S).max()


def test_one_camera_per_image_the_preconditioner_is_the_block_diagonal_of_S():
    import pxo
    prob, gauge = _six(False)
    rs = pxo.ba_reduced_system(prob, *_cfg_loss(), *gauge, pxo.lm_options(), pxo.linear_options())
    S, W, T, cols, n_c, kappa = _numpy_reduced_system(prob, gauge)
    tol = _tolerance(S, kappa)
    grp = rs["col_group"]
    same = grp[:, None] == grp[None, :]
    print("n_c %d, kappa(point blocks) %.1e, tolerance %.1e: S %.2e, blocks %.2e" % (
        n_c, kappa, tol, np.abs(rs["S"] - S).max(), np.abs(rs["M"] - np.where(same, S, 0.0)).max()))
    assert rs["n_c"] == n_c == 6 * 5 - 1 + 2 * 6
    assert np.abs(rs["S"] - S).max() < tol                                    # the oracle's dense S itself
    # joint blocks: pose + intrinsics of an image together (image 0: its two intrinsics alone)
    assert sorted(np.bincount(grp).tolist()) == [2, 7, 8, 8, 8, 8]
    for im in range(6):
        if ("img", im) in cols:
            assert grp[cols["img", im][0]] == grp[cols["cam", im][0]]
    assert np.abs(rs["M"] - np.where(same, S, 0.0)).max() < tol
    assert np.abs(np.where(same, 0.0, S)).max() > 1e3 * tol                   # (S is NOT block diagonal here: the comparison says something)


def test_shared_camera_the_preconditioner_drops_exactly_the_cross_terms():
    import pxo
    prob, gauge = _six(True)
    rs = pxo.ba_reduced_system(prob, *_cfg_loss(), *gauge, pxo.lm_options(), pxo.linear_options())
    S, W, T, cols, n_c, kappa = _numpy_reduced_system(prob, gauge)
    tol = _tolerance(S, kappa)
    grp = rs["col_group"]
    same = grp[:, None] == grp[None, :]
    assert rs["n_c"] == n_c == 6 * 5 - 1 + 2 and np.abs(rs["S"] - S).max() < tol
    assert sorted(np.bincount(grp).tolist()) == [2, 5, 6, 6, 6, 6]           # pose blocks and ONE intrinsics block
    # sum over points of sum_{i != j} W_i T_p W_j^T, restricted to the blocks
    cross = np.zeros((n_c, n_c))
    by_point = {}
    for i, pt in enumerate(prob["obs_point"]):
        by_point.setdefault(int(pt), []).append(i)
    for pt, obs in by_point.items():
        for i in obs:
            for j in obs:
                if i != j:
                    cross += W[i] @ T[pt] @ W[j].T
    cross = np.where(same, cross, 0.0)
    diff = rs["M"] - np.where(same, S, 0.0)
    k0, kn = cols["cam", 0][0], cols["cam", 0][0] + 2
    print("tolerance %.1e: |difference - cross terms| %.2e, |cross terms| %.2e" % (tol, np.abs(diff - cross).max(), np.abs(cross).max()))
    assert np.abs(diff - cross).max() < tol
    assert np.abs(diff[k0:kn, k0:kn]).max() > 1e3 * tol                        # nonzero, and only in the intrinsics block
    outside = diff.copy(); outside[k0:kn, k0:kn] = 0.0
    assert np.abs(outside).max() < tol
    assert np.abs(diff - diff.T).max() < tol                                   # symmetric
    for g in range(grp.max() + 1):                                             # every specified block is still positive definite
        c = np.flatnonzero(grp == g)
        assert np.linalg.eigvalsh(rs["M"][np.ix_(c, c)]).min() > 0.0


# ---- 4. the default configuration reaches the direct solve's optimum --------------------------------------------------------------------
@pytest.mark.parametrize("shared_camera", [False, True])
def test_default_eta_reaches_the_direct_optimum(shared_camera):
    prob, gauge = _six(shared_camera)
    sd, pd = geom_cases.oracle_solve(prob, pc.CAUCHY, gauge, max_iterations=30)
    si, tr, pi = pc.oracle_iterative(prob, gauge, 30)
    print("shared %d: direct %.9e iterative %.9e (%.1e), cg %d over %d iterations" % (
        shared_camera, sd["final_cost"], si["final_cost"], abs(si["final_cost"] - sd["final_cost"]) / sd["final_cost"],
        si["linear_iterations"], si["iterations"]))
    assert abs(si["final_cost"] - sd["final_cost"]) < 1e-3 * sd["final_cost"] + 1e-9 * sd["initial_cost"]
    assert 0 < si["linear_iterations"] <= 200 * si["iterations"]
    assert any(e["cg_stop"] == "q" for e in tr)


# ---- 5. the condition of the scenes the GPU file uses ------------------------------------------------------------------------------------
PERTURBATION_SEEDS = (99, 100, 101)


@pytest.mark.parametrize("name", sorted(pc.DECOUPLED))
def test_decoupled_scenes_are_stable_references(name):
    """The oracle's direct solve twice, the second time with the parameters moved by 1e-13 relative: the same decisions, and a tenth
    of the tolerances the GPU test applies (1e-8 of the initial cost, 1e-7 in the parameters)."""
    prob, gauge = pc.decoupled(name, ramp=True)
    for iters in (1, 4):
        s0, p0 = geom_cases.oracle_solve(prob, pc.CAUCHY, gauge, max_iterations=iters)
        for seed in PERTURBATION_SEEDS:
            s1, p1 = geom_cases.oracle_solve(pc.perturbed(prob, seed=seed), pc.CAUCHY, gauge, max_iterations=iters)
            dc, dp = abs(s1["final_cost"] - s0["final_cost"]) / s0["initial_cost"], pc.relative_gap(p1, p0)
            print("%s, %d iterations (%d successful), perturbation %d: cost %.1e of the initial, parameters %.1e" % (
                name, iters, s0["num_successful"], seed, dc, dp))
            assert (s1["iterations"], s1["num_successful"], s1["termination"]) == (s0["iterations"], s0["num_successful"], s0["termination"])
            assert dc < 1e-9 and dp < 1e-8


@pytest.mark.parametrize("cap", pc.LINEAR_CAPS)
@pytest.mark.parametrize("name", sorted(pc.INEXACT))
def test_inexact_scenes_are_stable_references(name, cap):
    """The oracle's inexact solve twice (unperturbed, parameters moved by 1e-13 relative): identical conjugate-gradient counts, stops
    and decisions per iteration, every stopping margin above 1e-6, relative_decrease and radius within a tenth of the per-iteration
    tolerance of the GPU test, end points within a tenth of test_ba_solve_gpu._assert_same's (1e-6)."""
    prob, gauge = pc.inexact(name)
    s0, t0, p0 = pc.inexact_oracle(name, cap)
    margins = [m for e in t0 for m in (e["margin_last"], e["margin_prev"], e["margin_min"]) if m >= 0.0]
    assert len(t0) == s0["iterations"] == pc.INEXACT_ITERATIONS and all(e["step_is_valid"] for e in t0)
    worst = 0.0
    for seed in PERTURBATION_SEEDS:
        s1, t1, p1 = pc.oracle_iterative(pc.perturbed(prob, seed=seed), gauge, pc.INEXACT_ITERATIONS, cap)
        assert pc.decisions(t1) == pc.decisions(t0)
        assert (s1["iterations"], s1["num_successful"], s1["termination"]) == (s0["iterations"], s0["num_successful"], s0["termination"])
        drel = max(abs(a["relative_decrease"] - b["relative_decrease"]) / abs(b["relative_decrease"]) for a, b in zip(t1, t0))
        drad = max(abs(a["radius"] - b["radius"]) / b["radius"] for a, b in zip(t1, t0))
        dc, dp = abs(s1["final_cost"] - s0["final_cost"]) / s0["final_cost"], pc.relative_gap(p1, p0)
        worst = max(worst, drel, drad)
        print("%s, cap %d, perturbation %d: relative_decrease %.1e radius %.1e final cost %.1e parameters %.1e" % (name, cap, seed, drel, drad, dc, dp))
        assert dc < 1e-7 and dp < 1e-7
    print("%s, cap %d: %d/%d successful, cg %s (%d), stops %s, smallest margin %.2e, worst per-iteration difference %.1e" % (
        name, cap, s0["num_successful"], s0["iterations"], [e["cg_iterations"] for e in t0], s0["linear_iterations"],
        "".join(e["cg_stop"][0] for e in t0), min(margins), worst))
    assert min(margins) > 1e-6
    assert worst <= pc.PER_ITERATION_RTOL / 10
    if cap == 3:
        assert any(e["cg_stop"] == "max_iterations" for e in t0) and all(e["cg_iterations"] <= 3 for e in t0)
    else:
        assert all(e["cg_stop"] == "q" for e in t0)
