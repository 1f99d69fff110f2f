"""GPU: the preconditioner, the stopping rule and the inexact steps of the iterative Schur solver (csrc/pxr_ba_pcg.hip, the iterative
branch of csrc/pxr_ba_solve.hip) -- what conjugate gradients driven to 1e-13 (tests/test_ba_pcg_gpu.py and the tests that follow
it) cannot see: with ANY symmetric positive definite preconditioner they reach the same x, the Q test never fires at eta = 0, and
x.(b - S x) is zero.  Geometric solver throughout (no patches); every case runs in the deterministic context (k_pre_assemble_det,
k_mloc_finish, k_col_finish) and with floating-point atomics (k_pre_assemble, k_ublk_matvec).

A. ONE conjugate-gradient iteration is exact where S is block diagonal.  Scenes (tests/pcg_cases.py: DECOUPLED) in which no point
is seen by two variable images -- images 0-2 fully constant, point p seen by them and by image 3 + p % nv, one camera per image, 30
points per variable image: S is block diagonal over exactly the preconditioner's blocks, M = blockdiag(S) + D_c / radius IS S and
the first iterate is S^-1 b.  The iterative solver limited to one linear iteration must take the direct solver's LM steps
(tolerances: tests/test_ba_pcg_gpu.py:44-47, none new); an error in assembling, damping, inverting or applying a block shows at
O(1).  With the default 200 iterations a solve ends in at most two (the second on the Q test or on rho == 0).

  case      block rows per variable image   DC  G   what it reaches
  pinhole8  8 x 5                            8   8  PINHOLE, principal point constant
  opencv12  12 x 5                          12  16  FULL_OPENCV, fx fy k1 k2 p1 p2 free
  opencv18  18 x 5                          18  32  FULL_OPENCV, everything free: PCG_GS rows
  mixed     18, 8, 16, 8, 12, 8             18  32  PINHOLE / FULL_OPENCV alternating, a pose part of 4 rows (tvec mask 0b101),
                                                    a pose-constant image whose block is its 12 intrinsics alone

Condition of the reference (CPU: tests/test_oracle_pcg.py::test_decoupled_scenes_are_stable_references -- the oracle's direct solve
twice, the second time with poses, intrinsics and points moved by 1e-13 relative, three perturbations; accepted at the same
decisions and a tenth of the tolerances: 1e-9 of the initial cost, 1e-8 in the parameters).  Largest over the perturbations:

  case      1 iteration: cost / parameters   4 iterations (all successful): cost / parameters
  pinhole8  2.7e-12 / 1.2e-12                2.3e-12 / 1.8e-12
  opencv12  1.6e-12 / 3.1e-12                1.3e-12 / 3.0e-12
  opencv18  1.4e-12 / 3.1e-11                1.1e-12 / 3.0e-11
  mixed     2.7e-12 / 7.9e-11                2.8e-12 / 5.0e-11
(the oracle's own one-iteration solve takes its direct solve's steps at the same tolerances, and |S x_1 - b| / |b| of its first
 iterate is 2.2e-14 at most with cond(S) up to 2.1e10: tests/test_oracle_pcg.py::test_first_cg_iterate_solves_a_block_diagonal_system)

C. The configuration users run (eta = 0.1, 200 linear iterations) and a cap of 3 against the oracle's iterative step
(oracle/pxo_solve.c: pxo_ba_solve_iterative -- written from the specification; its model cost change is -d.g - d.H.d / 2 with the
full step, so the comparison is independent of the GPU's x.(b - S x) correction), 7 LM iterations on ramp-form scenes
(tests/pcg_cases.py: INEXACT): iterations, successful steps, termination and the TOTAL number of conjugate-gradient iterations
equal, end points within test_ba_solve_gpu._assert_same, and per iteration (Context.set_iteration_callbacks) step_is_valid /
step_is_successful equal, relative_decrease and trust_region_radius within PER_ITERATION_RTOL = 1e-7: ten times the largest
difference between the oracle's unperturbed and 1e-13-perturbed runs (7.0e-9, scene g), rounded up to a power of ten; the ceiling is
1e-6 and a scene whose oracle alone needs more than 1e-8 would be replaced.

Condition of the scenes (CPU: tests/test_oracle_pcg.py::test_inexact_scenes_are_stable_references; three perturbations; identical
conjugate-gradient counts, stops and decisions in every run; margin = |zeta - eta| / eta of the Q test, the smallest over ALL
conjugate-gradient iterations of the solve, which includes the iteration that stopped and the one before it):

  scene       cap  successful  cg per LM iteration (total)      stops    smallest margin  relative_decrease  radius   cost     parameters
  six         200  7 / 7       2 4 5 6 6 4 6        (33)        qqqqqqq  5.8e-2           1.1e-10            0        1.3e-14  6.7e-13
  six           3  7 / 7       2 3 3 3 3 3 3        (20)        qmmmmmm  3.5e-1           2.0e-10            0        1.8e-14  6.7e-13
  six_shared  200  7 / 7       2 4 5 5 14 6 14      (50)        qqqqqqq  7.1e-2           2.1e-10            0        2.8e-14  4.0e-13
  six_shared    3  7 / 7       2 3 3 3 3 3 3        (20)        qmmmmmm  4.0e-1           2.0e-10            0        2.1e-14  4.0e-13
  g           200  6 / 7       3 4 3 3 3 3 3        (22)        qqqqqqq  4.5e-2           7.0e-9             1.6e-9   1.1e-12  6.4e-11
  g             3  6 / 7       3 3 3 3 3 3 3        (21)        qmqqqqq  1.7e-2           4.6e-9             1.7e-9   3.0e-12  1.0e-10
  i           200  7 / 7       3 6 6 15 16 16 8     (70)        qqqqqqq  4.3e-3           1.9e-9             0        3.4e-13  2.1e-8
  i             3  7 / 7       3 3 3 3 3 3 3        (21)        qmmmmmm  4.3e-3           2.2e-10            0        2.1e-13  5.7e-9
(q: the Q test, m: the cap.  six / six_shared: geom_cases.make_case(n_cams=6, n_points=60, obs_per_point=4), seed 0, one camera per
image / one shared camera; g, i: the scenes of those ids of tests/test_ba_wide_blocks_gpu.py, seeds 3 and 1.  These were the first
seeds tried: every one met the conditions, none was replaced.  Scene g rejects its sixth step.)

Measured on the GPU (MI355X, both contexts).  A: one iteration against the direct solver, cost at most 5.1e-13 of the initial cost,
parameters at most 3.9e-11 (1e-8 and 1e-7 are asked); the default configuration takes exactly 2 iterations per solve.  C: every
conjugate-gradient total equal to the oracle's; relative_decrease at most 3.0e-8 (scene i, 200 iterations, floating-point atomics)
and radius at most 2.5e-10 from the oracle's where 1e-7 is asked; final cost at most 1.1e-12 relative, intrinsics at most 6.9e-4
absolute on focal lengths of 1.2e3 (about 5.5e-7 relative where 1e-6 is asked: scene i), everything else below 2e-10.
What the file is for: with the damping term of k_pre_invert dropped, all 16 cases of A fail (final cost 4e-6 .. 8e-4 of the initial
cost away, or another number of successful steps) while the tight conjugate gradients of tests/test_ba_pcg_gpu.py,
tests/test_geom_ba_gpu.py and scenes a-d of tests/test_ba_wide_blocks_gpu.py still pass (its FULL_OPENCV scenes notice, because
the undamped blocks are singular there); with the damping halved all 16 fail again (4e-7 .. 7e-4) and 47 of those 49 earlier cases
pass."""
import numpy as np
import pytest

import pcg_cases as pc
from test_ba_solve_gpu import _assert_same
from test_ba_wide_blocks_gpu import any_ctx, atomics_ctx, det_ctx, expected_layout  # noqa: F401 -- the fixtures of that file
from test_geom_ba_gpu import _report
from test_geom_ba_gpu import _solve as _solve_geom

pytestmark = pytest.mark.gpu


def _close(pa, pb, tol):                                                   # tests/test_ba_pcg_gpu.py:25
    for a_, b_ in zip(pa, pb):
        assert np.abs(a_ - b_).max() < tol * max(1.0, np.abs(b_).max()), np.abs(a_ - b_).max()


# ---- A. one conjugate-gradient iteration on a block-diagonal S ------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [1, 4])
@pytest.mark.parametrize("name", sorted(pc.DECOUPLED))
def test_one_cg_iteration_takes_the_direct_step_where_S_is_block_diagonal(any_ctx, name, iters):
    spec = pc.DECOUPLED[name]
    prob, gauge = pc.decoupled(name)
    DC, n_c, rows = expected_layout(prob, gauge)                           # a case must not silently land at another width
    assert (DC, rows, n_c) == (spec["DC"], spec["rows"], sum(spec["rows"])) and pc.lane_group(DC) == spec["G"]
    sd, pd = _solve_geom(any_ctx, prob, gauge, max_iterations=iters, linear_solver="direct")
    s1, p1 = _solve_geom(any_ctx, prob, gauge, max_iterations=iters, linear_solver="iterative", max_linear_solver_iterations=1, eta=0.1)
    s2, p2 = _solve_geom(any_ctx, prob, gauge, max_iterations=iters, linear_solver="iterative", max_linear_solver_iterations=200, eta=0.1)
    print("%s (DC %d, n_c %d), %d iterations: direct %d/%d %.12e | one cg iteration %d/%d %.12e, cg %d, cost %.2e of the initial, parameters %.2e"
          " | default cg %d, %d/%d, parameters %.2e" % (
              name, DC, n_c, iters, sd["num_successful"], sd["iterations"], sd["final_cost"], s1["num_successful"], s1["iterations"],
              s1["final_cost"], s1["linear_iterations"], abs(s1["final_cost"] - sd["final_cost"]) / sd["initial_cost"], pc.relative_gap(p1, pd),
              s2["linear_iterations"], s2["num_successful"], s2["iterations"], pc.relative_gap(p2, pd)))
    assert sd["linear_solver"] == 1 and s1["linear_solver"] == 2 and s2["linear_solver"] == 2
    assert sd["num_camera_unknowns"] == s1["num_camera_unknowns"] == n_c
    assert s1["iterations"] == sd["iterations"] and s1["num_successful"] == sd["num_successful"]
    assert abs(s1["final_cost"] - sd["final_cost"]) < 1e-8 * sd["initial_cost"]
    _close(p1, pd, 1e-7)
    assert s1["linear_iterations"] == s1["iterations"]
    assert sd["final_cost"] < sd["initial_cost"] and sd["num_successful"] > 0
    # the default configuration: the second iteration ends on the Q test or on rho == 0
    assert s2["iterations"] == iters and 0 < s2["linear_iterations"] <= 2 * s2["iterations"]


# ---- C. inexact steps against the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", pc.LINEAR_CAPS)
@pytest.mark.parametrize("name", sorted(pc.INEXACT))
def test_inexact_trajectory_matches_the_oracle(any_ctx, name, cap):
    prob, gauge = pc.inexact(name)
    so, trace, po = pc.inexact_oracle(name, cap)
    log = []
    any_ctx.set_iteration_callbacks([log.append])
    try:
        s, pg = _solve_geom(any_ctx, prob, gauge, max_iterations=pc.INEXACT_ITERATIONS, linear_solver="iterative", eta=0.1,
                            max_linear_solver_iterations=cap)
    finally:
        any_ctx.set_iteration_callbacks([])
    _report("scene %s, cap %d" % (name, cap), s, so, pg, po)
    print("  cg: gpu %d oracle %d %s (%s)" % (s["linear_iterations"], so["linear_iterations"], [e["cg_iterations"] for e in trace],
                                             "".join(e["cg_stop"][0] for e in trace)))
    its = [c for c in log if c.iteration > 0]
    for c, e in zip(its, trace):
        print("  it %d: valid %d/%d successful %d/%d relative_decrease %.12e vs %.12e (%.1e) radius %.6e vs %.6e (%.1e)" % (
            c.iteration, c.step_is_valid, e["step_is_valid"], c.step_is_successful, e["step_is_successful"], c.relative_decrease,
            e["relative_decrease"], abs(c.relative_decrease - e["relative_decrease"]) / abs(e["relative_decrease"]),
            c.trust_region_radius, e["radius"], abs(c.trust_region_radius - e["radius"]) / e["radius"]))
    assert s["linear_solver"] == 2 and log[0].iteration == 0
    assert s["linear_iterations"] == so["linear_iterations"]
    _assert_same(s, pg, so, po, ptol=1e-6, trajectory=True)
    assert [c.iteration for c in its] == list(range(1, len(trace) + 1))
    for c, e in zip(its, trace):
        assert (c.step_is_valid, c.step_is_successful) == (e["step_is_valid"], e["step_is_successful"]), c.iteration
        assert abs(c.relative_decrease - e["relative_decrease"]) <= pc.PER_ITERATION_RTOL * abs(e["relative_decrease"]), c.iteration
        assert abs(c.trust_region_radius - e["radius"]) <= pc.PER_ITERATION_RTOL * e["radius"], c.iteration
    assert s["final_cost"] < s["initial_cost"]
