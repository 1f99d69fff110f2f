"""GPU: camera blocks wider than 8 columns in every path of the BA solver.

DC -- the largest number of camera-side columns of one observation (csrc/pxr_ba_structure.h: block_layout) -- selects the lane-group
width G of k_schur_lds / k_backsub (csrc/pxr_ba_solve.hip) and of k_pt_u / k_img_wu / k_img_block (csrc/pxr_ba_pcg.hip), the
staging loop of k_img (prefetching while LS = 11 + 2 DC <= 32), the rows of the preconditioner blocks k_pre_invert inverts (up to
PCG_GS = 18), the strides of the deterministic tables and the dynamic LDS of k_jac, k_schur_lds and k_img_block.  The rest of the
suite runs the iterative solver at DC <= 8 only, G = 16 in the direct solver only and G = 32 nowhere.  The scenes here:

  id  scene                                                  DC  G   what it reaches
  a   PINHOLE, principal point constant (control)             8   8  upper edge of <8>
  b   FULL_OPENCV, nine parameters constant                   9  16  lower edge of <16>
  c   FULL_OPENCV, eight parameters constant                 10  16  k_img: last width of the prefetching loop (LS = 31)
  d   FULL_OPENCV, seven parameters constant                 11  16  k_img: first width of the plain loop (LS = 33)
  e   FULL_OPENCV, cmask = 0b1100                            16  16  upper edge of <16>
  f   FULL_OPENCV, cmask = 1 << 11                           17  32  lower edge of <32>
  g   FULL_OPENCV, cmask = 0                                 18  32  the joint preconditioner block of 18 rows (PCG_GS), NE = 189
  h   THIN_PRISM_FISHEYE, cmask = 0                          18  32  the forward-mode dual Jacobians at full width
  i   g with one camera shared by all images                 18  32  pose blocks of 6 or 5 rows, one intrinsics block of 12 with an
                                                                     entry from every image
  j   g with 12 cameras, 60 points, tracks of 10             18  32  second partner batch of k_schur_lds; k_pt_u over 10 observations
  k   8 cameras, PINHOLE (0b1100) and FULL_OPENCV (0) mixed  18  32  blocks of 12 / 17 / 2 / 16 / 8 / 18 rows: lanes beyond an image's
                                                                     own block idle, images whose own block differs from DC
  l   g with 52 cameras, 400 points                          18  32  n_c = 929: two column tiles of k_schur_lds

(a to i: 6 cameras, 90 points, tracks of 4.  Default gauge: image 0 pose-constant, tvec_mask[1] = 1.  k: image 0 is FULL_OPENCV too
-- the pose-constant image then has a block of the 12 intrinsics alone -- and the models alternate from image 1 on; image 2
pose-constant, tvec_mask[3] = 0b101, every seventh point constant.)

References: the oracle's restated Ceres loop on the ramp form of the scene (tests/geom_cases.py) for the direct solver, the direct
solver for the iterative one (tests/test_ba_pcg_gpu.py).  Tolerances: the ones of the tests this file imports from, none new.

Stability of the reference (CPU, no GPU needed: the oracle run twice per scene, the second time with poses, points and keypoints
perturbed by 1e-13 relative; a scene is accepted only if both runs take the same accept / reject decisions and stay within a
tenth of the tolerance the test applies -- 1e-7 where _assert_same asks 1e-6).  Measured, 7 iterations (l: 3):

  id  n_c  iterations / successful  same decisions  final cost (relative)  parameters (relative)  oracle time
  a    41  7 / 6                    yes             1.9e-12                1.1e-11                0.03 s
  b    47  7 / 6                    yes             1.5e-12                6.7e-12                0.04 s
  c    53  7 / 6                    yes             1.2e-12                7.1e-12                0.04 s
  d    59  7 / 4                    yes             3.6e-12                3.9e-12                0.04 s
  e    89  7 / 7                    yes             2.0e-11                3.9e-10                0.06 s
  f    95  7 / 5                    yes             2.8e-12                2.4e-11                0.05 s
  g   101  7 / 5                    yes             8.8e-12                4.7e-10                0.05 s
  g with inner iterations: 7 / 5    yes             1.3e-11                1.8e-9 (the test asks 1e-4)
  h   101  7 / 5                    yes             4.8e-12                7.3e-11                0.06 s
  i    41  7 / 5                    yes             1.6e-12                3.3e-10                0.04 s
  j   209  7 / 7                    yes             3.5e-12                6.8e-11                0.10 s
  k    99  7 / 6                    yes             5.6e-12                1.7e-10                0.06 s
  l   929  3 / 3                    yes             4.5e-13                7.8e-11                4.8 s
(largest initial reprojection error 2.7 px: far inside the ramp's 13 px)

Featuremetric scenes (test_camera_models_ext._problem(6, seed=66), 5 iterations, tolerances 1e-6 / 1.2e-2 on the intrinsics):
  cmask 0 (DC 18):        5 / 5 both runs, final cost 1.2e-12, q 5.7e-14, X 1.4e-13, intrinsics 2.5e-8 absolute
  cmask 1 << 11 (DC 17):  5 / 5 both runs, final cost 8.7e-12, q 5.3e-14, X 1.8e-13, intrinsics 4.7e-8 absolute
  cmask 0, inner:         5 / 5 both runs, final cost 8.8e-12, q 4.6e-14, X 1.6e-13, intrinsics 2.8e-8 absolute
THIN_PRISM_FISHEYE with all twelve parameters free is ill-conditioned as a featuremetric scene (2e-7 in cost, 1.7e-4 in the
intrinsics under the same perturbation): it is scene h here, geometric, where it is stable.

What these scenes found (fixed in csrc/pxr_ba_solve.hip, "columns that stay small under Ceres' Jacobi scaling"): with the parent's
solver 20 of the 68 cases failed, all of them the DIRECT solver in the DETERMINISTIC context on scenes whose cameras refine the r^6
coefficients k3 and k6 together (e, g, h, j, k, l) -- intrinsics 3.6e-6 .. 9.0e-5 (relative to the largest) from the oracle where
1e-6 is asked, 1e-6 .. 1e-5 from the tight iterative solve where 1e-7 is asked -- while every width passed with floating-point
atomics: no lane group, stride or LDS size was wrong.  The fixed-point slots of U, g_c and S share ONE absolute grid made for the
largest diagonal entry, and Ceres' scaling 1 / (1 + sqrt d) leaves a column with d = |J_col|^2 << 1 (k3, k6: 1e-6 .. 1e-10) as small
as it was: 30 .. 40 significant bits where the others have 60, in exactly the columns the reduced system is ill-conditioned in.
The solver now carries a power of two per column (exact in floating point) that follows the linearisations; measured with it:
direct against the oracle, intrinsics of e 1e-9 (relative), all others below; tight conjugate gradients against the direct solver
at most 2.4e-8 in the parameters (scene l) and 1.6e-9 of the initial cost."""
import functools

import numpy as np
import pytest

import geom_cases
from test_ba_solve_gpu import _assert_same
from test_geom_ba_gpu import CAUCHY, _assert_inner_same, _report
from test_geom_ba_gpu import _solve as _solve_geom

pytestmark = pytest.mark.gpu

PINHOLE, FULL_OPENCV, THIN_PRISM_FISHEYE = 1, 6, 10
TIGHT = dict(linear_solver="iterative", eta=0.0, linear_r_tolerance=1e-13, max_linear_solver_iterations=2000)   # test_ba_pcg_gpu.py:40


def _all_but(*free):
    """cam_const_mask of a 12-parameter model with only the parameters `free` refined"""
    return 0xFFF & ~sum(1 << a for a in free)


# id: (make_model_case arguments, cam_const_mask per model, DC)        FULL_OPENCV: fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6
_SIX = dict(n_cams=6, n_points=90, obs_per_point=4)
SCENES = {
    "a": (dict(models=PINHOLE, seed=1, **_SIX), {PINHOLE: 0b1100}, 8),
    "b": (dict(models=FULL_OPENCV, seed=2, **_SIX), {FULL_OPENCV: _all_but(0, 1, 4)}, 9),
    "c": (dict(models=FULL_OPENCV, seed=3, **_SIX), {FULL_OPENCV: _all_but(0, 1, 4, 5)}, 10),
    "d": (dict(models=FULL_OPENCV, seed=4, **_SIX), {FULL_OPENCV: _all_but(0, 1, 4, 5, 6)}, 11),
    "e": (dict(models=FULL_OPENCV, seed=1, **_SIX), {FULL_OPENCV: 0b1100}, 16),
    "f": (dict(models=FULL_OPENCV, seed=2, **_SIX), {FULL_OPENCV: 1 << 11}, 17),
    "g": (dict(models=FULL_OPENCV, seed=3, **_SIX), {FULL_OPENCV: 0}, 18),
    "h": (dict(models=THIN_PRISM_FISHEYE, seed=4, **_SIX), {THIN_PRISM_FISHEYE: 0}, 18),
    "i": (dict(models=FULL_OPENCV, seed=1, shared_camera=True, **_SIX), {FULL_OPENCV: 0}, 18),
    "j": (dict(models=FULL_OPENCV, seed=2, n_cams=12, n_points=60, obs_per_point=10), {FULL_OPENCV: 0}, 18),
    "k": (dict(models=[FULL_OPENCV] + [FULL_OPENCV, PINHOLE] * 3 + [FULL_OPENCV], seed=3, n_cams=8, n_points=90, obs_per_point=4),
          {PINHOLE: 0b1100, FULL_OPENCV: 0}, 18),
    "l": (dict(models=FULL_OPENCV, seed=4, n_cams=52, n_points=400, obs_per_point=4), {FULL_OPENCV: 0}, 18),
}
WIDE = ("e", "f", "g", "h", "i", "j", "k", "l")
NUM_PARAMS = {PINHOLE: 4, FULL_OPENCV: 12, THIN_PRISM_FISHEYE: 12}


def gauge_of(name, prob):
    """default_problem_setup (image 0 pose-constant, one translation component of image 1 constant) with the scene's masks"""
    n_img, n_pt = len(prob["image_camera"]), len(prob["xyz"])
    pose_const = np.zeros(n_img, np.uint8); pose_const[0] = 1
    tmask = np.zeros(n_img, np.uint8); tmask[1] = 1
    cmask = np.array([SCENES[name][1][int(m)] for m in prob["cam_model"]], np.uint16)
    ptc = np.zeros(n_pt, np.uint8)
    if name == "k":
        pose_const[2] = 1
        tmask[3] = 0b101
        ptc[::7] = 1
    return pose_const, tmask, cmask, ptc


def expected_layout(prob, gauge):
    """(DC, n_c, block rows per image) by the rules of csrc/pxr_ba_structure.h"""
    pose_const, tmask, cmask, _ = gauge
    pose_dim = [0 if pose_const[i] else 6 - bin(int(tmask[i]) & 7).count("1") for i in range(len(pose_const))]
    intr_dim = [NUM_PARAMS[int(m)] - bin(int(cmask[c])).count("1") for c, m in enumerate(prob["cam_model"])]
    dci = [pose_dim[i] + intr_dim[prob["image_camera"][i]] for i in range(len(pose_dim))]
    return max(pose_dim) + max(intr_dim), sum(pose_dim) + sum(intr_dim), dci


@functools.lru_cache(maxsize=None)
def scene(name, ramp=True):
    prob = geom_cases.make_model_case(ramp=ramp, **SCENES[name][0])
    gauge = gauge_of(name, prob)
    assert expected_layout(prob, gauge)[0] == SCENES[name][2], name
    return prob, gauge


@functools.lru_cache(maxsize=None)
def oracle(name, max_iterations, inner=False):
    """the oracle's solve of a scene: computed once, shared by the tests that need it, left unchanged"""
    prob, gauge = scene(name)
    return geom_cases.oracle_solve(prob, CAUCHY, gauge, max_iterations=max_iterations, use_inner_iterations=inner)


def _iterations(name):
    return 3 if name == "l" else 7


@pytest.fixture(scope="module")
def det_ctx():
    """the default context: deterministic accumulation (fixed point in the direct solver, ordered partial sums in the iterative)"""
    from pixsfm_amd.engine import Context
    c = Context(0)
    assert c.deterministic
    yield c
    c.close()


@pytest.fixture(scope="module")
def atomics_ctx():
    """the opt-out: floating-point atomics"""
    from pixsfm_amd.engine import Context
    c = Context(0)
    c.deterministic = False
    assert not c.deterministic
    yield c
    c.close()


@pytest.fixture(params=["deterministic", "atomics"])
def any_ctx(request):
    return request.getfixturevalue("det_ctx" if request.param == "deterministic" else "atomics_ctx")


# ---- 1. the direct solver against the oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
def test_direct_solver_trajectory_matches_the_oracle(det_ctx, name):
    prob, gauge = scene(name)
    DC, n_c, dci = expected_layout(prob, gauge)
    if name == "k":
        assert dci == [12, 17, 2, 16, 8, 18, 8, 18]
    if name == "l":
        assert n_c * 18 > 128 * 1024 // 8 - 18              # the premise: k_schur_lds needs a second column tile
    it = _iterations(name)
    s, pg = _solve_geom(det_ctx, prob, gauge, max_iterations=it, linear_solver="direct")
    so, po = oracle(name, it)
    _report("scene %s (DC %d, n_c %d)" % (name, DC, n_c), s, so, pg, po)
    assert s["linear_solver"] == 1 and s["num_camera_unknowns"] == n_c
    _assert_same(s, pg, so, po, ptol=1e-6, trajectory=True)
    assert s["final_cost"] < s["initial_cost"]
    if name == "k":
        q, t, k, X = pg
        assert np.array_equal(X[::7], prob["xyz"][::7]) and np.array_equal(t[2], prob["tvec"][2])
        assert t[3][0] == prob["tvec"][3][0] and t[3][2] == prob["tvec"][3][2] and t[3][1] != prob["tvec"][3][1]
        assert np.array_equal(k[2, 2:4], prob["cam_params"][2, 2:4]) and k[2, 0] != prob["cam_params"][2, 0]


def test_a_wide_scene_rejects_a_step(det_ctx):
    """The trajectories above include a rejected step at full width (the radius shrinks, the same linearisation is solved again
    with more damping): g, i and j are the scenes on which the oracle rejects one."""
    rejected = []
    for name in ("g", "i", "j"):
        prob, gauge = scene(name)
        s, _ = _solve_geom(det_ctx, prob, gauge, max_iterations=_iterations(name), linear_solver="direct")
        so, _ = oracle(name, _iterations(name))
        assert s["iterations"] == so["iterations"] and s["num_successful"] == so["num_successful"]
        if s["num_successful"] < s["iterations"]:
            rejected.append(name)
    assert rejected


def test_inner_iterations_at_full_width(det_ctx):
    prob, gauge = scene("g")
    s, pg = _solve_geom(det_ctx, prob, gauge, max_iterations=7, use_inner_iterations=True, linear_solver="direct")
    so, po = oracle("g", 7, True)
    _report("scene g, inner iterations", s, so, pg, po)
    _assert_inner_same(s, pg, so, po, True)
    assert s["final_cost"] < s["initial_cost"]


# ---- 2. the iterative solver against the direct one ----------------------------------------------------------------------------------
def _assert_tight_cg_equals_direct(ctx, prob, gauge, iters, tag):
    sd, pd = _solve_geom(ctx, prob, gauge, max_iterations=iters, linear_solver="direct")
    si, pi = _solve_geom(ctx, prob, gauge, max_iterations=iters, **TIGHT)
    dp = max(np.abs(a - b).max() / max(1.0, np.abs(b).max()) for a, b in zip(pi, pd))
    print("%s, %d iterations: direct %.12e iterative %.12e (initial %.6e, %d/%d vs %d/%d), cg %d, parameters %.2e" % (
        tag, iters, sd["final_cost"], si["final_cost"], sd["initial_cost"], si["num_successful"], si["iterations"], sd["num_successful"],
        sd["iterations"], si["linear_iterations"], dp))
    assert sd["linear_solver"] == 1 and si["linear_solver"] == 2 and si["linear_iterations"] > 0
    assert si["iterations"] == sd["iterations"] and si["num_successful"] == sd["num_successful"]
    assert abs(si["final_cost"] - sd["final_cost"]) < 1e-8 * sd["initial_cost"]
    for a, b in zip(pi, pd):                                               # test_ba_pcg_gpu.py: _close(pi, pd, 1e-7)
        assert np.abs(a - b).max() < 1e-7 * max(1.0, np.abs(b).max()), np.abs(a - b).max()


@pytest.mark.parametrize("iters", [1, 4])
@pytest.mark.parametrize("name", [n for n in sorted(SCENES) if n != "l"])
def test_tight_cg_takes_the_direct_solvers_steps(any_ctx, name, iters):
    prob, gauge = scene(name)
    _assert_tight_cg_equals_direct(any_ctx, prob, gauge, iters, "scene %s" % name)


def test_tight_cg_on_two_column_tiles(det_ctx):
    prob, gauge = scene("l")
    _assert_tight_cg_equals_direct(det_ctx, prob, gauge, 3, "scene l")


# ---- 3. bit reproducibility at width 32 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["direct", "iterative"])
@pytest.mark.parametrize("shared_camera", [False, True])
def test_two_solves_at_full_width_are_bit_identical(det_ctx, atomics_ctx, shared_camera, solver):
    """FULL_OPENCV with everything free, 1400 observations per image: three 512-chunks for k_img (kpart[chunk][189]), two
    1024-chunks for the Schur and conjugate-gradient kernels (wpart[chunk][18], mpart[chunk][18][18])."""
    prob = geom_cases.make_model_case(FULL_OPENCV, n_cams=4, n_points=1400, obs_per_point=4, seed=5, shared_camera=shared_camera, ramp=False)
    assert np.bincount(prob["obs_image"]).tolist() == [1400] * 4
    n_img, n_cam = 4, len(prob["cam_model"])
    pose_const = np.zeros(n_img, np.uint8); pose_const[0] = 1
    tmask = np.zeros(n_img, np.uint8); tmask[1] = 1
    gauge = (pose_const, tmask, np.zeros(n_cam, np.uint16), np.zeros(1400, np.uint8))
    assert expected_layout(prob, gauge)[0] == 18
    opts = dict(max_iterations=6, linear_solver=solver)
    if solver == "iterative":
        opts.update(eta=1e-3, max_linear_solver_iterations=200)          # test_deterministic_gpu.py:101
    (s0, p0), (s1, p1) = (_solve_geom(det_ctx, prob, gauge, **opts) for _ in range(2))
    assert s0["linear_solver"] == (1 if solver == "direct" else 2) and s0["accumulation"] == (1 if solver == "direct" else 2)
    assert s0["final_cost"] < s0["initial_cost"] and (solver == "direct" or s0["linear_iterations"] > 0)
    assert s1["iterations"] == s0["iterations"] and s1["num_successful"] == s0["num_successful"]
    assert s1["linear_iterations"] == s0["linear_iterations"]
    assert s1["initial_cost"] == s0["initial_cost"] and s1["final_cost"] == s0["final_cost"]              # the same BITS
    for a, b in zip(p1, p0):
        assert np.array_equal(a, b)
    # one tight first step agrees with the floating-point atomics' (test_deterministic_gpu.py:123-129)
    opts = dict(max_iterations=1, linear_solver="direct") if solver == "direct" else dict(max_iterations=1, **TIGHT)
    s3, p3 = _solve_geom(det_ctx, prob, gauge, **opts)
    sf, pf = _solve_geom(atomics_ctx, prob, gauge, **opts)
    assert sf["iterations"] == s3["iterations"] and sf["num_successful"] == s3["num_successful"]
    assert abs(sf["final_cost"] - s3["final_cost"]) < 1e-7 * s3["initial_cost"]
    for a, b in zip(pf, p3):
        assert np.quantile(np.abs(a - b), 0.99) < 1e-6 * max(1.0, np.median(np.abs(b)))


# ---- 4. featuremetric: k_jac and k_img with patches at DC = 17 and 18 ----------------------------------------------------------------
def _feat_scene(cmask):
    import test_camera_models_ext as ext
    prob = ext._problem(FULL_OPENCV, seed=66)
    n_img = len(prob["image_camera"])
    pose_const = np.zeros(n_img, np.uint8); pose_const[0] = 1
    tmask = np.zeros(n_img, np.uint8); tmask[1] = 1
    return prob, (pose_const, tmask, np.full(n_img, cmask, np.uint16), np.zeros(len(prob["xyz"]), np.uint8))


@functools.lru_cache(maxsize=None)
def _feat_oracle(cmask, inner):
    import pxo
    prob, gauge = _feat_scene(cmask)
    return pxo.ba_solve(prob, pxo.cfg(), pxo.loss("cauchy", 0.25), *gauge, pxo.lm_options(max_iterations=5, use_inner_iterations=int(inner)))


def _feat_check(exact_ctx, cmask, inner, **opt_kw):
    """test_camera_models_ext.py::test_gpu_lm_with_extended_models_matches_oracle on the exact-order path, its tolerances"""
    from pixsfm_amd.engine import BAProblem, PatchArena, interp_cfg, lm_options, make_loss
    prob, gauge = _feat_scene(cmask)
    arena = PatchArena.from_numpy(exact_ctx, prob["patches"], prob["corners"], prob["scales"])
    ba = BAProblem(exact_ctx, arena, prob)
    s = ba.solve(interp_cfg(), make_loss("cauchy", [0.25]), *gauge, options=lm_options(max_iterations=5, use_inner_iterations=inner, **opt_kw))
    q, t, k, X = ba.params()
    arena.close()
    so, qo, to, ko, Xo = _feat_oracle(cmask, inner)
    print("cmask %#x inner %d %s: it %d/%d vs %d/%d, cost %.12e vs %.12e (%.2e), dq %.1e dX %.1e dk %.1e, cg %d" % (
        cmask, inner, opt_kw.get("linear_solver"), s["iterations"], s["num_successful"], so["iterations"], so["num_successful"], s["final_cost"],
        so["final_cost"], abs(s["final_cost"] - so["final_cost"]) / so["final_cost"], np.abs(q - qo).max(), np.abs(X - Xo).max(),
        np.abs(k - ko).max(), s["linear_iterations"]))
    assert s["num_camera_unknowns"] == 23 + 5 * (12 - bin(cmask).count("1"))
    assert s["iterations"] == so["iterations"] and s["num_successful"] == so["num_successful"]
    tol = 1e-4 if inner else 1e-6
    assert abs(s["final_cost"] - so["final_cost"]) < tol * max(so["final_cost"], 1e-9)
    assert np.abs(q - qo).max() < tol and np.abs(X - Xo).max() < tol and np.abs(k - ko).max() < 10 * tol * 1200
    return s


@pytest.mark.parametrize("solver", ["direct", "iterative"])
@pytest.mark.parametrize("cmask", [0, 1 << 11])
def test_featuremetric_full_opencv_matches_the_oracle(exact_ctx, cmask, solver):
    s = _feat_check(exact_ctx, cmask, False, **(dict(linear_solver="direct") if solver == "direct" else TIGHT))
    assert s["linear_solver"] == (1 if solver == "direct" else 2) and (solver == "direct" or s["linear_iterations"] > 0)


def test_featuremetric_full_opencv_with_inner_iterations(exact_ctx):
    _feat_check(exact_ctx, 0, True, linear_solver="direct")
