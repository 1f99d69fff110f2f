"""GPU parity: Ceres-style inner iterations (bundle_adjustment/main.py:43 default; per-point nested LM after
every trust-region step, csrc/pxr_ba_inner.hip) vs the oracle's restatement (oracle/pxo_solve.c
ba_inner_iterations).  Parity unpinned w.r.t. real Ceres; tolerances as in test_ba_solve_gpu.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["reference-order", "default"])
def arith(request, monkeypatch, exact_ctx, ctx):
    """(context, final-cost tolerance against the oracle, compare EVERY point).
    reference-order: the packed inner-iteration kernel (PXR_INNER_PACKED=1) and the exact-order evaluation -- the reference's fp32
    horizontal pass everywhere, what the oracle restates: the tolerances of rounds 1-3 (cost 1e-4: the nested LMs stop on 1e-6
    relative tolerances), every point compared (the deterministic default: one trajectory).
    default: Gram-matrix arithmetic in the nested LMs and in the outer evaluation (exact fp64): conftest.FP32_PASS_INNER_*."""
    from conftest import FP32_PASS_INNER_FINAL_COST_RTOL
    if request.param == "reference-order":
        monkeypatch.setenv("PXR_INNER_PACKED", "1")
        return exact_ctx, 1e-4, True
    monkeypatch.delenv("PXR_INNER_PACKED", raising=False)
    return ctx, FP32_PASS_INNER_FINAL_COST_RTOL, False


def _gauge(prob):
    n_img, n_cam, n_pt = len(prob["image_camera"]), len(prob["cam_model"]), len(prob["xyz"])
    pose_const = np.zeros(n_img, np.uint8); pose_const[0] = 1
    tmask = np.zeros(n_img, np.uint8); tmask[1] = 1
    return pose_const, tmask, np.full(n_cam, 0b0110, np.uint16), np.zeros(n_pt, np.uint8)


@pytest.mark.parametrize("obs_per_point,pt_sigma", [(3, 0.03), (6, 0.01)])
def test_inner_iterations_match_oracle(arith, obs_per_point, pt_sigma):
    import pxo
    ctx, cost_tol, every_point = arith
    from pixsfm_amd import synthetic
    from pixsfm_amd.engine import BAProblem, PatchArena, interp_cfg, lm_options, make_loss
    prob = synthetic.make_ba_problem(n_cams=7, n_points=50, obs_per_point=obs_per_point, seed=50 + obs_per_point,
                                     pt_sigma=pt_sigma)
    gauge = list(_gauge(prob))
    gauge[3][::9] = 1                                            # a few constant points: not refined by the inner loop
    for it in (1, 4):
        arena = PatchArena.from_numpy(ctx, prob["patches"], prob["corners"], prob["scales"])
        ba = BAProblem(ctx, arena, prob)
        s = ba.solve(interp_cfg(), make_loss("cauchy", [0.25]), *gauge,
                     options=lm_options(max_iterations=it, use_inner_iterations=True))
        q, t, k, X = ba.params()
        so, qo, to, ko, Xo = pxo.ba_solve(prob, pxo.cfg(), pxo.loss("cauchy", 0.25), *gauge,
                                          pxo.lm_options(max_iterations=it, use_inner_iterations=1))
        assert s["iterations"] == so["iterations"] and s["num_successful"] == so["num_successful"]
        # the nested LMs stop on Ceres' default tolerances (1e-6 relative cost change): a borderline decision may
        # differ by one inner iteration between the two implementations -> compare at north_star's 1e-4
        assert abs(s["final_cost"] - so["final_cost"]) < cost_tol * max(so["final_cost"], 1e-9)
        assert np.abs(q - qo).max() < 1e-4 and np.abs(t - to).max() < 1e-4
        if every_point:              # the reference's arithmetic, one deterministic trajectory: no carve-out
            assert np.abs(X - Xo).max() < 1e-4 * max(1.0, np.abs(Xo).max())
        # Points: 1e-4 -- except a point that ran away (three observations, a robust loss: seed 53 sends point 17 from inside the
        # unit cube to y = -15.8, where it projects 1 700 pixels outside its 16 x 16 patches).  There the interpolation is
        # clamped at the patch border: the cost no longer depends on the position, every solver leaves such a point wherever
        # its last step put it (run to run by 5e-3 with floating-point atomics in the outer loop).  Both solvers must lose the
        # SAME points; the costs above already agree.
        inside = np.abs(Xo).max(axis=1) < 3.0
        assert np.array_equal(inside, np.abs(X).max(axis=1) < 3.0) and inside.sum() >= len(Xo) - 2
        assert np.abs(X - Xo)[inside].max() < 1e-4
        assert np.array_equal(X[::9], prob["xyz"][::9])
    # with inner iterations the first step already lands lower than without
    arena = PatchArena.from_numpy(ctx, prob["patches"], prob["corners"], prob["scales"])
    ba0 = BAProblem(ctx, arena, prob)
    s0 = ba0.solve(interp_cfg(), make_loss("cauchy", [0.25]), *gauge, options=lm_options(max_iterations=1))
    ba1 = BAProblem(ctx, arena, prob)
    s1 = ba1.solve(interp_cfg(), make_loss("cauchy", [0.25]), *gauge,
                   options=lm_options(max_iterations=1, use_inner_iterations=True))
    assert s1["final_cost"] < s0["final_cost"]


@pytest.mark.parametrize("dtype,channels,float_simd", [(np.float16, 64, False), (np.float64, 128, False),
                                                        (np.float32, 64, True), (np.float16, 128, True)])
def test_inner_iterations_other_storage_and_float_simd(arith, dtype, channels, float_simd):
    """The nested LM for CHANNELS = 64, fp64 patches and InterpolationConfig.use_float_simd (rows of 8 lanes,
    fp32 vertical pass) against the oracle."""
    import pxo
    ctx, cost_tol, _ = arith
    from pixsfm_amd import synthetic
    from pixsfm_amd.engine import BAProblem, PatchArena, interp_cfg, lm_options, make_loss
    prob = synthetic.make_ba_problem(n_cams=6, n_points=40, obs_per_point=5, seed=77, dtype=dtype, channels=channels,
                                     pt_sigma=0.02)
    gauge = _gauge(prob)
    arena = PatchArena.from_numpy(ctx, prob["patches"], prob["corners"], prob["scales"])
    ba = BAProblem(ctx, arena, prob)
    s = ba.solve(interp_cfg(use_float_simd=float_simd), make_loss("cauchy", [0.25]), *gauge,
                 options=lm_options(max_iterations=3, use_inner_iterations=True))
    q, t, k, X = ba.params()
    so, qo, to, ko, Xo = pxo.ba_solve(prob, pxo.cfg(use_float_simd=float_simd), pxo.loss("cauchy", 0.25), *gauge,
                                      pxo.lm_options(max_iterations=3, use_inner_iterations=1))
    assert s["iterations"] == so["iterations"] and s["num_successful"] == so["num_successful"]
    assert abs(s["final_cost"] - so["final_cost"]) < cost_tol * max(so["final_cost"], 1e-9)
    assert np.abs(q - qo).max() < 1e-4 and np.abs(t - to).max() < 1e-4 and np.abs(X - Xo).max() < 1e-4


@pytest.mark.parametrize("obs_per_point,n_cams,loss,l2", [(20, 24, ("huber", 0.3), True), (40, 44, ("soft_l1", 0.3), True),
                                                          (5, 6, ("trivial", None), False), (2, 6, ("cauchy", 0.25), True)])
def test_inner_iterations_track_lengths_losses_and_unnormalised(arith, obs_per_point, n_cams, loss, l2):
    """The packed kernel's other paths: tracks of 20 / 40 observations (one point per wavefront, several trips of 16 slots,
    observation records beyond the 32 staged in LDS), four points per wavefront (tracks of two), the other robustifiers,
    un-normalised descriptors (the residual is formed per channel instead of from the channel sums)."""
    import pxo
    ctx, cost_tol, _ = arith
    from pixsfm_amd import synthetic
    from pixsfm_amd.engine import BAProblem, PatchArena, interp_cfg, lm_options, make_loss
    prob = synthetic.make_ba_problem(n_cams=n_cams, n_points=14 if obs_per_point >= 20 else 45, obs_per_point=obs_per_point,
                                     seed=90 + obs_per_point, pt_sigma=0.02)
    gauge = list(_gauge(prob))
    gauge[3][::7] = 1
    name, a = loss
    arena = PatchArena.from_numpy(ctx, prob["patches"], prob["corners"], prob["scales"])
    ba = BAProblem(ctx, arena, prob)
    s = ba.solve(interp_cfg(l2_normalize=l2), make_loss(name, [] if a is None else [a]), *gauge,
                 options=lm_options(max_iterations=2, use_inner_iterations=True))
    q, t, k, X = ba.params()
    so, qo, to, ko, Xo = pxo.ba_solve(prob, pxo.cfg(l2_normalize=l2), pxo.loss(name, a) if a is not None else pxo.loss(name),
                                      *gauge, pxo.lm_options(max_iterations=2, use_inner_iterations=1))
    assert s["iterations"] == so["iterations"] and s["num_successful"] == so["num_successful"]
    assert abs(s["final_cost"] - so["final_cost"]) < cost_tol * max(so["final_cost"], 1e-9)
    assert np.abs(q - qo).max() < 1e-4 and np.abs(t - to).max() < 1e-4 and np.abs(X - Xo).max() < 1e-4
    assert np.array_equal(X[::7], prob["xyz"][::7])


@pytest.mark.parametrize("model", [0, 1, 3, 4])
@pytest.mark.parametrize("dtype,channels", [(np.float32, 64), (np.float32, 128), (np.float16, 128)])
def test_inner_iterations_every_camera_model_and_storage(arith, model, dtype, channels):
    """Regression: the packed kernel's fp32-storage instantiation returned garbage pixel coordinates for SIMPLE_PINHOLE
    (found by tests/fuzz/fuzz_solve_vs_oracle.py: the unused d(x,y)/dk outputs of the camera model survived as private-memory
    stores behind a pointer select); the camera model is now instantiated without them there."""
    import pxo
    ctx, cost_tol, _ = arith
    from pixsfm_amd import synthetic
    from pixsfm_amd.engine import BAProblem, PatchArena, interp_cfg, lm_options, make_loss
    prob = synthetic.make_ba_problem(n_cams=5, n_points=60, obs_per_point=3, seed=11 + model, model=model, dtype=dtype,
                                     channels=channels, shared_camera=True)
    gauge = _gauge(prob)
    arena = PatchArena.from_numpy(ctx, prob["patches"], prob["corners"], prob["scales"])
    ba = BAProblem(ctx, arena, prob)
    s = ba.solve(interp_cfg(), make_loss("cauchy", [0.25]), *gauge, options=lm_options(max_iterations=2, use_inner_iterations=True))
    q, t, k, X = ba.params()
    so, qo, to, ko, Xo = pxo.ba_solve(prob, pxo.cfg(), pxo.loss("cauchy", 0.25), *gauge,
                                      pxo.lm_options(max_iterations=2, use_inner_iterations=1))
    assert s["iterations"] == so["iterations"] and s["num_successful"] == so["num_successful"]
    # These noise-free scenes converge to residuals of |r| ~ 6e-4 (|r|^2 ~ 4e-7 per block, final cost 1e-9 of the initial one),
    # where the fp32 rounding of the reference's horizontal spline pass (6e-8 per channel: 2 r . df ~ 7e-11 per block) is
    # itself ~2e-4 of the cost: the Gram-matrix kernel's nested LM (exact fp64 bicubic) and the oracle's (fp32 pass) then
    # minimise costs that differ by that much (conftest.FP32_PASS_INNER_FINAL_COST_RTOL).  In the reference's own arithmetic
    # (`arith` = reference-order) the comparison stands at the 1e-4 of rounds 1-3; the parameters at north_star's 1e-4 in both.
    assert abs(s["final_cost"] - so["final_cost"]) < cost_tol * max(so["final_cost"], 1e-9)
    assert np.abs(q - qo).max() < 1e-4 and np.abs(t - to).max() < 1e-4 and np.abs(X - Xo).max() < 1e-4


def _ragged_scene(seed, channels, dtype, n_cams=24):
    """Tracks of 2 .. 22 observations (beyond 16 the Gram matrices of a point no longer fit a wavefront's LDS: those points take
    the packed kernel), initial errors of about a texel (cells change inside the nested LM: Gram matrices are rebuilt)."""
    from pixsfm_amd import synthetic
    rng = np.random.default_rng(seed)
    prob = synthetic.make_ba_problem(n_cams=n_cams, n_points=60, obs_per_point=22, seed=seed, channels=channels, dtype=dtype,
                                     pt_sigma=0.02, rot_deg=0.3)
    keep = np.zeros(len(prob["obs_point"]), bool)
    lengths = rng.integers(2, 23, 60)
    lengths[:3] = (16, 17, 22)
    for p in range(60):
        idx = np.nonzero(prob["obs_point"] == p)[0]
        keep[idx[:lengths[p]]] = True
    for k in ("obs_image", "obs_point", "obs_patch"):
        prob[k] = prob[k][keep]
    return prob, lengths


@pytest.mark.parametrize("dtype,channels,l2,loss", [(np.float16, 128, True, "cauchy"), (np.float32, 64, True, "huber"),
                                                    (np.float16, 64, False, "trivial"), (np.float32, 128, False, "cauchy")])
def test_gram_matrix_kernel_equals_the_interpolating_kernel(ctx, monkeypatch, dtype, channels, l2, loss):
    """The inner iterations on the stencils' Gram matrices (k_inner_gram_packed: nine channel sums as quadratic forms
    in the Catmull-Rom weights, fp64 MFMA) against the kernel that interpolates the descriptor at every round (k_inner_packed,
    PXR_INNER_PACKED=1): same outer trajectory, refined parameters equal far inside the nested LM's own 1e-6 tolerances, on
    tracks of 2 .. 22 observations with texel-sized initial errors."""
    from pixsfm_amd.engine import BAProblem, PatchArena, interp_cfg, lm_options, make_loss
    prob, lengths = _ragged_scene(7, channels, dtype)
    assert lengths.max() > 16 and lengths.min() <= 3
    gauge = _gauge(prob)
    out = {}
    for mode in ("gram", "packed"):
        if mode == "packed":
            monkeypatch.setenv("PXR_INNER_PACKED", "1")
        arena = PatchArena.from_numpy(ctx, prob["patches"], prob["corners"], prob["scales"])
        ba = BAProblem(ctx, arena, prob)
        s = ba.solve(interp_cfg(l2_normalize=l2), make_loss(loss, [0.25] if loss != "trivial" else []), *gauge,
                     options=lm_options(max_iterations=3, use_inner_iterations=True))
        out[mode] = (s, ba.params())
        arena.close()
    (sg, pg), (sp, pp) = out["gram"], out["packed"]
    assert sg["iterations"] == sp["iterations"] and sg["num_successful"] == sp["num_successful"]
    assert abs(sg["initial_cost"] - sp["initial_cost"]) <= 1e-13 * sp["initial_cost"]
    assert abs(sg["final_cost"] - sp["final_cost"]) < 2e-6 * sp["final_cost"]
    for a, b in zip(pg, pp):
        assert (np.abs(a - b) <= 2e-6 * np.maximum(1.0, np.abs(b))).all()
    # the first iteration's refinement really moved the points (the kernels did run)
    assert np.abs(pg[3] - prob["xyz"]).max() > 1e-4
