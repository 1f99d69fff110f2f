"""CPU: the numpy reference of the fundamental-matrix estimator (tests/fundamental_cases.py) against ground truth, numpy.roots
and finite differences, the classification rules of api.two_view_config_uncalibrated on counts, and the argument checks of the
API functions that need no GPU."""
import numpy as np
import pytest

import fundamental_cases as fc


def test_seven_point_solver_recovers_the_fundamental_matrix():
    """256 noise-free samples of seven matches, a third each through a focal length stated x 0.7, x 1 and x 1.4.  Measured: largest
    |det F| 6.3e-17, largest |x2^t F x1| on a sample's own seven points 2.4e-15, largest distance of the closest root from the true
    F 4.6e-13; the bounds are 100 x these.  Against the mp reference of tests/test_minimal_solvers_cpu.py the same generator
    gives err <= 14 kappa u with kappa (the norm of d F / d sample) up to 1e4: the 4.6e-13 is the problem's conditioning times
    rounding, and the solver's own share is within a factor 10 of a Newton-polished solution's."""
    rec, Ft = fc.noise_free_samples(256, seed=1)
    F, valid, det = fc.seven_point(rec, details=True)
    assert det["ok"].all() and (det["n_roots"] >= 1).all() and set(det["n_roots"]) == {1, 3}
    assert np.abs(np.linalg.norm(F[valid], axis=1) - 1.0).max() <= 1e-15
    dets = np.abs(np.linalg.det(F.reshape(256, 3, 3, 3)))[valid]
    x1 = np.concatenate([rec[:, :, :2], np.ones((256, 7, 1))], 2)
    x2 = np.concatenate([rec[:, :, 2:], np.ones((256, 7, 1))], 2)
    alg = np.abs(np.einsum("bmi,brij,bmj->brm", x2, F.reshape(256, 3, 3, 3), x1))[valid]
    d = np.array([min(fc.f_distance(fc.signed(F[b, r]), Ft[b]) for r in range(3) if valid[b, r]) for b in range(256)])
    print("largest |det F| %.3e, largest |x2^t F x1| %.3e, largest distance of the closest root %.3e" % (dets.max(), alg.max(), d.max()))
    assert dets.max() <= 100 * 6.3e-17 and alg.max() <= 100 * 2.4e-15 and d.max() <= 100 * 4.6e-13


def test_degenerate_samples_give_no_hypothesis():
    rec, _ = fc.noise_free_samples(3, seed=2)
    rec[0, 1] = rec[0, 0]                                   # a repeated match: rank 6
    rec[1, :] = rec[1, 0]                                   # seven copies of one match
    rec[2, 0, 2] = np.nan
    _, valid = fc.seven_point(rec)
    assert not valid.any()


def test_cubic_roots_against_numpy_roots():
    """Random cubics with one and with three real roots, and cubics built from roots as close as 1e-3: the bisection ends at an
    interval of 2 bound 2^-64 and Newton at the rounding of the evaluation, ~ eps |c| / |p'(z)|; with roots at least 1e-3 apart
    |p'| >= 1e-6 or so, hence 1e-9 (numpy.roots itself is no better there)."""
    rng = np.random.default_rng(3)
    c = rng.normal(size=(200, 4))
    for k in range(100):
        z = np.sort(rng.uniform(-3, 3, 3))
        if k % 4 == 0:
            z[1] = z[0] + 1e-3
        c[k] = np.poly(z)[::-1] * rng.uniform(0.5, 2.0)
    c = c / np.abs(c).max(1)[:, None]
    z, n_roots, ok = fc.cubic_roots(c)
    assert ok.all() and (n_roots[:100] == 3).all() and set(n_roots[100:]) == {1, 3}
    worst = 0.0
    for b in range(200):
        want = np.roots(c[b, ::-1])
        want = np.sort(want[np.abs(want.imag) < 1e-12].real)
        assert len(want) == n_roots[b]
        assert (np.diff(z[b, :n_roots[b]]) > 0).all()
        worst = max(worst, np.abs(z[b, :n_roots[b]] - want).max())
    print("largest difference to numpy.roots %.3e" % worst)
    assert worst <= 1e-9
    # the mix: a root at infinity needs N0 + N1, not one of the null vectors alone
    assert fc.cubic_roots(np.array([[1.0, 0.5, 0.2, 1e-10]]))[2].tolist() == [False]


def test_rank_two_parametrisation_round_trips():
    """F -> (columns, alpha, beta) -> F reproduces a rank-2 F to rounding (1e-14 for unit-norm matrices whose chosen columns are
    the best conditioned pair), whichever column is the dependent one; a rank-1 or zero matrix has no parametrisation."""
    _, Ft = fc.noise_free_samples(60, seed=4)
    seen = set()
    for b in range(60):
        F = Ft[b].reshape(3, 3)[:, np.roll(np.arange(3), b % 3)].reshape(9)      # move the dependent column around
        cols, x = fc.parametrise(F)
        seen.add(cols)
        assert sorted(cols) == [0, 1, 2] and cols[0] < cols[1]
        assert np.abs(fc.build(cols, x) - F).max() <= 1e-14
        assert abs(np.linalg.det(fc.build(cols, x + 0.1).reshape(3, 3))) <= 1e-15            # rank 2 wherever the state moves
    assert len(seen) >= 2
    assert fc.parametrise(np.zeros(9)) is None
    assert fc.parametrise(np.outer([1.0, 2, 3], [0.5, -1, 2]).reshape(9)) is None


def _central(f, x, h=1e-6):
    cols = []
    for k in range(len(x)):
        e = np.zeros(len(x))
        e[k] = h
        cols.append((f(x + e) - f(x - e)) / (2 * h))
    return np.stack(cols, -1)


def test_jacobian_against_finite_differences():
    """Central differences with h = 1e-6 on Sampson residuals of order 1e-2 and derivatives of order 1: truncation ~ h^2 |f'''| ~
    1e-12, rounding ~ eps / h ~ 1e-10; 1e-7 as in the homography's test."""
    batch = fc.make_pairs(["general"], [40], (1,), seed=9, p_outlier=0.0)
    k = np.array([1200.0, 1180, 500, 480])
    rec = np.concatenate([(batch["xy1"] - k[2:]) / k[:2], (batch["xy2"] - k[2:]) / k[:2]], 1)
    rng = np.random.default_rng(4)
    F, valid = fc.seven_point(rec[None, :7])
    cols, x = fc.parametrise(F[0, np.flatnonzero(valid[0])[0]])
    x = x + 1e-3 * rng.normal(size=8)
    J = fc.f_jacobian(cols, x, rec)
    fd = _central(lambda y: fc.f_residuals(fc.build(cols, y), rec), x)
    assert J.shape == (40, 8) and np.abs(J - fd).max() <= 1e-7


def test_stop_rule_has_no_floor():
    """log(0.001) / log(1 - 0.25^7) = 113173 samples: a floor at the success rule's ratio would lie above max_num_trials."""
    o = dict(fc.DEFAULTS)
    assert fc.trials_needed(o, 10048, -1, 64) == 10048.0 and fc.trials_needed(o, 10048, 16, 64) == 10048.0
    assert 113173.0 < np.log(0.001) / np.log(1.0 - 0.25 ** 7) < 113174.0
    assert fc.trials_needed(o, 10048, 64, 64) == 64.0 and 80.0 < fc.trials_needed(o, 10048, 140, 200) < 81.0
    assert fc.sample(0, 5, 7) == (0, 1, 2, 3, 4, 5, 6) and len(set(fc.sample(7, 3, 100))) == 7


def test_classification_rules():
    from pixsfm_amd.api import two_view_config, two_view_config_uncalibrated
    T, F = True, False
    table = [  # e_ok, n_E, f_ok, n_F, h_ok, n_H, n_R, both_trusted -> class
        ((F, 0, F, 0, F, 0, 0, T), "DEGENERATE"),
        ((T, 140, T, 140, F, 0, 0, T), "CALIBRATED"),
        ((T, 133, T, 140, F, 0, 0, T), "CALIBRATED"),          # n_E = 0.95 n_F exactly: E stays
        ((T, 132, T, 140, F, 0, 0, T), "UNCALIBRATED"),
        ((T, 140, F, 0, F, 0, 0, T), "CALIBRATED"),            # F failed
        ((T, 140, T, 140, F, 0, 0, F), "UNCALIBRATED"),        # a camera that is not trusted: E is not asked
        ((T, 140, F, 0, F, 0, 0, F), "DEGENERATE"),            # ... and alone it counts for nothing
        ((F, 0, T, 140, F, 0, 0, T), "UNCALIBRATED"),
        ((T, 100, T, 100, T, 80, 80, T), "CALIBRATED"),        # n_H / n_M = 0.8 exactly: not above
        ((T, 100, T, 100, T, 81, 0, T), "PLANAR"),
        ((T, 100, T, 100, T, 100, 81, T), "PANORAMIC"),
        ((T, 100, T, 100, T, 100, 80, T), "PLANAR"),
        ((T, 100, T, 100, T, 100, 100, F), "PLANAR_OR_PANORAMIC"),
        ((T, 90, T, 100, T, 81, 81, T), "PANORAMIC"),          # M is F (90 < 95): 81 > 0.8 x 100
        ((T, 95, T, 100, T, 77, 77, T), "PANORAMIC"),          # M is E: 77 > 0.8 x 95 = 76
        ((T, 90, T, 100, T, 77, 77, T), "UNCALIBRATED"),       # M is F: 77 <= 80
        ((F, 0, F, 0, T, 140, 0, T), "PLANAR"),                # only H succeeded
        ((F, 0, F, 0, T, 140, 140, F), "PLANAR_OR_PANORAMIC"),
    ]
    for args, want in table:
        assert two_view_config_uncalibrated(*args) == want, args
    assert two_view_config_uncalibrated(T, 90, T, 100, F, 0, 0, T, min_E_F_inlier_ratio=0.9) == "CALIBRATED"
    assert two_view_config_uncalibrated(T, 100, T, 100, T, 60, 60, T, max_H_inlier_ratio=0.5) == "PANORAMIC"
    # with E and F level and both cameras trusted the rules are two_view_config's
    for n_h, n_r in ((0, 0), (80, 80), (81, 0), (100, 81), (100, 80)):
        assert two_view_config_uncalibrated(T, 100, T, 100, n_h > 0, n_h, n_r, T) == two_view_config(T, 100, n_h > 0, n_h, n_r)


def test_api_argument_errors_and_defaults():
    from pixsfm_amd.api import TwoViewClassifier, fundamental_matrix_estimation
    from pixsfm_amd.api.fundamental import conditioning_camera, fundamental_in_pixels
    from pixsfm_amd.api.homography import CONFIGS
    from pixsfm_amd.api.reconstruction import Camera
    cam = Camera(1, 1, 1000, 960, [1200.0, 1180, 500, 480])
    pts = np.zeros((8, 2))
    with pytest.raises(ValueError, match="same length"):
        fundamental_matrix_estimation(pts, pts[:7])
    with pytest.raises(ValueError, match="go together"):
        fundamental_matrix_estimation(pts, pts, camera1=cam)
    with pytest.raises(ValueError, match="unknown fundamental option"):
        fundamental_matrix_estimation(pts, pts, {"max_eror": 4.0})
    with pytest.raises(ValueError, match="unknown fundamental option"):
        fundamental_matrix_estimation(pts, pts, {"ransac": {"confidense": 0.9}})
    with pytest.raises(ValueError, match="unknown"):
        TwoViewClassifier.create({"fundamental": {"max_eror": 4.0}})
    # what the classifier held before holds still; the new keys are opt-in
    old = {"max_H_inlier_ratio": 0.8, "keep": ("CALIBRATED", "PLANAR", "PANORAMIC")}
    assert {k: TwoViewClassifier.default_conf[k] for k in old} == old
    assert TwoViewClassifier.default_conf["two_view"]["max_error"] == 4.0 and TwoViewClassifier.default_conf["homography"]["lo_rounds"] == 4
    assert TwoViewClassifier.default_conf["fundamental"] is None and TwoViewClassifier.default_conf["min_E_F_inlier_ratio"] == 0.95
    assert set(TwoViewClassifier.default_conf) == {"two_view", "homography", "max_H_inlier_ratio", "keep", "fundamental", "min_E_F_inlier_ratio"}
    assert CONFIGS[:4] == ("CALIBRATED", "PLANAR", "PANORAMIC", "DEGENERATE") and set(CONFIGS[4:]) == {"UNCALIBRATED", "PLANAR_OR_PANORAMIC"}
    plain = TwoViewClassifier.create({})
    assert plain.conf["fundamental"] is None and plain.conf["keep"] == old["keep"]
    c = TwoViewClassifier.create({"fundamental": {"ransac": {"seed": 5}}, "min_E_F_inlier_ratio": 0.9})
    assert c.conf["fundamental"]["seed"] == 5 and c.conf["fundamental"]["max_error"] == 4.0 and c.conf["min_E_F_inlier_ratio"] == 0.9
    assert set(c.conf["keep"]) == set(old["keep"]) | {"UNCALIBRATED", "PLANAR_OR_PANORAMIC"}
    assert TwoViewClassifier.create({"fundamental": {}, "keep": ["UNCALIBRATED"]}).conf["keep"] == ("UNCALIBRATED",)
    assert c.classify_pairs({}, {}, [], [], prior_focal_length={"a": False}) == ([], None, [])
    # the conditioning camera: centroid, mean distance sqrt 2 afterwards; F in the points' own units
    rng = np.random.default_rng(1)
    p = rng.uniform(0, 1000, (50, 2))
    p[3] = np.nan
    k = conditioning_camera(p)
    good = np.delete(p, 3, 0)
    assert k.model_id == 0 and np.allclose(k.params[1:], good.mean(0))
    assert abs(np.linalg.norm((good - k.params[1:]) / k.params[0], axis=1).mean() - np.sqrt(2.0)) <= 1e-12
    assert list(conditioning_camera(np.full((4, 2), np.nan)).params) == [1.0, 0.0, 0.0]
    Fn = rng.normal(size=(3, 3))
    Fp = fundamental_in_pixels(Fn, cam, k)
    x1, x2 = np.array([640.0, 200, 1]), np.array([100.0, 900, 1])
    n1 = np.array([(x1[0] - 500) / 1200, (x1[1] - 480) / 1180, 1])
    n2 = np.array([(x2[0] - k.params[1]) / k.params[0], (x2[1] - k.params[2]) / k.params[0], 1])
    assert abs(np.linalg.norm(Fp) - 1.0) <= 1e-15
    ratio = (x2 @ Fp @ x1) / (n2 @ Fn @ n1)
    y1, y2 = np.array([10.0, 20, 1]), np.array([300.0, 40, 1])
    m1 = np.array([(y1[0] - 500) / 1200, (y1[1] - 480) / 1180, 1])
    m2 = np.array([(y2[0] - k.params[1]) / k.params[0], (y2[1] - k.params[2]) / k.params[0], 1])
    assert abs((y2 @ Fp @ y1) / (m2 @ Fn @ m1) - ratio) <= 1e-9 * abs(ratio)      # one scale for every pair of points
