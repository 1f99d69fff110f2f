"""CPU: the numpy reference of the homography estimator (tests/homography_cases.py) against ground truth and finite
differences, the classification rules of api.TwoViewClassifier on counts, and the argument checks of the API functions that
need no GPU."""
import numpy as np
import pytest

import homography_cases as hc
from pixsfm_amd import synthetic


def test_four_point_solver_recovers_the_homography():
    """256 noise-free samples of four points of a plane, spread over 0.8 of the normalised plane.  The null vector of the 8 x 9
    system moves by about eps / (its smallest singular value / its largest); four random points leave that ratio above 1e-5
    unless three of them are collinear to 1e-5 of their spread, which 256 draws do not meet: 1e-9 holds with two decades to
    spare, and the transfer error of the four points themselves is rounding."""
    rec, Ht = hc.noise_free_samples(256, seed=1)
    H, ok = hc.four_point(rec)
    assert ok.all()
    assert np.abs(np.linalg.norm(H, axis=1) - 1.0).max() <= 1e-15
    d = np.linalg.norm(H - Ht, axis=1)
    err = np.array([hc.transfer(H[b], rec[b]).max() for b in range(256)])
    print("largest |H - H_true| %.3e, largest squared transfer error of a sample %.3e" % (d.max(), err.max()))
    assert d.max() <= 1e-9 and err.max() <= 1e-24
    # the sign rule: the third component is positive on every sample point
    w = np.einsum("bk,bmk->bm", H[:, 6:], np.concatenate([rec[:, :, :2], np.ones((256, 4, 1))], 2))
    assert (w > 0).all()


def test_degenerate_samples_give_no_hypothesis():
    rec, _ = hc.noise_free_samples(3, seed=2)
    rec[0, 1] = rec[0, 0]                                   # a repeated match: rank 6
    rec[1, :, 0] = rec[1, :, 1]                             # four collinear points in image 1
    rec[1, :, 2:] = rec[1, :, :2]
    rec[2, 0, 2] = np.nan
    H, ok = hc.four_point(rec)
    assert ok.tolist() == [False, False, False]


def _central(f, x, h=1e-6):
    cols = []
    for k in range(len(x)):
        e = np.zeros(len(x))
        e[k] = h
        cols.append((f(x + e) - f(x - e)) / (2 * h))
    return np.stack(cols, -1)


def test_jacobians_against_finite_differences():
    """Central differences with h = 1e-6: truncation ~ h^2 |f'''| ~ 1e-12, rounding ~ eps / h ~ 1e-10 on residuals of order 1;
    1e-7 leaves room for the larger third derivatives near the image border."""
    batch = hc.make_pairs(["planar", "rotation"], [40, 40], (1,), seed=9, p_outlier=0.0)
    rng = np.random.default_rng(4)
    for p in range(2):
        s = slice(batch["pair_offsets"][p], batch["pair_offsets"][p + 1])
        k = np.array([1200.0, 1180, 500, 480])
        rec = np.concatenate([(batch["xy1"][s] - k[2:]) / k[:2], (batch["xy2"][s] - k[2:]) / k[:2]], 1)
        H = batch["gt_H"][p] + 1e-3 * rng.normal(size=9)
        J = hc.h_jacobian(H, rec)
        fd = _central(lambda x: hc.h_residuals(x, rec), H)
        assert np.abs(J - fd).max() <= 1e-7
        q = synthetic.rotmat_to_qvec(hc.rotation_of(H))
        q = q / np.linalg.norm(q)
        Jr = hc.rot_jacobian(q, rec)
        fdr = _central(lambda d: hc.rot_residuals(hc.quat_plus(q, d), rec), np.zeros(3))
        assert np.abs(Jr - fdr).max() <= 1e-7


def test_rotation_of_a_homography():
    rng = np.random.default_rng(6)
    q, _ = hc.tv.random_relative_pose(rng)
    R = synthetic.qvec_to_rotmat(q)
    for s in (1.0, -1.0, 0.3, -1.0 / np.sqrt(3.0)):
        assert np.abs(hc.rotation_of(s * R.reshape(9)) - R).max() <= 1e-15
    assert hc.rotation_of(np.array([0, 0, 0, 1.0, 0, 0, 0, 1, 0])) is None           # a zero row
    assert hc.rotation_of(np.array([1.0, 0, 0, 2, 0, 0, 0, 0, 1])) is None           # two parallel rows


def test_floored_stop_rule():
    """At ratio 0.25 a pair without a model stops after log(0.001) / log(1 - 0.25^4) = 1764.9 samples: 28 rounds of 64."""
    o = dict(hc.DEFAULTS)
    assert 1764.0 < hc.trials_needed(o, 10048, -1, 64) < 1766.0 and hc.trials_needed(o, 10048, 0, 64) == hc.trials_needed(o, 10048, 16, 64)
    assert hc.trials_needed(o, 10048, 45, 64) == 64.0 and hc.trials_needed(o, 10048, 64, 64) == 64.0
    assert hc.trials_needed(dict(o, min_num_inliers=41), 10048, -1, 40) == 64.0         # need > n: w is capped at 1
    assert hc.trials_needed(dict(o, min_num_inliers=0, min_inlier_ratio=0.0), 10048, -1, 40) == 10048.0
    assert hc.sample(0, 5, 4) == (0, 1, 2, 3) and len(set(hc.sample(7, 3, 100))) == 4


def test_classification_rules():
    from pixsfm_amd.api import two_view_config
    table = [  # e_ok, n_E, h_ok, n_H, n_R -> class
        ((False, 0, False, 0, 0), "DEGENERATE"),
        ((True, 140, False, 0, 0), "CALIBRATED"),
        ((True, 140, True, 14, 1), "CALIBRATED"),
        ((True, 100, True, 80, 80), "CALIBRATED"),          # n_H / n_E = 0.8 exactly: not above
        ((True, 100, True, 81, 0), "PLANAR"),
        ((True, 141, True, 140, 1), "PLANAR"),
        ((True, 100, True, 100, 80), "PLANAR"),             # n_R / n_H = 0.8 exactly: not above
        ((True, 100, True, 100, 81), "PANORAMIC"),
        ((True, 144, True, 140, 140), "PANORAMIC"),
        ((False, 0, True, 140, 0), "PLANAR"),               # only H succeeded
        ((False, 0, True, 140, 140), "PANORAMIC"),
        ((True, 20, True, 140, 140), "PANORAMIC"),          # more H inliers than E inliers
    ]
    for args, want in table:
        assert two_view_config(*args) == want, args
    assert two_view_config(True, 100, True, 60, 60, max_H_inlier_ratio=0.5) == "PANORAMIC"
    assert two_view_config(True, 100, True, 50, 50, max_H_inlier_ratio=0.5) == "CALIBRATED"


def test_api_argument_errors():
    from pixsfm_amd.api import TwoViewClassifier, homography_matrix_estimation
    from pixsfm_amd.api.reconstruction import Camera
    cam = Camera(1, 1, 1000, 960, [1200.0, 1180, 500, 480])
    pts = np.zeros((6, 2))
    with pytest.raises(ValueError, match="same length"):
        homography_matrix_estimation(pts, pts[:5])
    with pytest.raises(ValueError, match="go together"):
        homography_matrix_estimation(pts, pts, camera1=cam)
    with pytest.raises(ValueError, match="unknown homography option"):
        homography_matrix_estimation(pts, pts, {"max_eror": 4.0})
    with pytest.raises(ValueError, match="unknown homography option"):
        homography_matrix_estimation(pts, pts, {"ransac": {"confidense": 0.9}})
    for conf in ({"max_error": 4.0}, {"two_view": {"max_eror": 4.0}}, {"homography": {"max_eror": 4.0}}, {"keep": ("PLANER",)}):
        with pytest.raises(ValueError, match="unknown"):
            TwoViewClassifier.create(conf)
    c = TwoViewClassifier.create({"two_view": {"max_error": 3.0}, "homography": {"ransac": {"seed": 5}}, "max_H_inlier_ratio": 0.7, "keep": ["CALIBRATED"]})
    assert c.conf["two_view"]["max_error"] == 3.0 and c.conf["two_view"]["lo_rounds"] == 4 and c.conf["homography"]["seed"] == 5
    assert c.conf["max_H_inlier_ratio"] == 0.7 and c.conf["keep"] == ("CALIBRATED",)
    assert TwoViewClassifier.default_conf["max_H_inlier_ratio"] == 0.8 and TwoViewClassifier.default_conf["keep"] == ("CALIBRATED", "PLANAR", "PANORAMIC")
    assert c.classify_pairs({}, {}, [], []) == ([], None, []) and c.classify_pairs({}, {}, [], [], scores=[]) == ([], [], [])
    with pytest.raises(ValueError, match="same length"):
        c.classify_pairs({}, {}, [("a", "b")], [])
    with pytest.raises(KeyError, match="'b'"):
        c.classify_pairs({"a": pts}, {"a": cam, "b": cam}, [("a", "b")], [np.zeros((0, 2), int)])
