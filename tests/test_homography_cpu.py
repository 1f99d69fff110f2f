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
    spare, and the transfer error of the four points themselves is rounding.  Measured against the mp reference
    (tests/test_minimal_solvers_cpu.py, the same generator): err <= 0.53 kappa u with kappa (the norm of d H / d sample) up to
    5e3, so the largest |H - H_true| of about 1e-13 here is conditioning times rounding and 1e-9 leaves four decades."""
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


def test_classifier_batch_assembly_and_selection(monkeypatch):
    """classify_pairs without a GPU: the three seams (_estimate of api.two_view, api.homography and api.fundamental) are replaced
    by fakes that record the batch they are handed and return chosen results.  3 pairs over 3 images with 0, 1 and 5 matches."""
    from pixsfm_amd.api import TwoViewClassifier, TwoViewVerifier, fundamental, homography, two_view
    from pixsfm_amd.api.reconstruction import Camera
    rng = np.random.default_rng(12)
    cam1, cam2 = Camera(1, 1, 1000, 960, [1200.0, 1180, 500, 480]), Camera(2, 2, 1000, 960, [1100.0, 500, 480, 0.01])
    keypoints = {n: rng.uniform(0, 900, (7, 3)) for n in "abc"}                  # a third column (a scale, say) is not read
    cameras = {"a": cam1, "b": cam2, "c": cam1}
    pairs = [("a", "b"), ("b", "c"), ("a", "c")]
    matches = [np.zeros((0, 2), np.uint64), np.array([[3, 6]], np.uint64), np.array([[0, 1], [1, 0], [2, 5], [6, 6], [4, 3]], np.uint64)]
    scores = [np.zeros(0, np.float32), np.array([0.5], np.float32), np.linspace(0.1, 0.9, 5).astype(np.float32)]
    nan = np.full((3, 9), np.nan)
    mask_e, mask_f, mask_h = np.array([1, 1, 0, 1, 1, 1], np.uint8), np.array([1, 0, 1, 1, 1, 1], np.uint8), np.array([0, 1, 1, 0, 1, 1], np.uint8)
    results = {       # pair 0: nothing succeeds; pair 1: F alone; pair 2: E with as many inliers as F, H fails
        "E": dict(qvec=nan[:, :4], tvec=nan[:, :3], E=nan, status=np.array([1, 1, 0]), n_inliers=np.array([0, 0, 4]), n_trials=np.zeros(3, int),
                  inlier=mask_e, err=np.zeros(6)),
        "H": dict(H=nan, rot_qvec=nan[:, :4], status=np.array([1, 1, 1]), n_inliers=np.array([0, 0, 4]), n_rot_inliers=np.zeros(3, int),
                  n_trials=np.zeros(3, int), inlier=mask_h, err=np.zeros(6)),
        "F": dict(F=nan, status=np.array([1, 0, 0]), n_inliers=np.array([0, 1, 4]), n_trials=np.zeros(3, int), inlier=mask_f, err=np.zeros(6)),
    }
    seen = []
    for model, module in (("E", two_view), ("H", homography), ("F", fundamental)):
        monkeypatch.setattr(module, "_estimate", lambda ctx, batch, opts, model=model: seen.append((model, batch, dict(opts))) or results[model])

    out_m, out_s, geoms = TwoViewClassifier.create({"fundamental": {}, "homography": {"seed": 3}}).classify_pairs(keypoints, cameras, pairs, matches, scores)
    assert [s[0] for s in seen] == ["E", "H", "F"] and seen[1][2]["seed"] == 3 and seen[0][2]["seed"] == 0
    expect = dict(pair_offsets=np.array([0, 0, 1, 6]), xy1=np.concatenate([keypoints["b"][[3], :2], keypoints["a"][[0, 1, 2, 6, 4], :2]]),
                  xy2=np.concatenate([keypoints["c"][[6], :2], keypoints["c"][[1, 0, 5, 6, 3], :2]]),
                  pair_camera=np.array([[0, 1], [1, 0], [0, 0]]), cam_model=np.array([1, 2]),
                  cam_params=np.array([[1200.0, 1180, 500, 480] + [0.0] * 8, [1100.0, 500, 480, 0.01] + [0.0] * 8]))
    for _, batch, _ in seen:
        assert set(batch) == set(expect)
        for k, v in expect.items():
            assert np.array_equal(batch[k], v) and np.asarray(batch[k]).shape == v.shape, k
    assert seen[0][1] is seen[1][1] and seen[0][1] is seen[2][1]                   # one batch, so one upload, for the three
    # the class, and the matches and scores of the model that decided it
    assert [g["config"] for g in geoms] == ["DEGENERATE", "UNCALIBRATED", "CALIBRATED"]
    assert out_m[0].shape == (0, 2) and out_s[0].shape == (0,)
    assert np.array_equal(out_m[1], matches[1]) and np.array_equal(out_s[1], scores[1])                       # F's mask: [1]
    keep_e = mask_e[1:].astype(bool)
    assert np.array_equal(out_m[2], matches[2][keep_e]) and np.array_equal(out_s[2], scores[2][keep_e]) and out_m[2].dtype == np.uint64
    assert geoms[2]["success"] and geoms[2]["inliers"] == keep_e.tolist() and geoms[2]["num_inliers_F"] == 4 and geoms[1]["F"].shape == (3, 3)
    # a class outside "keep" keeps no match; without scores there are none to return
    out_m, out_s, geoms = TwoViewClassifier.create({"fundamental": {}, "keep": ("CALIBRATED",)}).classify_pairs(keypoints, cameras, pairs, matches, scores)
    assert geoms[1]["config"] == "UNCALIBRATED" and out_m[1].shape == (0, 2) and out_s[1].shape == (0,) and len(out_m[2]) == 4
    assert TwoViewClassifier.create({"fundamental": {}}).classify_pairs(keypoints, cameras, pairs, matches)[1] is None
    # without "fundamental": two seams, and the model with more inliers decides (E on a tie)
    del seen[:]
    out_m, _, geoms = TwoViewClassifier.create().classify_pairs(keypoints, cameras, pairs, matches)
    assert [s[0] for s in seen] == ["E", "H"] and geoms[2]["config"] == "CALIBRATED" and np.array_equal(out_m[2], matches[2][keep_e])
    # TwoViewVerifier.verify_pairs builds the same batch from the same input
    del seen[:]
    TwoViewVerifier.create().verify_pairs(keypoints, cameras, pairs, matches, scores)
    assert [s[0] for s in seen] == ["E"] and set(seen[0][1]) == set(expect)
    for k, v in expect.items():
        assert np.array_equal(seen[0][1][k], v), k
