"""GPU: the fundamental-matrix kernels (csrc/pxr_fundamental.hip) against the numpy reference of tests/fundamental_cases.py, the
pycolmap-shaped function and the opt-in path of api.TwoViewClassifier built on them -- no pair is excused: the generated outliers
sit at a Sampson distance of at least 20 px under the true geometry, so around the 4 px threshold there is a gap and every correct
implementation ends at the generated inlier set."""
import numpy as np
import pytest

import fundamental_cases as fc
import homography_cases as hc

pytestmark = pytest.mark.gpu


def _run(ctx, batch, F=None, timed=False, **options):
    from pixsfm_amd.engine import FundamentalProblem
    prob = FundamentalProblem(ctx, batch)
    out = prob.estimate(F=F, timed=timed, **options)
    res = {k: a.download() for k, a in zip(fc.NAMES, out)}
    res["kernel_ms"] = prob.kernel_ms
    return res


@pytest.fixture(scope="module")
def boundary(ctx):
    batch, ref = fc.boundary_batch()
    return batch, ref, _run(ctx, batch)


def test_boundary_batch_equals_the_reference(boundary):
    """The comparisons and bounds of tests/test_fundamental_lanes_cpu.py (fc.compare: fc.F_TOL, fc.ERR_TOL)."""
    batch, ref, got = boundary
    assert len(ref["status"]) == 37
    fc.check_reference(batch, ref)
    fc.compare(got, ref, report="GPU vs reference: ")


def test_alone_equals_inside_the_batch_and_run_to_run(ctx, boundary):
    batch, _, got = boundary
    again = _run(ctx, batch, timed=True)
    for k in fc.NAMES:
        assert np.array_equal(again[k], got[k], equal_nan=True), k
    assert set(again["kernel_ms"]) == {"records", "compact", "hypotheses", "refine"} and all(v >= 0 for v in again["kernel_ms"].values())
    off = batch["pair_offsets"]
    counts = np.diff(off)
    for n in (15, 65, 257, fc.LDS_MATCHES + 1, 2 * fc.LDS_MATCHES + 7):
        for p in np.flatnonzero(counts == n):
            one = _run(ctx, fc.single(batch, int(p)))
            assert one["status"][0] == 0
            for k in ("F", "status", "n_inliers", "n_trials"):
                assert np.array_equal(one[k][0], got[k][p], equal_nan=True), (n, k)
            assert np.array_equal(one["inlier"], got["inlier"][off[p]:off[p + 1]])
            assert np.array_equal(one["err"], got["err"][off[p]:off[p + 1]], equal_nan=True)


def test_every_status_code_and_untouched_sentinels(ctx):
    batch = fc.make_pairs(["general"] * 4, [6, 7, 40, 50], (1,), seed=5, p_outlier=0.0)
    off = batch["pair_offsets"]
    batch["xy1"][off[1]:off[2]], batch["xy2"][off[1]:off[2]] = batch["xy1"][off[1]], batch["xy2"][off[1]]          # seven copies of one match
    sF = np.arange(36.0).reshape(4, 9) - 50
    got = _run(ctx, batch, F=sF, min_num_inliers=41, max_num_trials=256)
    assert got["status"].tolist() == [1, 2, 3, 0] and got["n_inliers"].tolist() == [0, 0, 0, 50]
    assert np.array_equal(got["F"][:3], sF[:3])
    assert not got["inlier"][:off[3]].any() and np.isnan(got["err"][:off[3]]).all() and got["inlier"][off[3]:].all()
    assert got["n_trials"].tolist() == [0, 256, 64, 64]
    ref = fc.reference(batch, min_num_inliers=41, max_num_trials=256)
    assert np.array_equal(ref["status"], got["status"]) and np.array_equal(ref["n_trials"], got["n_trials"])


def test_invalid_arguments_are_refused(ctx):
    from pixsfm_amd import PixsfmHipError
    batch = hc.make_pairs(["general"] * 3, [10, 12, 9], (1, 2), seed=4, p_outlier=0.0)
    for change, word in ((dict(pair_offsets=np.array([0, 22, 10, 31], np.int64)), "monotone"),
                         (dict(pair_offsets=np.array([0, 10, 22, 30], np.int64)), "n_matches"),
                         (dict(pair_offsets=np.array([1, 10, 22, 31], np.int64)), "not 0"),
                         (dict(pair_camera=np.array([[0, 1], [0, 2], [1, 0]], np.int32)), "camera"),
                         (dict(pair_camera=np.array([[0, 1], [-1, 0], [1, 0]], np.int32)), "camera")):
        with pytest.raises(PixsfmHipError, match=word) as e:
            _run(ctx, dict(batch, **change))
        assert e.value.code == -1                               # PXR_EINVAL
    for bad in (dict(confidence=1.0), dict(max_error=0.0), dict(round_size=0), dict(max_num_trials=0), dict(min_inlier_ratio=1.5),
                dict(lo_rounds=-1), dict(min_num_inliers=-1), dict(min_num_trials=-1), dict(refine_max_iterations=-1)):
        with pytest.raises(PixsfmHipError, match="option") as e:
            _run(ctx, batch, **bad)
        assert e.value.code == -1
    assert (_run(ctx, batch, min_num_inliers=7)["status"] == 0).all()              # the context is fine afterwards


def test_all_eleven_camera_models(ctx):
    """Every model's undistortion: noise-free pairs of 40 matches end at the true fundamental matrix with zero residuals.  The
    error bound is the lanes test's; F is held to fc.POSE_CAP: 40 noise-free matches fix it to rounding times the conditioning of
    the 40 x 9 system, which the lanes test's bound (a kernel-against-reference difference) does not cover."""
    batch, gF = fc.eleven_models_pairs()
    got = _run(ctx, batch)
    assert (got["status"] == 0).all() and (got["n_inliers"] == 40).all()
    d = max(fc.f_distance(gF[i], got["F"][i]) for i in range(len(gF)))
    print("largest error over the eleven models, noise-free: %.3e px; F %.3e" % (got["err"].max(), d))
    assert got["err"].max() <= fc.ERR_TOL
    assert d <= fc.POSE_CAP


def _scene(batch, trusted_focal=1200.0):
    """The pairs of a batch as TwoViewClassifier takes them: two images per pair, both through the pair's (one) camera; an image
    whose stated focal length is not the true one is marked as having no prior."""
    from pixsfm_amd.api.reconstruction import Camera
    off = batch["pair_offsets"]
    kps, cams, pairs, matches, scores, prior = {}, {}, [], [], [], {}
    for p in range(len(off) - 1):
        a, b = "p%02d_a.jpg" % p, "p%02d_b.jpg" % p
        kps[a], kps[b] = batch["xy1"][off[p]:off[p + 1]], batch["xy2"][off[p]:off[p + 1]]
        c = int(batch["pair_camera"][p][0])
        cams[a] = cams[b] = Camera(c + 1, 0, 1000, 960, batch["cam_params"][c][:3])
        prior[a] = prior[b] = bool(batch["cam_params"][c][0] == trusted_focal)
        n = int(off[p + 1] - off[p])
        pairs.append((a, b)); matches.append(np.stack([np.arange(n), np.arange(n)], 1)); scores.append(np.linspace(0.5, 1.0, n))
    return kps, cams, pairs, matches, scores, prior


def test_fundamental_matrix_estimation(ctx):
    """Raw pixels in, no camera: the conditioning happens on the host and F comes back in pixels.  Measured on an MI355X: the
    generated inliers lie at most 1.2 px (Sampson) from the returned F, and the two ways to F in pixels -- conditioned by the data,
    or normalised by the true camera and mapped by K^-t F K^-1 -- differ by 2.0e-8 in Frobenius norm: two least-squares fits on one
    inlier set of costs that are not quite the same (the Sampson distance of the normalised planes weighs the two images by their
    own conditioning scales, which differ by a few per cent).  Held to 100 x that."""
    from pixsfm_amd.api import fundamental_matrix_estimation
    from pixsfm_amd.api.reconstruction import Camera
    import triangulation_cases as tc
    batch, ref_f, _, _ = fc.uncalibrated_batch()
    off = batch["pair_offsets"]
    p = 0                                                   # a general pair
    xy1, xy2, truth = batch["xy1"][off[p]:off[p + 1]], batch["xy2"][off[p]:off[p + 1]], batch["true_inlier"][off[p]:off[p + 1]]
    cam = Camera(1, 0, 1000, 960, tc.MODEL_PARAMS[0])
    with_cam = fundamental_matrix_estimation(xy1, xy2, {"max_error": 4.0}, cam, cam, ctx=ctx)
    assert set(with_cam) == {"success", "F", "num_inliers", "inliers", "F_pixels"} and with_cam["success"] is True
    assert with_cam["inliers"] == [bool(x) for x in truth] and with_cam["num_inliers"] == 140
    assert with_cam["F"].shape == (3, 3) and fc.f_distance(with_cam["F"], ref_f["F"][p]) <= fc.F_TOL
    plain = fundamental_matrix_estimation(xy1, xy2, ctx=ctx)
    assert set(plain) == {"success", "F", "num_inliers", "inliers"} and plain["inliers"] == with_cam["inliers"]
    assert abs(np.linalg.norm(plain["F"]) - 1.0) <= 1e-12
    rec = np.concatenate([xy1, xy2], 1)
    d = np.sqrt(fc.sampson(plain["F"].reshape(9), rec))
    a, b = fc.signed(plain["F"]), fc.signed(with_cam["F_pixels"])
    print("largest Sampson distance of a generated inlier %.3e px; F and F_pixels %.3e apart" % (d[truth].max(), fc.f_distance(a, b)))
    assert d[truth].max() < 4.0 and d[~truth].min() > 4.0
    assert fc.f_distance(a, b) <= 100 * 2.0e-8
    radial = Camera(2, 2, 1000, 960, tc.MODEL_PARAMS[2])
    assert "F_pixels" not in fundamental_matrix_estimation(xy1, xy2, None, radial, radial, ctx=ctx)
    assert fundamental_matrix_estimation(xy1[:6], xy2[:6], ctx=ctx) == {"success": False}


def test_classifier_with_the_fundamental_matrix(ctx):
    """Six pairs of 200 matches with 30 % outliers: two general pairs with their true focal length, the same two with the focal
    length x 0.7, a planar and a rotation-only pair.  First what the references alone say (fc.CLASSIFIER_SEED was chosen for it):
    F ends at the 140 generated inliers on all four general pairs, E too under the true focal length but below 0.95 x 140 under
    the wrong one; then that the kernels name every pair as generated, with trusted cameras and without."""
    from pixsfm_amd.api import TwoViewClassifier
    batch, ref_f, ref_e, ref_h = fc.uncalibrated_batch()
    kind, wrong = np.array(batch["kind"]), batch["focal_scale"] != 1.0
    general = kind == "general"
    off = batch["pair_offsets"]
    assert (ref_f["status"] == 0).all() and (ref_f["n_inliers"][general] == 140).all()
    assert np.array_equal(ref_f["inlier"][:off[4]].astype(bool), batch["true_inlier"][:off[4]])
    assert (ref_e["n_inliers"][general & ~wrong] == 140).all() and wrong.sum() == 2
    assert (ref_e["n_inliers"][wrong] < 0.95 * ref_f["n_inliers"][wrong]).all()
    assert (ref_h["status"][general] == 3).all() and (ref_h["n_inliers"][~general] == 140).all()
    assert ref_h["n_rot_inliers"][kind == "rotation"] == 140 and ref_h["n_rot_inliers"][kind == "planar"] <= 8
    assert (ref_h["n_inliers"][~general] > 0.8 * np.maximum(ref_e["n_inliers"], ref_f["n_inliers"])[~general]).all()

    kps, cams, pairs, matches, scores, prior = _scene(batch)
    clf = TwoViewClassifier.create({"fundamental": {}}, ctx=ctx)
    want_trusted = ["CALIBRATED", "CALIBRATED", "UNCALIBRATED", "UNCALIBRATED", "PLANAR", "PANORAMIC"]
    m, s, geoms = clf.classify_pairs(kps, cams, pairs, matches, scores)                       # every camera trusted
    assert [g["config"] for g in geoms] == want_trusted
    for p, g in enumerate(geoms):
        assert g["num_inliers_F"] == ref_f["n_inliers"][p] and g["F"].shape == (3, 3)
        assert fc.f_distance(g["F"], ref_f["F"][p]) <= fc.F_TOL
        assert g["num_inliers_H"] == ref_h["n_inliers"][p] and (g["num_inliers"] if g["success"] else 0) == ref_e["n_inliers"][p]
        truth = batch["true_inlier"][off[p]:off[p + 1]]
        decides = {"CALIBRATED": ref_e, "UNCALIBRATED": ref_f, "PLANAR": ref_h, "PANORAMIC": ref_h}[g["config"]]
        keep = decides["inlier"][off[p]:off[p + 1]].astype(bool)                  # the inliers of the model that decided the class
        assert np.array_equal(m[p], matches[p][keep]) and np.array_equal(s[p], scores[p][keep])
        if general[p] and wrong[p]:                          # ... which is the generated set where F decided
            assert np.array_equal(keep, truth)
    # the images whose focal length is off are declared so: E is not asked there; nothing else changes
    m2, _, g2 = clf.classify_pairs(kps, cams, pairs, matches, prior_focal_length=prior)
    assert [g["config"] for g in g2] == want_trusted and all(np.array_equal(x, y) for x, y in zip(m, m2))
    # no camera trusted at all
    none = {n: False for n in kps}
    m3, _, g3 = clf.classify_pairs(kps, cams, pairs, matches, prior_focal_length=none)
    assert [g["config"] for g in g3] == ["UNCALIBRATED"] * 4 + ["PLANAR_OR_PANORAMIC"] * 2
    assert all(np.array_equal(m3[p], matches[p][batch["true_inlier"][off[p]:off[p + 1]]]) for p in range(4))
    assert all(np.array_equal(m3[p], m[p]) for p in (4, 5))
    # keep
    m4, _, g4 = TwoViewClassifier.create({"fundamental": {}, "keep": ("UNCALIBRATED",)}, ctx=ctx).classify_pairs(kps, cams, pairs, matches)
    assert [g["config"] for g in g4] == want_trusted and [len(x) > 0 for x in m4] == [False, False, True, True, False, False]


def test_classifier_without_the_fundamental_matrix_is_unchanged(ctx):
    """"fundamental": None (the default) launches nothing new and returns what the classifier returned before it knew the option:
    the keys, classes, counts and arrays on hc.classifier_batch(), which are those of the two references there."""
    from pixsfm_amd.api import TwoViewClassifier
    batch, ref_h, ref_e = hc.classifier_batch()
    kps, cams, pairs, matches, scores, _ = _scene(batch)
    off = batch["pair_offsets"]
    launched = []
    import pixsfm_amd.api.fundamental as mod               # its _estimate is the classifier's only way to pxr_fundamental
    real = mod._estimate
    mod._estimate = lambda *a, **k: launched.append(a) or real(*a, **k)
    try:
        outs = [TwoViewClassifier.create(conf, ctx=ctx).classify_pairs(kps, cams, pairs, matches, scores) for conf in ({}, {"fundamental": None})]
    finally:
        mod._estimate = real
    assert not launched
    for m, s, geoms in outs:
        for p, g in enumerate(geoms):
            assert set(g) == {"success", "E", "qvec", "tvec", "num_inliers", "inliers", "config", "H", "num_inliers_H", "num_inliers_R"}
            assert g["config"] == hc.CLASS_OF_KIND[batch["kind"][p]]
            assert g["num_inliers"] == ref_e["n_inliers"][p] and g["num_inliers_H"] == ref_h["n_inliers"][p]
            assert g["num_inliers_R"] == ref_h["n_rot_inliers"][p]
            assert g["inliers"] == [bool(x) for x in ref_e["inlier"][off[p]:off[p + 1]]]
            keep = (ref_h if ref_h["n_inliers"][p] > ref_e["n_inliers"][p] else ref_e)["inlier"][off[p]:off[p + 1]].astype(bool)
            assert np.array_equal(m[p], matches[p][keep]) and np.array_equal(s[p], scores[p][keep])
    for (ma, sa, ga), (mb, sb, gb) in [outs]:
        for p in range(len(ga)):
            assert np.array_equal(ma[p], mb[p]) and np.array_equal(sa[p], sb[p])
            for k in ga[p]:
                assert np.array_equal(ga[p][k], gb[p][k]) if isinstance(ga[p][k], np.ndarray) else ga[p][k] == gb[p][k], k
