"""GPU: the homography kernels (csrc/pxr_homography.hip) against the numpy reference of tests/homography_cases.py, and the
two-view configurations built on them -- no pair is excused: the generated outliers sit at a transfer error of at least 20 px
under the true homography, so around the 4 px threshold there is a gap and every correct implementation ends at the generated
inlier set."""
import numpy as np
import pytest

import homography_cases as hc

pytestmark = pytest.mark.gpu


def _run(ctx, batch, H=None, rot_qvec=None, timed=False, **options):
    from pixsfm_amd.engine import HomographyProblem
    prob = HomographyProblem(ctx, batch)
    out = prob.estimate(H=H, rot_qvec=rot_qvec, timed=timed, **options)
    res = {k: a.download() for k, a in zip(hc.NAMES, out)}
    res["kernel_ms"] = prob.kernel_ms
    return res


@pytest.fixture(scope="module")
def boundary(ctx):
    batch, ref = hc.boundary_batch()
    return batch, ref, _run(ctx, batch)


def test_boundary_batch_equals_the_reference(boundary):
    """The comparisons and bounds of tests/test_homography_lanes_cpu.py (hc.compare: hc.H_TOL, hc.ROT_TOL, hc.ERR_TOL)."""
    batch, ref, got = boundary
    assert len(ref["status"]) == 38
    hc.check_reference(batch, ref)
    hc.compare(got, ref, report="GPU vs reference: ")


def test_alone_equals_inside_the_batch_and_run_to_run(ctx, boundary):
    batch, _, got = boundary
    again = _run(ctx, batch, timed=True)
    for k in hc.NAMES:
        assert np.array_equal(again[k], got[k], equal_nan=True), k
    assert set(again["kernel_ms"]) == {"records", "compact", "hypotheses", "refine"} and all(v >= 0 for v in again["kernel_ms"].values())
    off = batch["pair_offsets"]
    counts = np.diff(off)
    for n in (15, 65, 257, hc.LDS_MATCHES + 1, 2 * hc.LDS_MATCHES + 7):
        for p in np.flatnonzero(counts == n):                  # the planar and the rotation-only pair of that size; 257: the general one too
            one = _run(ctx, hc.single(batch, int(p)))
            assert one["status"][0] == (3 if batch["kind"][p] == "general" else 0)
            for k in ("H", "rot_qvec", "status", "n_inliers", "n_rot_inliers", "n_trials"):
                assert np.array_equal(one[k][0], got[k][p], equal_nan=True), (n, k)
            assert np.array_equal(one["inlier"], got["inlier"][off[p]:off[p + 1]])
            assert np.array_equal(one["err"], got["err"][off[p]:off[p + 1]], equal_nan=True)


def test_seed_changes_the_trials_not_the_inliers(ctx, boundary):
    """Rounds of 8 from 8 trials on, so that the stop rule (about 25 samples at 70 % inliers) and not the lower clamp ends a
    pair: where it ends depends on the samples, what it ends at does not."""
    batch, ref, _ = boundary
    a = _run(ctx, batch, seed=1, round_size=8, min_num_trials=8)
    b = _run(ctx, batch, seed=2, round_size=8, min_num_trials=8)
    assert not np.array_equal(a["n_trials"], b["n_trials"])
    for g in (a, b):
        assert np.array_equal(g["inlier"], ref["inlier"]) and np.array_equal(g["status"], ref["status"])
        assert np.array_equal(g["n_inliers"], ref["n_inliers"]) and np.array_equal(g["n_rot_inliers"], ref["n_rot_inliers"])


def test_every_status_code_and_untouched_sentinels(ctx):
    batch = hc.make_pairs(["planar"] * 4, [3, 40, 40, 50], (1,), seed=5, p_outlier=0.0)
    off = batch["pair_offsets"]
    batch["xy1"][off[1]:off[2]], batch["xy2"][off[1]:off[2]] = batch["xy1"][off[1]], batch["xy2"][off[1]]        # 40 copies of one match
    sH, sq = np.arange(36.0).reshape(4, 9) - 50, np.arange(16.0).reshape(4, 4) - 70
    got = _run(ctx, batch, H=sH, rot_qvec=sq, min_num_inliers=41)
    assert got["status"].tolist() == [1, 2, 3, 0] and got["n_inliers"].tolist() == [0, 0, 0, 50]
    assert np.array_equal(got["H"][:3], sH[:3]) and np.array_equal(got["rot_qvec"][:3], sq[:3])
    assert not got["inlier"][:off[3]].any() and np.isnan(got["err"][:off[3]]).all() and got["inlier"][off[3]:].all()
    assert got["n_trials"].tolist() == [0, 64, 64, 64]
    ref = hc.reference(batch, min_num_inliers=41)
    assert np.array_equal(ref["status"], got["status"]) and np.array_equal(ref["n_trials"], got["n_trials"])


def test_invalid_arguments_are_refused(ctx):
    from pixsfm_amd import PixsfmHipError
    batch = hc.make_pairs(["planar"] * 3, [10, 12, 9], (1, 2), seed=4, p_outlier=0.0)
    for change, word in ((dict(pair_offsets=np.array([0, 22, 10, 31], np.int64)), "monotone"),
                         (dict(pair_offsets=np.array([0, 10, 22, 30], np.int64)), "n_matches"),
                         (dict(pair_offsets=np.array([1, 10, 22, 31], np.int64)), "not 0"),
                         (dict(pair_camera=np.array([[0, 1], [0, 2], [1, 0]], np.int32)), "camera"),
                         (dict(pair_camera=np.array([[0, 1], [-1, 0], [1, 0]], np.int32)), "camera")):
        with pytest.raises(PixsfmHipError, match=word) as e:
            _run(ctx, dict(batch, **change))
        assert e.value.code == -1                               # PXR_EINVAL
    for bad in (dict(confidence=1.0), dict(confidence=0.0), dict(max_error=0.0), dict(round_size=0), dict(max_num_trials=0),
                dict(min_inlier_ratio=1.5), dict(min_inlier_ratio=-0.1), dict(lo_rounds=-1), dict(min_num_inliers=-1),
                dict(min_num_trials=-1), dict(refine_max_iterations=-1)):
        with pytest.raises(PixsfmHipError, match="option") as e:
            _run(ctx, batch, **bad)
        assert e.value.code == -1
    assert (_run(ctx, batch, min_num_inliers=5)["status"] == 0).all()              # the context is fine afterwards


def test_all_eleven_camera_models(ctx):
    """Every model's undistortion: noise-free planar pairs of 40 matches end at the true homography with zero residuals (the
    lanes test's bounds; measured lane by lane on the CPU: 6.9e-13 px, 5.3e-16)."""
    batch, gH = hc.eleven_models_pairs()
    got = _run(ctx, batch)
    assert (got["status"] == 0).all() and (got["n_inliers"] == 40).all()
    d = max(hc.h_distance(gH[i], got["H"][i]) for i in range(len(gH)))
    print("largest error over the eleven models, noise-free: %.3e px; H %.3e" % (got["err"].max(), d))
    assert got["err"].max() <= hc.ERR_TOL
    assert d <= hc.H_TOL
    assert (10 * got["n_rot_inliers"] <= got["n_inliers"]).all()                   # a baseline in front of a plane is no rotation


def _scene(batch):
    """The pairs of a batch as TwoViewVerifier / TwoViewClassifier take them: two images per pair, one camera."""
    from pixsfm_amd.api.reconstruction import Camera
    import triangulation_cases as tc
    cam = Camera(1, 0, 1000, 960, tc.MODEL_PARAMS[0])
    off = batch["pair_offsets"]
    kps, cams, pairs, matches, scores = {}, {}, [], [], []
    for p in range(len(off) - 1):
        a, b = "p%02d_a.jpg" % p, "p%02d_b.jpg" % p
        kps[a], kps[b] = batch["xy1"][off[p]:off[p + 1]], batch["xy2"][off[p]:off[p + 1]]
        cams[a] = cams[b] = cam
        n = int(off[p + 1] - off[p])
        pairs.append((a, b)); matches.append(np.stack([np.arange(n), np.arange(n)], 1)); scores.append(np.linspace(0.5, 1.0, n))
    return cam, kps, cams, pairs, matches, scores


def test_classifier_names_the_configurations(ctx):
    """Twelve pairs of 200 matches with 30 % outliers, four per class.  The margins are those the two references show for
    hc.CLASSIFIER_SEED: every homography ends at the 140 generated inliers and the rotation-only model keeps all of them on the
    rotation-only pairs and at most 8 on the planar ones; the essential matrix ends at 142-147 inliers on both (a few outliers
    lie by chance near their epipolar line: n_H / n_E >= 0.95, asserted as >= 0.9); on the general pairs it ends at exactly the
    generated 140, and no homography passes the success rule."""
    from pixsfm_amd.api import TwoViewClassifier, TwoViewVerifier
    batch, ref_h, ref_e = hc.classifier_batch()
    kind = np.array(batch["kind"])
    assert (ref_h["n_inliers"][kind != "general"] == 140).all() and (ref_h["status"][kind == "general"] == 3).all()
    assert (ref_h["n_rot_inliers"][kind == "rotation"] == 140).all() and (ref_h["n_rot_inliers"][kind == "planar"] <= 8).all()
    assert (ref_e["status"] == 0).all() and (ref_e["n_inliers"][kind == "general"] == 140).all() and ref_e["n_inliers"].max() <= 147
    cam, kps, cams, pairs, matches, scores = _scene(batch)
    m, s, geoms = TwoViewClassifier.create({}, ctx=ctx).classify_pairs(kps, cams, pairs, matches, scores)
    off = batch["pair_offsets"]
    for p, g in enumerate(geoms):
        assert g["config"] == hc.CLASS_OF_KIND[kind[p]], (p, kind[p], g)
        assert g["num_inliers_H"] == ref_h["n_inliers"][p] and g["num_inliers_R"] == ref_h["n_rot_inliers"][p]
        truth = batch["true_inlier"][off[p]:off[p + 1]]
        if kind[p] == "general":
            assert g["H"] is None and g["success"] and g["num_inliers"] == 140
            assert np.array_equal(m[p], matches[p][truth]) and np.array_equal(s[p], scores[p][truth])
        else:
            assert g["H"].shape == (3, 3) and g["success"] and 10 * g["num_inliers_H"] >= 9 * g["num_inliers"]
            assert set(map(tuple, matches[p][truth])) <= set(map(tuple, m[p])) and len(m[p]) == g["num_inliers"] == len(s[p])
    # what TwoViewVerifier alone reports for the rotation-only pairs: a pose like any other
    _, _, plain = TwoViewVerifier.create({}, ctx=ctx).verify_pairs(kps, cams, pairs, matches, scores)
    assert all(g["success"] and "config" not in g for g in plain)
    assert all(np.array_equal(plain[p]["E"], geoms[p]["E"]) for p in range(12))
    # keep: classes left out return no match
    m2, s2, g2 = TwoViewClassifier.create({"keep": ("CALIBRATED",)}, ctx=ctx).classify_pairs(kps, cams, pairs, matches)
    assert s2 is None and [g["config"] for g in g2] == [g["config"] for g in geoms]
    assert all((len(m2[p]) > 0) == (kind[p] == "general") for p in range(12))


def test_homography_matrix_estimation(ctx):
    from pixsfm_amd.api import homography_matrix_estimation
    batch, ref_h, _ = hc.classifier_batch()
    cam = _scene(batch)[0]
    off = batch["pair_offsets"]
    p = 1                                                   # a planar pair
    xy1, xy2, truth = batch["xy1"][off[p]:off[p + 1]], batch["xy2"][off[p]:off[p + 1]], batch["true_inlier"][off[p]:off[p + 1]]
    with_cam = homography_matrix_estimation(xy1, xy2, {"max_error": 4.0}, cam, cam, ctx=ctx)
    assert set(with_cam) == {"success", "H", "num_inliers", "inliers", "H_pixels"} and with_cam["success"] is True
    assert with_cam["inliers"] == [bool(x) for x in truth] and with_cam["num_inliers"] == 140
    assert with_cam["H"].shape == (3, 3) and hc.h_distance(with_cam["H"].reshape(9), ref_h["H"][p]) <= hc.H_TOL
    plain = homography_matrix_estimation(xy1, xy2, ctx=ctx)       # pixels in, a homography of pixels out, max_error in pixels
    assert set(plain) == {"success", "H", "num_inliers", "inliers"} and plain["inliers"] == with_cam["inliers"]
    x = np.concatenate([xy1, np.ones((len(xy1), 1))], 1)
    a, b = x @ with_cam["H_pixels"].T, x @ plain["H"].T
    d = np.abs(a[:, :2] / a[:, 2:] - b[:, :2] / b[:, 2:]).max()
    print("H_pixels and the homography of the pixels map the points %.3e px apart" % d)
    assert d <= hc.ERR_CAP          # two least-squares fits of one cost on one inlier set (one f: pixels = f x normalised + c)
    assert np.abs((a[:, :2] / a[:, 2:] - xy2)[truth]).max() < 4.0
    import triangulation_cases as tc
    from pixsfm_amd.api.reconstruction import Camera
    radial = Camera(2, 2, 1000, 960, tc.MODEL_PARAMS[2])
    assert "H_pixels" not in homography_matrix_estimation(xy1, xy2, None, radial, radial, ctx=ctx)
    assert homography_matrix_estimation(xy1[:3], xy2[:3], ctx=ctx) == {"success": False}
