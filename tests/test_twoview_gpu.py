"""GPU: the two-view geometry kernels (csrc/pxr_twoview.hip) against the numpy reference of tests/twoview_cases.py -- no pair is
excused: the generated outliers sit at a Sampson distance of at least 20 px under the true geometry, so around the 4 px
threshold there is a gap and every correct implementation ends at the generated inlier set."""
import numpy as np
import pytest

import triangulation_cases as tc
import twoview_cases as tv

pytestmark = pytest.mark.gpu


def _run(ctx, batch, qvec=None, tvec=None, E=None, timed=False, **options):
    from pixsfm_amd.engine import TwoViewProblem
    prob = TwoViewProblem(ctx, batch)
    out = prob.estimate(qvec=qvec, tvec=tvec, E=E, timed=timed, **options)
    res = {k: a.download() for k, a in zip(tv.NAMES, out)}
    res["kernel_ms"] = prob.kernel_ms
    return res


@pytest.fixture(scope="module")
def boundary(ctx):
    batch, ref = tv.boundary_batch()
    return batch, ref, _run(ctx, batch)


def test_boundary_batch_equals_the_reference(boundary):
    """The comparisons and bounds of tests/test_twoview_lanes_cpu.py (tv.compare: tv.POSE_TOL, tv.ERR_TOL)."""
    batch, ref, got = boundary
    assert {0, 1, 3}.issubset(set(ref["status"])) and len(ref["status"]) == 54
    assert np.array_equal(ref["inlier"].astype(bool), batch["true_inlier"] & np.repeat(ref["status"] == 0, np.diff(batch["pair_offsets"])))
    tv.compare(got, ref, report="GPU vs reference: ")


def test_alone_equals_inside_the_batch_and_run_to_run(ctx, boundary):
    batch, _, got = boundary
    again = _run(ctx, batch, timed=True)
    for k in tv.NAMES:
        assert np.array_equal(again[k], got[k], equal_nan=True), k
    assert set(again["kernel_ms"]) == {"records", "compact", "hypotheses", "refine"} and all(v >= 0 for v in again["kernel_ms"].values())
    off = batch["pair_offsets"]
    counts = np.diff(off)
    for n in (15, 65, 257, tv.LDS_MATCHES + 1, 2 * tv.LDS_MATCHES + 7):
        p = int(np.flatnonzero(counts == n)[2])
        one = _run(ctx, tv.single(batch, p))
        assert one["status"][0] == 0
        for k in ("qvec", "tvec", "E", "status", "n_inliers", "n_trials"):
            assert np.array_equal(one[k][0], got[k][p]), (n, k)
        assert np.array_equal(one["inlier"], got["inlier"][off[p]:off[p + 1]])
        assert np.array_equal(one["err"], got["err"][off[p]:off[p + 1]], equal_nan=True)


def test_every_status_code_and_untouched_sentinels(ctx):
    batch = tv.make_pairs([4, 40, 40, 50], (1,), seed=5, p_outlier=0.0)
    off = batch["pair_offsets"]
    batch["xy1"][off[1]:off[2]], batch["xy2"][off[1]:off[2]] = batch["xy1"][off[1]], batch["xy2"][off[1]]        # 40 copies of one match
    sq, stv, sE = np.arange(16.0).reshape(4, 4) - 50, np.arange(12.0).reshape(4, 3) - 70, np.arange(36.0).reshape(4, 9) - 90
    got = _run(ctx, batch, qvec=sq, tvec=stv, E=sE, min_num_inliers=41)
    assert got["status"].tolist() == [1, 2, 3, 0] and got["n_inliers"].tolist() == [0, 0, 0, 50]
    assert np.array_equal(got["qvec"][:3], sq[:3]) and np.array_equal(got["tvec"][:3], stv[:3]) and np.array_equal(got["E"][:3], sE[:3])
    assert not got["inlier"][:off[3]].any() and np.isnan(got["err"][:off[3]]).all() and got["inlier"][off[3]:].all()
    assert got["n_trials"].tolist()[:2] == [0, 10048] and got["n_trials"][2:].min() >= 64
    ref = tv.reference(batch, min_num_inliers=41)
    assert np.array_equal(ref["status"], got["status"]) and np.array_equal(ref["n_trials"], got["n_trials"])


def test_unusable_matches_leave_their_neighbours_alone(ctx):
    batch = tv.make_pairs([40, 6, 120], (2, 8), seed=21, p_outlier=0.25)
    clean = _run(ctx, batch, min_num_inliers=5)
    assert (clean["status"] == 0).all()
    dirty = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in batch.items()}
    off = batch["pair_offsets"]
    bad = [off[0] + 3, off[0] + 17, off[1] + 1, off[1] + 4, off[2] + 60, off[2] + 61]
    dirty["xy1"][bad[0], 0] = np.nan
    dirty["xy2"][bad[1]] = np.inf
    dirty["xy2"][bad[2], 1] = np.nan
    dirty["xy1"][bad[3], 1] = -np.inf                          # pair 1 keeps 4 usable matches: status 1
    dirty["xy1"][bad[4]] = np.nan
    dirty["xy2"][bad[5], 0] = np.inf
    got = _run(ctx, dirty, min_num_inliers=5)
    assert got["status"].tolist() == [0, 1, 0]
    assert not got["inlier"][bad].any() and np.isnan(got["err"][bad]).all()
    # the same pairs with the unusable rows taken out give the same bits
    keep = np.ones(off[-1], bool)
    keep[bad] = False
    cut = dict(dirty, xy1=dirty["xy1"][keep], xy2=dirty["xy2"][keep],
               pair_offsets=np.concatenate([[0], np.cumsum([keep[off[i]:off[i + 1]].sum() for i in range(3)])]).astype(np.int64))
    want = _run(ctx, cut, min_num_inliers=5)
    for k in ("qvec", "tvec", "E", "status", "n_inliers", "n_trials"):
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    assert np.array_equal(got["inlier"][keep], want["inlier"]) and np.array_equal(got["err"][keep], want["err"], equal_nan=True)
    ref = tv.reference(dirty, min_num_inliers=5)
    tv.compare(got, ref, report="with unusable rows, GPU vs reference: ")


def test_invalid_arguments_are_refused(ctx):
    from pixsfm_amd import PixsfmHipError
    batch = tv.make_pairs([10, 12, 9], (1, 2), seed=4, p_outlier=0.0)
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
    # one prior array without the other: engine.TwoViewProblem refuses that itself, so the library is called directly
    import ctypes as C
    from pixsfm_amd.engine import TwoViewProblem, check, two_view_options
    prob = TwoViewProblem(ctx, dict(batch, prior_qvec=np.tile([1.0, 0, 0, 0], (3, 1)), prior_tvec=np.tile([1.0, 0, 0], (3, 1))))
    d, T, N = prob.d, prob.n_pairs, prob.n_matches
    outs = [ctx.empty((T, 4), np.float64), ctx.empty((T, 3), np.float64), ctx.empty((T, 9), np.float64), ctx.empty((T,), np.int32),
            ctx.empty((T,), np.int32), ctx.empty((T,), np.int32), ctx.empty((N,), np.uint8), ctx.empty((N,), np.float64)]
    opts = two_view_options()
    for prior in ((d["prior_qvec"].ptr, None), (None, d["prior_tvec"].ptr)):
        with pytest.raises(PixsfmHipError, match="prior") as e:
            check(ctx.lib.pxr_two_view_geometry(ctx.handle, T, d["pair_offsets"].ptr, N, d["xy1"].ptr, d["xy2"].ptr, d["pair_camera"].ptr,
                                                prob.n_cameras, d["cam_model"].ptr, d["cam_params"].ptr, prior[0], prior[1], C.byref(opts),
                                                *[o.ptr for o in outs]), "pxr_two_view_geometry")
        assert e.value.code == -1
    assert (_run(ctx, batch, min_num_inliers=5)["status"] == 0).all()              # the context is fine afterwards


def test_all_eleven_camera_models(ctx):
    """Every model's undistortion: noise-free pairs of 40 matches end at a zero-residual pose (the lanes test's bounds)."""
    batch, gq, gt = tv.eleven_models_pairs()
    L = len(batch["cam_model"])
    got = _run(ctx, batch)
    assert (got["status"] == 0).all() and (got["n_inliers"] == 40).all()
    d = np.array([tv.pose_distance(gq[i], gt[i], got["qvec"][i], got["tvec"][i]) for i in range(L)])
    print("largest error over the eleven models, noise-free: %.3e px; pose %.3e rad" % (got["err"].max(), d.max()))
    assert got["err"].max() <= tv.ERR_TOL
    assert d.max() <= tv.POSE_TOL


def test_pose_prior_mode(ctx):
    batch = tv.make_pairs([4, 30, 70, tv.LDS_MATCHES + 1], (1, 2, 8), seed=61, p_outlier=0.3)
    batch = dict(batch, prior_qvec=batch["gt_qvec"], prior_tvec=2.5 * batch["gt_tvec"])
    got = _run(ctx, batch)
    ref = tv.reference(batch)
    assert got["status"].tolist() == [1, 0, 0, 0] and (got["n_trials"] == 0).all()
    assert np.array_equal(got["inlier"], ref["inlier"]) and np.array_equal(got["n_inliers"], ref["n_inliers"])
    assert np.array_equal(got["inlier"][4:].astype(bool), batch["true_inlier"][4:])
    assert np.array_equal(got["qvec"][1:], batch["prior_qvec"][1:]) and np.array_equal(got["tvec"][1:], batch["prior_tvec"][1:])
    assert np.isnan(got["qvec"][0]).all()
    have = ~np.isnan(ref["err"])
    assert np.array_equal(np.isnan(got["err"]), ~have) and np.abs(got["err"][have] - ref["err"][have]).max() <= tv.ERR_TOL


HARD_SEED = 43


def test_hard_pairs(ctx):
    """16 pairs of 300 matches, 60 % outliers drawn uniformly with no minimum distance: every pair succeeds, the mask is the
    error test, contains every generated inlier, and the trials stay within the stop rule's count for w = 0.4 (672 -> 704).  The
    last needs all-inlier samples among the first 704.  All pairs of one size share their samples, so that is a property of
    the data alone: the seed used here is one for which every pair has at least two (checked below from the hash, without the
    kernel)."""
    batch = tv.make_pairs([300] * 16, (2, 1, 8), seed=HARD_SEED, p_outlier=0.6, min_outlier_sampson=None)
    fives = np.array([tv.sample(0, h, 300) for h in range(704)])
    assert batch["true_inlier"].reshape(16, 300)[:, fives].all(2).sum(1).min() >= 2
    got = _run(ctx, batch)
    assert (got["status"] == 0).all()
    with np.errstate(invalid="ignore"):
        assert np.array_equal(got["inlier"].astype(bool), got["err"] <= 4.0)
    assert got["inlier"].astype(bool)[batch["true_inlier"]].all()
    assert (got["n_inliers"] >= 120).all()
    bound = int(np.ceil(tv.trials_needed(dict(tv.DEFAULTS), 10048, 120, 300) / 64)) * 64
    assert bound == 704 and got["n_trials"].max() <= bound and got["n_trials"].min() >= 64
    d = np.array([tv.pose_distance(batch["gt_qvec"][i], batch["gt_tvec"][i], got["qvec"][i], got["tvec"][i]) for i in range(16)])
    assert d[:, 0].max() < 1e-2


def test_api_shapes(ctx):
    from pixsfm_amd.api import TwoViewVerifier, essential_matrix_estimation
    from pixsfm_amd.api.keypoint_adjustment import build_matching_graph
    from pixsfm_amd.api.reconstruction import Camera
    batch = tv.make_pairs([60, 80, 30], (2, 1), seed=51, p_outlier=0.3)
    off = batch["pair_offsets"]
    cams = {1: Camera(1, 2, 1000, 960, tc.MODEL_PARAMS[2]), 2: Camera(2, 1, 1000, 960, tc.MODEL_PARAMS[1])}
    one = essential_matrix_estimation(batch["xy1"][:off[1]], batch["xy2"][:off[1]], cams[1], cams[2], {"max_error": 4}, ctx=ctx)
    assert set(one) == {"success", "E", "qvec", "tvec", "num_inliers", "inliers"} and one["success"] is True
    assert one["inliers"] == [bool(x) for x in batch["true_inlier"][:off[1]]] and one["num_inliers"] == sum(one["inliers"])
    assert one["E"].shape == (3, 3) and one["qvec"].shape == (4,) and one["tvec"].shape == (3,) and one["E"].dtype == np.float64
    assert essential_matrix_estimation(batch["xy1"][:4], batch["xy2"][:4], cams[1], cams[2], ctx=ctx) == {"success": False}
    # three pairs over three images: a.jpg (camera 1) - b.jpg (camera 2), b - c (camera 1), c - a; the third pair is noise
    names = ["a.jpg", "b.jpg", "c.jpg"]
    image_cam = {"a.jpg": cams[1], "b.jpg": cams[2], "c.jpg": cams[1]}
    pairs = [("a.jpg", "b.jpg"), ("b.jpg", "c.jpg"), ("c.jpg", "a.jpg")]
    side = [batch["xy1"][off[p]:off[p + 1]] for p in range(3)], [batch["xy2"][off[p]:off[p + 1]] for p in range(3)]
    rng = np.random.default_rng(2)
    side[1][2][:] = rng.uniform(0, 900, side[1][2].shape)
    # the keypoints of an image: what its pairs see, stacked; matches index them
    keypoints = {"a.jpg": np.concatenate([side[0][0], side[1][2]]), "b.jpg": np.concatenate([side[1][0], side[0][1]]),
                 "c.jpg": np.concatenate([side[1][1], side[0][2]])}
    n0, n1, n2 = (int(off[p + 1] - off[p]) for p in range(3))
    matches = [np.stack([np.arange(n0), np.arange(n0)], 1), np.stack([n0 + np.arange(n1), np.arange(n1)], 1),
               np.stack([n1 + np.arange(n2), n0 + np.arange(n2)], 1)]
    scores = [np.linspace(0.5, 1.0, len(m)) for m in matches]
    verifier = TwoViewVerifier.create({"max_error": 4.0}, ctx=ctx)
    v_matches, v_scores, geoms = verifier.verify_pairs(keypoints, image_cam, pairs, matches, scores)
    assert len(v_matches) == len(v_scores) == len(geoms) == 3
    for p in range(2):
        keep = batch["true_inlier"][off[p]:off[p + 1]]
        assert np.array_equal(v_matches[p], matches[p][keep]) and np.array_equal(v_scores[p], scores[p][keep])
        assert geoms[p]["success"] and geoms[p]["num_inliers"] == keep.sum()
    assert len(v_matches[2]) == 0 and len(v_scores[2]) == 0 and not geoms[2]["success"]
    graph = build_matching_graph(pairs, v_matches, v_scores)
    assert graph is not None
    with pytest.raises(ValueError):
        TwoViewVerifier.create({"max_eror": 4.0})


def test_verifier_takes_the_merged_tracks_apart(ctx):
    """The scene of examples/match_verify_triangulate.py, smaller: a fifth of the points carries another point's descriptor, so
    mutual nearest neighbours join keypoints of different points and the track labelling merges their tracks.  A wrong match
    survives verification only where the other point happens to lie within 4 px of the epipolar line: a band of 8 px across
    points spread over some hundred pixels, a few per cent -- at most a quarter is asserted, and with the wrong matches at
    least half of the merged tracks go, while at least three quarters of the right matches stay."""
    import importlib.util
    import os
    from pixsfm_amd.api import DescriptorMatcher, TwoViewVerifier
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "match_verify_triangulate.py")
    spec = importlib.util.spec_from_file_location("match_verify_triangulate", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    rec, camera, names, kps, descs, owner, poses, n_twins = ex.make_scene(n_images=6, n_points=200, views=4, n_extra=20, seed=1)
    pairs = [(names[i], names[j]) for i in range(len(names)) for j in range(i + 1, len(names))]
    matches, scores = DescriptorMatcher.create("NN-mutual", ctx=ctx).match_pairs(descs, pairs)
    total0, wrong0, _, merged0, _, _ = ex.count(owner, pairs, matches, scores)
    assert n_twins == 40 and wrong0 >= 40 and merged0 >= 10
    for given in (None, poses):
        m, s, geoms = TwoViewVerifier.create({}, ctx=ctx).verify_pairs(kps, {n: camera for n in names}, pairs, matches, scores, poses=given)
        total1, wrong1, _, merged1, _, _ = ex.count(owner, pairs, m, s)
        print("wrong matches %d -> %d, merged tracks %d -> %d, right matches %d -> %d" % (wrong0, wrong1, merged0, merged1, total0 - wrong0, total1 - wrong1))
        assert 4 * wrong1 <= wrong0 and 2 * merged1 <= merged0 and 4 * (total1 - wrong1) >= 3 * (total0 - wrong0)
