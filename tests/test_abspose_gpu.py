"""GPU: the absolute-pose kernels (csrc/pxr_abspose.hip) against the numpy reference of tests/abspose_cases.py -- no query is
excused: the generated outliers sit at least 40 px from their true projection, so around the 12 px threshold there is a gap of
more than 25 px and every correct implementation ends at the generated inlier set."""
import numpy as np
import pytest

import abspose_cases as ac
import triangulation_cases as tc

pytestmark = pytest.mark.gpu


def _run(ctx, batch, qvec=None, tvec=None, timed=False, **options):
    from pixsfm_amd.engine import AbsolutePoseProblem
    prob = AbsolutePoseProblem(ctx, batch)
    out = prob.estimate(qvec=qvec, tvec=tvec, timed=timed, **options)
    names = ("qvec", "tvec", "status", "n_inliers", "n_trials", "inlier", "err")
    res = {k: a.download() for k, a in zip(names, out)}
    res["kernel_ms"] = prob.kernel_ms
    return res


@pytest.fixture(scope="module")
def boundary(ctx):
    batch, ref = ac.boundary_batch()
    return batch, ref, _run(ctx, batch)


def test_boundary_batch_equals_the_reference(boundary):
    """Measured on an MI355X: max rotation difference 6.8e-16 rad, max |dt|/|t| 3.7e-15, max pixel-error difference 1.8e-12 px."""
    batch, ref, got = boundary
    assert {0, 1}.issubset(set(ref["status"])) and len(ref["status"]) == 75
    assert np.array_equal(ref["inlier"].astype(bool), batch["true_inlier"] & np.repeat(ref["status"] == 0, np.diff(batch["query_offsets"])))
    ac.compare(got, ref, report="GPU vs reference: ")


def test_alone_equals_inside_the_batch_and_run_to_run(ctx, boundary):
    batch, _, got = boundary
    again = _run(ctx, batch, timed=True)
    for k in ("qvec", "tvec", "status", "n_inliers", "n_trials", "inlier", "err"):
        assert np.array_equal(again[k], got[k], equal_nan=True), k
    assert set(again["kernel_ms"]) == {"records", "compact", "hypotheses", "refine"} and all(v >= 0 for v in again["kernel_ms"].values())
    off = batch["query_offsets"]
    counts = np.diff(off)
    for n in (4, 65, 257, ac.LDS_CORR + 1, 2 * ac.LDS_CORR + 7):
        qi = int(np.flatnonzero(counts == n)[2])
        one = _run(ctx, ac.single(batch, qi))
        assert one["status"][0] == 0
        for k in ("qvec", "tvec", "status", "n_inliers", "n_trials"):
            assert np.array_equal(one[k][0], got[k][qi]), (n, k)
        assert np.array_equal(one["inlier"], got["inlier"][off[qi]:off[qi + 1]])
        assert np.array_equal(one["err"], got["err"][off[qi]:off[qi + 1]], equal_nan=True)


def test_every_status_code_and_untouched_sentinels(ctx):
    xy, X = ac.collinear_query()
    batch = ac.make_queries([3, len(xy), 40, 50], (1,), seed=5, p_outlier=0.0)
    off = batch["query_offsets"]
    batch["xy"][off[1]:off[2]], batch["xyz"][off[1]:off[2]] = xy, X
    batch["xy"][off[2]:off[3]] = np.random.default_rng(6).uniform(0, 900, (40, 2))        # all outliers
    sq, stv = np.arange(16.0).reshape(4, 4) - 50, np.arange(12.0).reshape(4, 3) - 70
    got = _run(ctx, batch, qvec=sq, tvec=stv, min_num_inliers=30)
    assert got["status"].tolist() == [1, 2, 3, 0] and got["n_inliers"].tolist() == [0, 0, 0, 50]
    assert np.array_equal(got["qvec"][:3], sq[:3]) and np.array_equal(got["tvec"][:3], stv[:3])
    assert not got["inlier"][:off[3]].any() and np.isnan(got["err"][:off[3]]).all() and got["inlier"][off[3]:].all()
    assert got["n_trials"].tolist() == [0, 4096, got["n_trials"][2], 64] and got["n_trials"][2] >= 64
    ref = ac.reference(batch, min_num_inliers=30)
    assert np.array_equal(ref["status"], got["status"]) and np.array_equal(ref["n_trials"], got["n_trials"])


def test_unusable_correspondences_leave_their_neighbours_alone(ctx):
    batch = ac.make_queries([40, 6, 120], (2, 8), seed=21, p_outlier=0.25)
    clean = _run(ctx, batch)
    assert (clean["status"] == 0).all()
    dirty = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in batch.items()}
    off = batch["query_offsets"]
    bad = [off[0] + 3, off[0] + 17, off[1] + 1, off[1] + 2, off[1] + 4, off[2] + 60]
    dirty["xy"][bad[0], 0] = np.nan
    dirty["xy"][bad[1]] = np.inf
    dirty["xyz"][bad[2], 2] = np.nan
    dirty["xy"][bad[3], 1] = -np.inf
    dirty["xyz"][bad[4]] = np.nan                               # query 1 keeps 3 usable correspondences: status 1
    dirty["xyz"][bad[5], 0] = np.inf
    got = _run(ctx, dirty)
    assert got["status"].tolist() == [0, 1, 0]
    assert not got["inlier"][bad].any() and np.isnan(got["err"][bad]).all()
    # the same queries with the unusable rows taken out give the same bits
    keep = np.ones(off[-1], bool)
    keep[bad] = False
    cut = dict(dirty, xy=dirty["xy"][keep], xyz=dirty["xyz"][keep],
               query_offsets=np.concatenate([[0], np.cumsum([keep[off[i]:off[i + 1]].sum() for i in range(3)])]).astype(np.int64))
    want = _run(ctx, cut)
    for k in ("qvec", "tvec", "status", "n_inliers", "n_trials"):
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    assert np.array_equal(got["inlier"][keep], want["inlier"]) and np.array_equal(got["err"][keep], want["err"], equal_nan=True)
    ref = ac.reference(dirty)
    ac.compare(got, ref, report="with unusable rows, GPU vs reference: ")


def test_invalid_arguments_are_refused(ctx):
    from pixsfm_amd import PixsfmHipError
    batch = ac.make_queries([10, 12, 9], (1, 2), seed=4, p_outlier=0.0)
    for change, word in ((dict(query_offsets=np.array([0, 22, 10, 31], np.int64)), "monotone"),
                         (dict(query_offsets=np.array([0, 10, 22, 30], np.int64)), "n_corr"),
                         (dict(query_offsets=np.array([1, 10, 22, 31], np.int64)), "not 0"),
                         (dict(query_camera=np.array([0, 2, 0], np.int32)), "camera"),
                         (dict(query_camera=np.array([0, -1, 0], np.int32)), "camera")):
        with pytest.raises(PixsfmHipError, match=word) as e:
            _run(ctx, dict(batch, **change))
        assert e.value.code == -1                               # PXR_EINVAL
    with pytest.raises(PixsfmHipError, match="option"):
        _run(ctx, batch, confidence=1.0)
    assert (_run(ctx, batch)["status"] == 0).all()              # the context is fine afterwards


def test_all_eleven_camera_models(ctx):
    """Every model's undistortion and refinement Jacobian: noise-free queries end at a zero-residual pose."""
    batch, gq, gt = ac.eleven_models_queries()
    models = batch["cam_model"]
    got = _run(ctx, batch)
    assert (got["status"] == 0).all() and (got["n_inliers"] == 40).all()
    print("largest error over the eleven models, noise-free: %.3e px" % got["err"].max())
    assert got["err"].max() <= 1e-6
    d = np.array([ac.pose_distance(gq[i], gt[i], got["qvec"][i], got["tvec"][i]) for i in range(len(models))])
    assert d.max() <= 1e-8


def test_hard_scene(ctx):
    """64 queries of 400 correspondences, 70 % outliers drawn uniformly with no shift: every query succeeds, the mask is the
    error test, contains every generated inlier, and the trials stay within the stop rule's count for w = 0.3 (421 -> 448).
    The last needs an all-inlier sample among the first 448.  All queries of one size share their sample triples, so that is a
    property of the data alone: with 448 x 0.3^3 = 12 expected it fails for about one query in 300, i.e. for one data seed in
    five; the seed used here is one for which every query has at least three (checked below from the hash, without the kernel)."""
    batch = ac.make_queries([400] * 64, (2, 1, 8), seed=42, p_outlier=0.7, min_outlier_shift=None)
    triples = np.array([ac.sample(0, h, 400) for h in range(448)])
    assert batch["true_inlier"].reshape(64, 400)[:, triples].all(2).sum(1).min() >= 3
    got = _run(ctx, batch)
    assert (got["status"] == 0).all()
    with np.errstate(invalid="ignore"):
        assert np.array_equal(got["inlier"].astype(bool), got["err"] <= 12.0)
    assert got["inlier"].astype(bool)[batch["true_inlier"]].all()
    assert (got["n_inliers"] >= 120).all()
    bound = int(np.ceil(ac.trials_needed(dict(ac.DEFAULTS), 4096, 120, 400) / 64)) * 64
    assert bound == 448 and got["n_trials"].max() <= bound and got["n_trials"].min() >= 64
    d = np.array([ac.pose_distance(batch["gt_qvec"][i], batch["gt_tvec"][i], got["qvec"][i], got["tvec"][i]) for i in range(64)])
    assert d[:, 0].max() < 5e-3


def test_api_shape_like_pycolmap(ctx):
    from pixsfm_amd.api import absolute_pose_estimation, absolute_pose_estimation_batch
    from pixsfm_amd.api.reconstruction import Camera
    batch = ac.make_queries([60, 80], (2, 1), seed=51, p_outlier=0.3)
    off = batch["query_offsets"]
    cams = [Camera(1, 2, 1000, 960, tc.MODEL_PARAMS[2]), Camera(2, 1, 1000, 960, tc.MODEL_PARAMS[1])]
    conf = {"ransac": {"max_error": 12}}
    one = absolute_pose_estimation(batch["xy"][:off[1]], list(batch["xyz"][:off[1]]), cams[0], estimation_options=conf,
                                   refinement_options={}, ctx=ctx)
    assert set(one) == {"success", "qvec", "tvec", "num_inliers", "inliers"} and one["success"] is True
    assert one["inliers"] == [bool(x) for x in batch["true_inlier"][:off[1]]] and one["num_inliers"] == sum(one["inliers"])
    assert one["qvec"].shape == (4,) and one["tvec"].shape == (3,) and one["qvec"].dtype == np.float64
    both = absolute_pose_estimation_batch([(batch["xy"][off[i]:off[i + 1]], batch["xyz"][off[i]:off[i + 1]], cams[i]) for i in range(2)],
                                          conf, None, ctx=ctx)
    assert np.array_equal(both[0]["qvec"], one["qvec"]) and np.array_equal(both[0]["tvec"], one["tvec"]) and both[0]["inliers"] == one["inliers"]
    assert both[1]["inliers"] == [bool(x) for x in batch["true_inlier"][off[1]:]]
    assert absolute_pose_estimation(batch["xy"][:3], batch["xyz"][:3], cams[0], ctx=ctx) == {"success": False}
    assert absolute_pose_estimation_batch([], ctx=ctx) == []
