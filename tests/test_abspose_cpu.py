"""CPU: the numpy reference of the absolute-pose estimator (tests/abspose_cases.py) on generated queries, the sample hash,
the option parsing of api.localization.absolute_pose_estimation, the unique-inlier helpers against the reference's own
outputs (tests/golden/unique_inliers_ref.npz) and QueryLocalizer's configuration.  The kernels are held to the same
reference in tests/test_abspose_lanes_cpu.py (their source, lane by lane) and tests/test_abspose_gpu.py."""
import os

import numpy as np
import pytest

import abspose_cases as ac
import pxo
import triangulation_cases as tc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unique_inliers_ref.npz")


def test_numpy_camera_models_match_the_oracle():
    grid = tc.polar_grid(n_radii=5, n_angles=6, r_max=0.45)
    for m in (0, 1, 2, 3, 4, 8):
        k = np.array(tc.MODEL_PARAMS[m])
        x, y = ac.world_to_image(m, k, grid[:, 0], grid[:, 1])
        J = ac.camera_jacobian(m, k, grid[:, 0], grid[:, 1])
        for i, (u, v) in enumerate(grid):
            xy, Jo, _ = pxo.world_to_image(m, k, u, v)
            assert abs(x[i] - xy[0]) <= 1e-9 and abs(y[i] - xy[1]) <= 1e-9
            assert np.abs(J[i] - Jo[:2, :2]).max() <= 1e-8
        uv, ok = ac.image_to_world(m, k, np.stack([x, y], 1))
        assert ok.all() and np.abs(uv - grid).max() <= 1e-12
        for i in (3, 17):
            u, v, good, _ = tc.image_to_world(m, k, x[i], y[i])
            assert good and abs(u - uv[i, 0]) <= 1e-12 and abs(v - uv[i, 1]) <= 1e-12
    uv, ok = ac.image_to_world(2, np.array(tc.MODEL_PARAMS[2]), np.array([[np.nan, 3.0], [500.0, np.inf], [510.0, 470.0]]))
    assert ok.tolist() == [False, False, True] and np.isnan(uv[:2]).all()


def test_sample_hash_is_pinned_and_gives_distinct_triples():
    assert ac.mix(ac.G) == 0xE220A8397B1DCDAF                   # the first output of splitmix64 seeded with 0
    pins = [(0, 0, 4, (1, 2, 3)), (0, 1, 4, (0, 2, 3)), (0, 2, 5, (0, 1, 2)), (0, 63, 64, (3, 13, 48)), (0, 64, 65, (13, 16, 25)),
            (0, 4095, 1000, (33, 299, 463)), (1, 0, 4, (0, 1, 2)), (1, 7, 300, (61, 143, 161)), (12345, 100, 2055, (473, 1730, 1838)),
            (9223372036854775813, 3, 17, (3, 5, 8))]
    for seed, h, n, want in pins:
        assert ac.sample(seed, h, n) == want
    seen = set()
    for n in (4, 5, 7, 64, 1000):
        for h in range(300):
            s = ac.sample(0, h, n)
            assert len(set(s)) == 3 and 0 <= s[0] < s[1] < s[2] < n
            seen.add((n,) + s)
    assert len([s for s in seen if s[0] == 4]) == 4 and len([s for s in seen if s[0] == 1000]) >= 299      # all four triples of n = 4


def test_reference_recovers_the_generated_inliers():
    """200 queries, counts 4 .. 300, 0 .. 60 % outliers at least 40 px off, four camera models: the inlier set is the generated one
    for every query, no query excused."""
    rng = np.random.default_rng(7)
    counts = np.concatenate([[4, 5, 6, 7, 8, 300], rng.integers(4, 301, 194)])
    batch = ac.make_queries(counts, (1, 2, 4, 8), seed=8, p_outlier=rng.uniform(0.0, 0.6, len(counts)))
    ref = ac.reference(batch)
    assert (ref["status"] == 0).all()
    assert np.array_equal(ref["inlier"].astype(bool), batch["true_inlier"])
    assert np.array_equal(ref["n_inliers"], np.add.reduceat(batch["true_inlier"].astype(np.int32), batch["query_offsets"][:-1]))
    assert (ref["n_trials"] % 64 == 0).all() and ref["n_trials"].min() == 64 and ref["n_trials"].max() > 64
    d = np.array([ac.pose_distance(batch["gt_qvec"][i], batch["gt_tvec"][i], ref["qvec"][i], ref["tvec"][i]) for i in range(len(counts))])
    big = counts >= 30
    assert d[big, 0].max() < 5e-3 and np.median(d[big, 0]) < 5e-4          # half a pixel of noise at f = 1200: ~4e-4 rad per point


def test_noise_free_queries_are_solved_exactly():
    """A zero-residual problem, on which Gauss-Newton converges quadratically: every inlier's pixel error under the returned pose
    is <= 1e-6 px (measured: 1.0e-12 px)."""
    counts = [4, 5, 9, 30, 100, 300] * 4
    batch = ac.make_queries(counts, (1, 2, 4, 8), seed=9, sigma=0.0, p_outlier=0.3)
    ref = ac.reference(batch)
    assert (ref["status"] == 0).all() and np.array_equal(ref["inlier"].astype(bool), batch["true_inlier"])
    worst = ref["err"][batch["true_inlier"]].max()
    print("largest inlier error on noise-free queries: %.3e px" % worst)
    assert worst <= 1e-6
    d = np.array([ac.pose_distance(batch["gt_qvec"][i], batch["gt_tvec"][i], ref["qvec"][i], ref["tvec"][i]) for i in range(len(counts))])
    assert d.max() <= 1e-8


def test_reference_status_codes():
    xy, X = ac.collinear_query()
    r = ac.estimate(xy, X, 1, tc.MODEL_PARAMS[1])
    assert r["status"] == 2 and r["n_trials"] == 4096 and not r["inlier"].any() and np.isnan(r["err"]).all()
    r = ac.estimate(xy[:3], X[:3], 1, tc.MODEL_PARAMS[1])
    assert r["status"] == 1 and r["n_trials"] == 0
    b = ac.make_queries([40], (1,), seed=5, p_outlier=0.0)
    r = ac.estimate(np.random.default_rng(6).uniform(0, 900, (40, 2)), b["xyz"], 1, tc.MODEL_PARAMS[1], min_num_inliers=30)
    assert r["status"] == 3 and r["n_inliers"] == 0 and not r["inlier"].any()
    # the stop rule: w = 1 asks for min_num_trials, w = 0.3 for 421 -> 448 samples
    o = dict(ac.DEFAULTS)
    assert ac.trials_needed(o, 4096, 10, 10) == 64 and ac.trials_needed(o, 4096, 0, 10) == 4096
    assert int(np.ceil(ac.trials_needed(o, 4096, 30, 100) / 64)) * 64 == 448


def test_option_parsing():
    from pixsfm_amd.api import localization as loc
    from pixsfm_amd.engine import abspose_options
    o = abspose_options()
    assert (o.max_error, o.min_inlier_ratio, o.min_num_inliers, o.confidence) == (12.0, 0.01, 4, 0.99999)
    assert (o.min_num_trials, o.max_num_trials, o.round_size, o.seed) == (64, 4096, 64, 0)
    assert (o.refine_max_iterations, o.refine_loss_scale, o.lo_rounds) == (100, 1.0, 4)
    for k, v in ac.DEFAULTS.items():
        assert getattr(o, k) == v
    kw = loc.abspose_engine_options({"ransac": {"max_error": 8, "min_inlier_ratio": 0.1, "confidence": 0.99, "min_num_trials": 128,
                                                "max_num_trials": 1000}}, {"max_num_iterations": 50, "loss_function_scale": 2.0})
    assert kw == dict(max_error=8, min_inlier_ratio=0.1, confidence=0.99, min_num_trials=128, max_num_trials=1000,
                      refine_max_iterations=50, refine_loss_scale=2.0)
    assert abspose_options(**kw).refine_loss_scale == 2.0
    assert loc.abspose_engine_options(None, None) == {} and loc.abspose_engine_options({"ransac": {}}, {"print_summary": False}) == {}
    for est, ref in (({"ransac": {"max_err": 3}}, None), ({"ransack": {}}, None), (None, {"max_iterations": 3})):
        with pytest.raises(ValueError, match="unknown"):
            loc.abspose_engine_options(est, ref)
    for est, ref in ((None, {"refine_focal_length": True}), (None, {"refine_extra_params": True}), ({"estimate_focal_length": True}, None)):
        with pytest.raises(NotImplementedError, match="QBA"):
            loc.abspose_engine_options(est, ref)
    assert loc.abspose_engine_options(None, {"refine_focal_length": False}) == {}


def test_unique_inlier_helpers_match_the_reference():
    from pixsfm_amd.api import find_unique_inliers, find_unique_min_by_group
    g = np.load(GOLDEN)
    names = sorted(k[:-5] for k in g.files if k.endswith("_idxs"))
    assert len(names) == 26
    ties = 0
    for name in names:
        idxs, errors, pre = g[name + "_idxs"], g[name + "_errors"], g[name + "_pre"]
        pre = None if len(pre) == 0 else [bool(x) for x in pre]
        got = find_unique_inliers([int(v) for v in idxs], pre_inliers=pre)
        assert isinstance(got, list) and got == [bool(x) for x in g[name + "_unique"]], name
        got = find_unique_min_by_group([float(e) for e in errors], [int(v) for v in idxs], pre_inliers=pre)
        assert isinstance(got, list) and got == [bool(x) for x in g[name + "_min"]], name
        ties += len(errors) - len(set(zip(idxs.tolist(), errors.tolist())))
    assert ties > 50                                           # equal errors inside a group are part of the data
    assert find_unique_inliers([]) == [] and find_unique_min_by_group([], []) == []


def test_reprojection_errors_and_min_reproj_inliers():
    from pixsfm_amd import synthetic
    from pixsfm_amd.api import compute_reprojection_errors, find_unique_min_reproj_inliers
    from pixsfm_amd.api.reconstruction import Camera, Point3D, Reconstruction
    rng = np.random.default_rng(3)
    q, t = ac.random_pose(rng)
    for m in (0, 1, 2, 3, 4):
        cam = Camera(1, m, 1000, 960, tc.MODEL_PARAMS[m])
        X = (np.concatenate([rng.uniform(-0.3, 0.3, (12, 2)), np.ones((12, 1))], 1) * rng.uniform(2, 9, (12, 1)) - t) @ synthetic.qvec_to_rotmat(q)
        p2D = np.array([pxo.world_to_pixel(m, np.array(tc.MODEL_PARAMS[m]), q, t, x, jac=False)[0] for x in X])
        shift = rng.normal(0, 2, (12, 2))
        err = compute_reprojection_errors(p2D + shift, list(X), q, t, cam)
        assert isinstance(err, list) and np.abs(np.array(err) - np.linalg.norm(shift, axis=1)).max() <= 1e-9
    rec = Reconstruction()
    for i, x in enumerate(X):
        rec.add_point3D(10 + i, Point3D(x))
    ids = [10, 10, 11, 12, 12, 13]                              # points 10 and 12 are matched twice; keypoint 5 is used twice
    kp_idx = [0, 1, 2, 3, 4, 2]
    off = np.array([3.0, 1.0, 2.0, 0.5, 4.0, 1.0])
    pts = p2D[[0, 0, 1, 2, 2, 3]] + off[:, None] * [1.0, 0.0]
    got = find_unique_min_reproj_inliers(ids, q, t, cam, pts, rec, pre_inliers=[True] * 6, point2D_idxs=kp_idx)
    assert got == [False, True, False, True, False, True]      # per point: 1, 2, 3, 5; per keypoint: 5 (error 1) beats 2 (error 2)
    assert find_unique_min_reproj_inliers(ids, q, t, cam, pts, rec, pre_inliers=[True, False, True, True, True, True]) == \
        [True, False, True, True, False, True]


def test_query_localizer_configuration():
    from pixsfm_amd.api import QueryBundleAdjuster, QueryKeypointAdjuster, QueryLocalizer, base
    from pixsfm_amd.api.reconstruction import Reconstruction
    d = QueryLocalizer.default_conf
    assert d["target_reference"] == "nearest" and d["unique_inliers"] == "min_error" and d["max_tracks_per_problem"] == 50
    assert d["overwrite_features_sparse"] is None and d["interpolation"] == base.interpolation_default_conf
    assert d["references"] == {"loss": {"name": "cauchy", "params": [0.25]}, "iters": 100, "keep_observations": True,
                               "compute_offsets3D": False, "num_threads": -1}
    assert d["PnP"] == {"estimation": {"ransac": {"max_error": 12}}, "refinement": {}}
    assert {k: v for k, v in d["QKA"].items() if k != "interpolation"} == \
        {k: v for k, v in QueryKeypointAdjuster.default_conf.items() if k != "interpolation"}
    assert {k: v for k, v in d["QBA"].items() if k != "interpolation"} == \
        {k: v for k, v in QueryBundleAdjuster.default_conf.items() if k != "interpolation"}
    assert d["dense_features"]["patch_size"] == 16 and d["dense_features"]["sparse"] is True
    rec = Reconstruction()
    loc = QueryLocalizer(rec, {"interpolation": {"l2_normalize": False}, "PnP": {"estimation": {"ransac": {"confidence": 0.999}}},
                               "QBA": {"apply": False}}, references=[{}])
    assert loc.conf["QKA"]["interpolation"]["l2_normalize"] is False and loc.conf["QBA"]["interpolation"]["l2_normalize"] is False
    assert loc.conf["PnP"]["estimation"]["ransac"] == {"max_error": 12, "confidence": 0.999} and loc.conf["QBA"]["apply"] is False
    assert QueryLocalizer(rec, {"localization": {"unique_inliers": None}}, references=[{}]).conf["unique_inliers"] is None
    with pytest.raises(ValueError, match="dense_features"):
        QueryLocalizer(rec)                                     # neither references nor map features
    with pytest.raises(ValueError, match="unknown"):
        QueryLocalizer(rec, {"target_references": "nearest"}, references=[{}])
    with pytest.raises(ValueError, match="target_reference"):
        QueryLocalizer(rec, {"target_reference": "closest"}, references=[{}])
    with pytest.raises(ValueError, match="Stacked QKA"):
        QueryLocalizer(rec, {"target_reference": "all_observations", "QKA": {"stack_correspondences": True}}, references=[{}])
    with pytest.raises(NotImplementedError, match="QBA"):
        QueryLocalizer(rec, {"PnP": {"refinement": {"refine_focal_length": True}}}, references=[{}])
    with pytest.raises(NotImplementedError, match="patch-warp"):
        QueryLocalizer(rec, {"target_reference": "full"}, references=[{}]).get_query_references([1], None, None, None)
    assert QueryLocalizer(rec, {"QKA": {"apply": False}, "QBA": {"apply": False}}).localize(np.zeros((0, 2)), [], [], None) == {"success": False}
