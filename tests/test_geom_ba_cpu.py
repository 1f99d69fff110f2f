"""CPU: the host side of the geometric bundle adjustment (strategy "geometric") -- configuration, the shim's class, the flat
problem GeometricBundleOptimizer::AddResiduals would add (geometric_bundle_optimizer.h:39-88), the rank share of the
keypoints, and the ramp-patch bridge (tests/geom_cases.py) the GPU tests lean on.  No Context is created here."""
import json
import os

import numpy as np
import pytest

import geom_cases
from pixsfm_amd.api import (BundleAdjuster, BundleAdjustmentSetup, GeometricBundleAdjuster, GeometricBundleOptimizer)
from pixsfm_amd.api.bundle_adjustment import _FlatBA, _geometric_dict, _rank_share
from pixsfm_amd.api.reconstruction import Camera, Image, Point2D, Point3D, Reconstruction, Track, TrackElement, reconstruction_from_flat

HERE = os.path.dirname(os.path.abspath(__file__))


def test_create_returns_the_geometric_adjuster_with_the_references_defaults():
    from test_api_defaults_golden import _diff
    adj = BundleAdjuster.create({"strategy": "geometric"})
    assert type(adj) is GeometricBundleAdjuster
    ref = json.load(open(os.path.join(HERE, "golden", "default_conf_ref.json")))["BundleAdjuster"]   # main.py:294: a deepcopy of it
    assert not _diff(ref, GeometricBundleAdjuster.default_conf, "GeometricBundleAdjuster")
    want = dict(ref, strategy="geometric")
    assert not _diff(want, adj.conf, "conf")
    assert adj.conf["optimizer"]["solver"]["use_inner_iterations"] is True
    tuned = BundleAdjuster.create({"strategy": "geometric", "optimizer": {"loss": {"name": "huber", "params": [1.0]}}})
    assert tuned.conf["optimizer"]["loss"] == {"name": "huber", "params": [1.0]}
    assert GeometricBundleAdjuster.default_conf["optimizer"]["loss"] == {"name": "cauchy", "params": [0.25]}   # untouched


def test_unknown_options_are_refused_and_the_refusal_names_the_strategies():
    with pytest.raises(ValueError):
        BundleAdjuster.create({"strategy": "geometric", "optimizer": {"no_such_option": 1}})
    with pytest.raises(ValueError):
        GeometricBundleOptimizer({"no_such_option": 1}, BundleAdjustmentSetup())
    with pytest.raises(ValueError):
        GeometricBundleOptimizer({}, None)                                   # a setup is required
    with pytest.raises(ValueError, match="geometric"):
        BundleAdjuster.create({"strategy": "no_such_strategy"})


def test_shim_exports_the_real_class_with_the_bound_names():
    import pixsfm_amd._pixsfm as shim
    cls = shim._bundle_adjustment.GeometricBundleOptimizer
    assert cls is GeometricBundleOptimizer
    bound = json.load(open(os.path.join(HERE, "golden", "shim_bindings_ref.json")))["_bundle_adjustment"]["classes"]["GeometricBundleOptimizer"]
    assert sorted(bound) == ["problem", "reset", "run", "set_up", "solve_problem", "summary"]
    for name in bound:
        assert hasattr(cls, name), name
    opt = cls({}, BundleAdjustmentSetup())                                    # constructible: (options, setup), bindings.cc:155-157
    assert opt.summary() is None
    with pytest.raises(ValueError):
        opt.solve_problem(None)                                               # before set_up


def _toy():
    """3 images of one SIMPLE_PINHOLE camera, 3 points; image 1 carries a point2D without a 3D point."""
    rec = Reconstruction()
    rec.add_camera(Camera(1, "SIMPLE_PINHOLE", 100, 100, [100.0, 50.0, 50.0]))
    xy = {1: [((1., 2.), 10), ((3., 4.), 11), ((5., 6.), -1)],
          2: [((7., 8.), 10), ((9., 10.), 12), ((11., 12.), 11)],
          3: [((13., 14.), 10), ((15., 16.), 12)]}
    for i in (1, 2, 3):
        rec.add_image(Image(i, "im%d.jpg" % i, 1, [1.0, 0, 0, 0], [0.1 * i, 0.0, 0.0], [Point2D(p, pid) for p, pid in xy[i]]))
    tracks = {10: [(1, 0), (2, 0), (3, 0)], 11: [(1, 1), (2, 2)], 12: [(2, 1), (3, 1)]}
    for pid, els in tracks.items():
        rec.add_point3D(pid, Point3D([0.1 * (pid - 10), 0.0, 5.0], Track([TrackElement(a, b) for a, b in els])))
    return rec


def test_flat_problem_lists_the_observations_add_residuals_would():
    rec = _toy()
    setup = BundleAdjustmentSetup()
    setup.add_images([1, 2])
    setup.set_constant_pose(1)
    flat = _FlatBA(rec, setup, None, {})
    # images 1 and 2 only; point-major, inside a point in track order; the point2D without a 3D point adds nothing
    assert flat.obs_keys == [(1, 0), (2, 0), (1, 1), (2, 2), (2, 1)]
    assert flat.obs_xy.tolist() == [[1, 2], [7, 8], [3, 4], [11, 12], [9, 10]]
    assert flat.image_ids == [1, 2] and flat.pose_const.tolist() == [1, 0]
    assert flat.point_ids == [10, 11, 12] and flat.point_const.tolist() == [1, 0, 1]     # seen from outside the setup: constant
    # ... unless they are variable points: the observations from image 3 come back, with a constant pose
    setup.add_variable_point(10)
    setup.add_variable_point(12)
    flat = _FlatBA(rec, setup, None, {})
    assert flat.obs_keys == [(1, 0), (2, 0), (3, 0), (1, 1), (2, 2), (2, 1), (3, 1)]
    assert flat.obs_xy.tolist() == [[1, 2], [7, 8], [13, 14], [3, 4], [11, 12], [9, 10], [15, 16]]
    assert flat.image_ids == [1, 2, 3] and flat.pose_const.tolist() == [1, 0, 1] and flat.outside_images == {3}
    assert not flat.point_const.any()
    d = _geometric_dict(flat)
    assert "obs_patch" not in d and "refs" not in d and d["obs_xy"].shape == (7, 2)
    assert np.array_equal(d["obs_image"], [0, 1, 2, 0, 1, 1, 2]) and np.array_equal(d["obs_point"], [0, 0, 0, 1, 1, 2, 2])
    # refine_extrinsics = False: every pose constant
    flat = _FlatBA(rec, setup, None, {"refine_extrinsics": False})
    assert flat.pose_const.tolist() == [1, 1, 1]


@pytest.mark.parametrize("world", [2, 3, 8])
def test_rank_share_slices_the_keypoints_with_their_observations(world):
    from pixsfm_amd import synthetic
    prob = synthetic.make_ba_problem(n_cams=5, n_points=23, obs_per_point=3, seed=4, channels=1, patch_size=2, dtype=np.float64)
    prob["centers"] = prob["centers"] + np.random.default_rng(0).normal(0, 0.5, prob["centers"].shape)
    rec, _ = reconstruction_from_flat(prob)
    setup = BundleAdjustmentSetup()
    setup.add_images(rec.reg_image_ids())
    flat = _FlatBA(rec, setup, None, {})
    all_xy = flat.obs_xy
    assert np.array_equal(all_xy, prob["centers"])                         # reconstruction_from_flat keeps the observation order
    seen = np.zeros(len(all_xy), bool)
    for rank in range(world):
        share = _rank_share(flat, rank, world)
        d = share.geometric_dict()
        assert np.array_equal(d["obs_xy"], all_xy[share.obs])
        assert np.array_equal(d["obs_image"], flat.obs_image[share.obs])
        assert np.array_equal(flat.obs_point[share.obs] - share.lo, d["obs_point"])
        assert len(d["xyz"]) == len(share.point_ids) and not seen[share.obs].any()
        seen[share.obs] = True
    assert seen.all()


@pytest.mark.parametrize("model,tracks", [(2, 2), (0, 4), (4, 9)])
@pytest.mark.parametrize("float_simd", [False, True])
def test_ramp_patches_turn_the_oracle_into_a_reprojection_cost(model, tracks, float_simd):
    """The bridge itself: pxo.ba_eval_batch on the ramp problem against pxo.world_to_pixel - xy (<= 1e-12 px; measured 0.0),
    so that a broken helper cannot silently weaken the GPU tests that compare with the oracle."""
    import pxo
    prob = geom_cases.make_case(n_cams=max(6, tracks), n_points=30, obs_per_point=tracks, seed=7 + model, model=model)
    want = geom_cases.reprojection(prob) - prob["obs_xy"]
    cost, r, _ = pxo.ba_eval_batch(prob, pxo.cfg(l2_normalize=False, use_float_simd=float_simd), pxo.loss("cauchy", 1.0), want_r=True)
    assert r.shape == want.shape and np.abs(r - want).max() <= 1e-12
    assert abs(cost - geom_cases.robust_cost(prob, ("cauchy", 1.0))) <= 1e-13 * cost
    assert np.hypot(want[:, 0], want[:, 1]).max() > 1.0                    # the case is not trivially at its optimum
    # three channels (what pxr_ba_eval accepts): the third is zero
    prob3 = geom_cases.as_ramp_problem(prob, prob["obs_xy"], channels=3)
    _, r3, _ = pxo.ba_eval_batch(prob3, pxo.cfg(l2_normalize=False), pxo.loss("cauchy", 1.0), want_r=True)
    assert np.abs(r3[:, :2] - want).max() <= 1e-12 and not r3[:, 2].any()


def test_a_case_outside_the_linear_zone_is_reported_as_broken():
    prob = geom_cases.make_case(n_cams=6, n_points=10, obs_per_point=3, seed=1)
    far = prob["obs_xy"].copy()
    far[0] += 40.0
    with pytest.raises(AssertionError, match="broken case"):
        geom_cases.assert_inside(dict(prob, obs_xy=far))
