"""GPU: QueryLocalizer.localize(..., return_covariance=True) on the scene of examples/localize_query.py at a small size."""
import importlib.util
import os
from copy import deepcopy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _example():
    spec = importlib.util.spec_from_file_location("localize_query_example", os.path.join(ROOT, "examples", "localize_query.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def scene():
    return _example().make_scene(n_images=5, n_points=60)


def test_localizer_returns_the_pose_covariance(ctx, scene):
    from pixsfm_amd.api import BundleAdjustmentSetup, QueryLocalizer, estimate_ba_covariance, features
    from pixsfm_amd.api.reconstruction import Image, Point2D, Point3D, Reconstruction, Track, TrackElement
    rec, manager, keypoints, kp_idx, p3d_id, fmap, camera, _, _ = scene
    localizer = QueryLocalizer(rec, None, dense_features=manager)
    plain = localizer.localize(keypoints, kp_idx, p3d_id, deepcopy(camera), query_fmaps=[fmap])
    cam = deepcopy(camera)
    pose = localizer.localize(keypoints, kp_idx, p3d_id, cam, query_fmaps=[fmap], return_covariance=True)
    assert plain["success"] and pose["success"]
    # without the flag the result is what it was; with it, one more key
    assert sorted(plain) == ["inliers", "num_inliers", "qvec", "success", "tvec"]
    assert sorted(pose) == sorted(list(plain) + ["covariance"])
    assert np.array_equal(plain["qvec"], pose["qvec"]) and np.array_equal(plain["tvec"], pose["tvec"])
    cov = pose["covariance"]
    assert cov.shape == (6, 6) and np.array_equal(cov, cov.T)
    assert np.linalg.eigvalsh(cov)[0] > 0.0
    print("sigma: rotation %s rad, translation %s" % (np.sqrt(np.diag(cov)[:3]), np.sqrt(np.diag(cov)[3:])))

    # the same QBA problem as a one-image reconstruction with every point constant, through estimate_ba_covariance
    inliers = localizer.last_qba_inliers
    refs = localizer.get_query_references(p3d_id, [fmap], np.array(keypoints)[kp_idx], kp_idx)[-1]
    points2D = [Point2D(xy) for xy in keypoints]
    one = Reconstruction()
    one.add_camera(cam)
    references, setup = {}, BundleAdjustmentSetup()
    for i, ok in enumerate(inliers):
        if not ok:
            continue
        assert not points2D[kp_idx[i]].has_point3D() and p3d_id[i] not in references       # unique pairs
        points2D[kp_idx[i]].point3D_id = p3d_id[i]
        one.add_point3D(p3d_id[i], Point3D(rec.points3D[p3d_id[i]].xyz, Track([TrackElement(1, kp_idx[i])])))
        references[p3d_id[i]] = features.Reference(1, kp_idx[i], np.asarray(refs[i]))
    one.add_image(Image(1, "query", cam.camera_id, pose["qvec"], pose["tvec"], points2D))
    setup.add_image(1)
    for pid in references:
        setup.add_constant_point(pid)
    qba = localizer.conf["QBA"]
    conf = {"strategy": "feature_reference", "interpolation": qba["interpolation"],
            "optimizer": {"loss": qba["optimizer"]["loss"], "refine_focal_length": False, "refine_principal_point": False,
                          "refine_extra_params": False}}
    est = estimate_ba_covariance(conf, one, setup, features.FeatureSet({"query": fmap}), references)
    want = est.pose_cov(1)
    print("localizer against estimate_ba_covariance: max relative difference %.3g" % (np.abs(cov - want).max() / np.abs(want).max()))
    assert est.summary["num_camera_unknowns"] == 6
    assert np.allclose(cov, want, rtol=1e-9, atol=1e-12 * np.abs(want).max())
    assert not est.point_cov(next(iter(references))).any()          # a constant point
