"""GPU: evaluate_point_cloud against the brute-force statement of tests/cloud_cases.py with exact equality, and the core of
examples/evaluate_reconstruction.py on a small scene."""
import os
import sys

import numpy as np
import pytest

import cloud_cases as cc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = (0.01, 0.02, 0.05)


@pytest.fixture(scope="module")
def plane_case():
    """A 20 000-point plane "scan" and a 2 000-point model on it, half of the model displaced by 3 cm along the normal."""
    rng = np.random.default_rng(11)
    scan = np.concatenate([rng.uniform(0, 1, (20000, 2)), np.zeros((20000, 1))], axis=1)
    model = np.concatenate([rng.uniform(0.02, 0.98, (2000, 2)), np.zeros((2000, 1))], axis=1)
    model[1000:, 2] = 0.03
    expected = {}
    for name, (query, ref) in (("accuracy", (model, scan)), ("completeness", (scan, model))):
        _, d2 = cc.nearest(ref, query, max(TOL))
        expected[name] = cc.voxel_fractions(query, d2, 0.01, TOL)
    return scan, model, expected


def test_accuracy_and_completeness_equal_the_reference(ctx, plane_case):
    from pixsfm_amd.api import evaluate_point_cloud
    scan, model, expected = plane_case
    out = evaluate_point_cloud(model, scan, ctx=ctx)
    assert out["tolerances"] == list(TOL)
    assert out["accuracy"] == list(expected["accuracy"][0]) and out["completeness"] == list(expected["completeness"][0])
    assert out["n_voxels"] == (expected["accuracy"][1], expected["completeness"][1])
    # the displaced half is 3 cm away: outside 1 and 2 cm, inside 5 cm
    assert 0.4 < out["accuracy"][0] < 0.6 and 0.4 < out["accuracy"][1] < 0.6 and out["accuracy"][2] == 1.0
    assert 0 < out["completeness"][0] < out["completeness"][1] < out["completeness"][2] <= 1.0
    plain = evaluate_point_cloud(model, scan, voxel_size=0, ctx=ctx)   # over the points: exactly the counts
    _, d2 = cc.nearest(scan, model, max(TOL))
    assert plain["accuracy"] == [float((d2 <= t * t).sum()) / 2000.0 for t in TOL] and plain["n_voxels"] == (2000, 20000)


def test_a_reconstruction_gives_the_result_of_its_points(ctx, plane_case):
    from pixsfm_amd.api import evaluate_point_cloud
    from pixsfm_amd.api.reconstruction import Point3D, Reconstruction
    scan, model, _ = plane_case
    rec = Reconstruction()
    ids = np.random.default_rng(0).permutation(len(model)) + 5         # (inserted out of order: taken in ascending id)
    for i in np.argsort(-ids):
        rec.add_point3D(int(ids[i]), Point3D(model[i]))
    d_scan = ctx.to_device(scan, np.float64)
    a = evaluate_point_cloud(rec, d_scan, ctx=ctx)
    b = evaluate_point_cloud(model[np.argsort(ids)], d_scan, ctx=ctx)
    c = evaluate_point_cloud(model, scan, ctx=ctx)
    assert a == b and a == c                                           # (and the order of the points does not matter)


def test_the_example_on_eight_images(ctx):
    """The example's mapper stops each of its own adjustments after one iteration, so the bundle adjustment that follows starts
    from poses that are not converged and has to improve them: at every threshold its pose AUC is not below the mapper's.
    Measured on an MI355X: mapper 39.904 / 70.035 / 88.014 / 94.007, adjusted 40.038 / 70.177 / 88.071 / 94.035."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import evaluate_reconstruction as ex
    res = ex.run(n_images=8, n_points=300, scan_step=0.01)
    assert res["summary"]["num_reg_images"] >= 6, res["summary"]
    before, after = res["mapper"], res["adjusted"]
    assert before is not None and after is not None
    print("pose AUC before %r after %r; accuracy before %s after %s" % (before["auc"], after["auc"], before["cloud"]["accuracy"],
                                                                        after["cloud"]["accuracy"]))
    assert before["inliers"] == res["summary"]["num_reg_images"] == after["inliers"]
    for a, b in zip(after["auc"], before["auc"]):
        assert a >= b, (after["auc"], before["auc"])
    assert after["auc"][-1] > 50.0 and after["dR"].max() < 1.0
    assert after["cloud"]["accuracy"][2] > 0.8 and 0 < after["cloud"]["completeness"][2] < 0.5
