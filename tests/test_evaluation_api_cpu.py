"""The host half of pixsfm_amd.api.evaluation: AUC and recall against results recorded from the reference's own functions
(tests/golden/eval_auc_cases.json: inputs and outputs only), pose errors against scipy's rotations, the robust similarity
alignment on a scene with known truth, the Sim3 algebra and PLY files."""
import json
import os

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

from pixsfm_amd.api import evaluation as ev
from pixsfm_amd.api.reconstruction import Image, Point3D, Reconstruction

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_auc_cases.json")
with open(GOLDEN) as _f:
    AUC_CASES = json.load(_f)


def _wxyz(rot):
    x, y, z, w = rot.as_quat()
    return np.array([w, x, y, z])


@pytest.mark.parametrize("case", AUC_CASES, ids=lambda c: "%s-%s" % (c["name"], c["min_error"]))
def test_auc_and_recall_equal_the_recorded_results(case):
    """1e-9 on the percent scale: a trapezoid sum of <= 1000 terms of magnitude <= 100 in double carries about 2e-11."""
    assert len(case["errors"]) <= 1000
    auc = ev.compute_auc(np.array(case["errors"]), case["thresholds"], min_error=case["min_error"])
    assert len(auc) == len(case["auc"])
    assert np.abs(np.array(auc) - np.array(case["auc"])).max() <= 1e-9, (auc, case["auc"])
    if "recall" in case:
        e, r = ev.compute_recall(np.array(case["errors"]))
        assert np.array_equal(e, np.array(case["sorted_errors"])) and np.abs(r - np.array(case["recall"])).max() <= 1e-15
    assert ev.compute_auc(list(case["errors"]), case["thresholds"], min_error=case["min_error"]) == auc      # a list is taken too


def test_the_recorded_cases_cover_what_they_should():
    names = {c["name"] for c in AUC_CASES}
    assert len(names) >= 12 and {c["min_error"] for c in AUC_CASES} == {None, 0.001, 0.02}
    by = {c["name"]: c for c in AUC_CASES if c["min_error"] is None}
    assert max(len(c["errors"]) for c in AUC_CASES) == 1000
    assert np.isinf(by["with_infinities"]["errors"]).any() and np.isinf(by["all_infinite"]["errors"]).all()
    assert min(by["all_above_largest"]["errors"]) > max(by["all_above_largest"]["thresholds"])
    assert max(by["all_below_min_error"]["errors"]) < 0.001
    assert len(set(by["ties"]["errors"])) < len(by["ties"]["errors"])


def test_pose_error_against_scipy():
    rng = np.random.default_rng(0)
    worst = 0.0
    for _ in range(50):
        Rg, Re = Rotation.random(random_state=rng), Rotation.random(random_state=rng)
        tg, te = rng.normal(0, 3, 3), rng.normal(0, 3, 3)
        dt, dR = ev.compute_pose_error(_wxyz(Rg), tg, {"success": True, "qvec": _wxyz(Re), "tvec": te})
        cg, ce = -Rg.as_matrix().T @ tg, -Re.as_matrix().T @ te
        assert abs(dt - np.linalg.norm(cg - ce)) <= 1e-12 * (1 + dt)
        angle = np.degrees((Rg * Re.inv()).magnitude())
        worst = max(worst, abs(dR - angle))
    assert worst <= 1e-6                                               # (arccos near 0 and 180 degrees loses half the digits)
    q = _wxyz(Rotation.random(random_state=rng))
    dt, dR = ev.compute_pose_error(q, [1.0, 2.0, 3.0], {"success": True, "qvec": -q, "tvec": [1.0, 2.0, 3.0]})
    assert dt <= 1e-15 and dR <= 1e-6
    assert ev.compute_pose_error(q, [0, 0, 0], {"success": False}) == (np.inf, 180)
    assert ev.compute_pose_error(q, [0, 0, 0], {"success": False, "qvec": q, "tvec": [0, 0, 0]}) == (np.inf, 180)


def _scene(n_images=40, outliers=0.3, seed=5):
    """Two reconstructions of the same cameras: `dst` = a known similarity of `src`, with a share of dst's centres grossly moved."""
    rng = np.random.default_rng(seed)
    src, dst = Reconstruction(), Reconstruction()
    rot = Rotation.from_rotvec([0.4, -0.9, 0.3])
    scale, R, t = 2.5, rot.as_matrix(), np.array([3.0, -1.0, 7.0])
    truth = ev.Sim3(scale, _wxyz(rot), t)
    bad = np.zeros(n_images, bool)
    bad[rng.permutation(n_images)[:int(round(outliers * n_images))]] = True
    for i in range(n_images):
        q = _wxyz(Rotation.random(random_state=rng))
        c = rng.uniform(-5, 5, 3)
        name = "im%03d.jpg" % i
        src.add_image(Image(i + 1, name, 1, q, -ev._rotmat(q) @ c))
        q2, t2 = truth.transform_pose(q, -ev._rotmat(q) @ c)
        if bad[i]:
            c2 = truth.transform_points(c) + rng.uniform(2.0, 6.0, 3) * rng.choice([-1, 1], 3)
            t2 = -ev._rotmat(q2) @ c2
        dst.add_image(Image(100 + i, name, 1, q2, t2))                 # (ids differ: images are paired by name)
    for k in range(20):
        x = rng.uniform(-4, 4, 3)
        src.add_point3D(k + 1, Point3D(x))
        dst.add_point3D(k + 1, Point3D(truth.transform_points(x)))
    return src, dst, truth, bad


def test_alignment_recovers_a_known_similarity_among_gross_outliers():
    """Scene size ~ 25 (centres in a 10-cube scaled by 2.5).  Largest deviations observed: scale 1.8e-16, rotation entries 1.1e-16,
    translation 5.3e-17 of the scene size -- the 1e-9 bound covers the conditioning of a 28-point fit a millionfold."""
    src, dst, truth, bad = _scene()
    out = ev.align_reconstructions(src, dst, max_error=0.05)
    assert out is not None
    sim, inliers = out
    assert inliers.dtype == bool and np.array_equal(inliers, ~bad)
    size = 25.0
    dev = (abs(sim.scale - truth.scale) / truth.scale, np.abs(sim.rotmat - truth.rotmat).max(), np.abs(sim.tvec - truth.tvec).max() / size)
    print("deviations: scale %.3g rotation %.3g translation %.3g" % dev)
    assert max(dev) <= 1e-9, dev
    again, inliers2 = ev.align_reconstructions(src, dst, max_error=0.05)        # the same call twice: the same bits
    assert again.scale == sim.scale and again.qvec.tobytes() == sim.qvec.tobytes() and again.tvec.tobytes() == sim.tvec.tobytes()
    assert np.array_equal(inliers2, inliers)
    # too many outliers for the ratio asked for
    assert ev.align_reconstructions(src, dst, max_error=0.05, min_inlier_ratio=0.8) is None
    # after the transform the inlier poses and all points agree
    cmp_ = ev.compare_reconstructions(src, dst, sim)
    assert cmp_["names"] == sorted(im.name for im in src.images.values())     # the order of the mask
    assert np.array_equal(inliers, cmp_["dt"] <= 0.05)                 # the mask is that of the transform returned
    assert cmp_["dt"][inliers].max() <= 1e-9 * size and cmp_["dt"][~inliers].min() > 1.0 and cmp_["dR"].max() <= 1e-5
    assert len(cmp_["point3D_ids"]) == 20 and cmp_["point_distances"].max() <= 1e-9 * size
    moved = sim.transform_reconstruction(src)
    same = ev.compare_reconstructions(moved, dst)
    assert np.abs(same["dt"] - cmp_["dt"]).max() <= 1e-9 * size and same["point_distances"].max() <= 1e-9 * size


def test_alignment_needs_three_common_images():
    src, dst, _, _ = _scene(n_images=6, outliers=0.0)
    for i in list(dst.images)[2:]:
        dst.images[i].name = "other_" + dst.images[i].name
    assert ev.align_reconstructions(src, dst, max_error=0.05) is None
    src, dst, truth, _ = _scene(n_images=5, outliers=0.0)            # few images: every triple is a hypothesis
    sim, inl = ev.align_reconstructions(src, dst, max_error=0.05)
    assert inl.all() and abs(sim.scale - truth.scale) <= 1e-9


def test_samples_are_distinct_and_reproducible():
    for n in (3, 4, 40):
        for h in range(64):
            s = ev._sample_three(0, h, n)
            assert len(set(s)) == 3 and s == tuple(sorted(s)) and 0 <= s[0] and s[2] < n and s == ev._sample_three(0, h, n)
    assert len({ev._sample_three(0, h, 40) for h in range(64)}) > 50


def test_sim3_inverse_round_trips():
    rng = np.random.default_rng(3)
    sim = ev.Sim3(0.37, _wxyz(Rotation.random(random_state=rng)), rng.normal(0, 5, 3))
    x = rng.normal(0, 10, (100, 3))
    back = sim.inverse().transform_points(sim.transform_points(x))
    assert np.abs(back - x).max() <= 1e-12 * 10
    inv2 = sim.inverse().inverse()
    assert abs(inv2.scale - sim.scale) <= 1e-15 and np.abs(inv2.rotmat - sim.rotmat).max() <= 1e-15 and np.abs(inv2.tvec - sim.tvec).max() <= 1e-14
    q = _wxyz(Rotation.random(random_state=rng))
    t = rng.normal(0, 2, 3)
    q2, t2 = sim.inverse().transform_pose(*sim.transform_pose(q, t))
    assert np.abs(ev._rotmat(q2) - ev._rotmat(q)).max() <= 1e-14 and np.abs(t2 - t).max() <= 1e-13


@pytest.mark.parametrize("binary", [True, False])
@pytest.mark.parametrize("colored", [True, False])
def test_ply_round_trip(tmp_path, binary, colored):
    rng = np.random.default_rng(1)
    xyz = np.concatenate([rng.normal(0, 30, (257, 3)), [[0.0, -0.0, 1e-30], [1e20, -1e-20, 3.0]]])
    rgb = rng.integers(0, 256, (len(xyz), 3)).astype(np.uint8) if colored else None
    path = str(tmp_path / "cloud.ply")
    ev.export_PLY(xyz, path, colors=rgb, binary=binary)
    with open(path, "rb") as f:
        head = f.read(200)
    assert head.startswith(b"ply\nformat " + (b"binary_little_endian" if binary else b"ascii") + b" 1.0\n")
    back, back_rgb = ev.read_ply_points(path, with_colors=True)
    assert np.array_equal(back.astype(np.float32), xyz.astype(np.float32)) and back.shape == xyz.shape
    assert (back_rgb is None) if not colored else np.array_equal(back_rgb, rgb)
    assert np.array_equal(ev.read_ply_points(path), back)


def test_ply_of_a_reconstruction_and_an_empty_cloud(tmp_path):
    rec = Reconstruction()
    for i, x in ((7, [1.0, 2.0, 3.0]), (2, [4.0, 5.0, 6.0])):
        rec.add_point3D(i, Point3D(x))
    path = str(tmp_path / "rec.ply")
    ev.export_PLY(rec, path)
    assert np.array_equal(ev.read_ply_points(path), [[4.0, 5.0, 6.0], [1.0, 2.0, 3.0]])     # ascending id
    ev.export_PLY(np.zeros((0, 3)), path)
    assert ev.read_ply_points(path).shape == (0, 3)


def test_public_names():
    import pixsfm_amd.api as api
    for name in ("evaluate_point_cloud", "compute_pose_error", "compute_recall", "compute_auc", "align_reconstructions", "Sim3",
                 "compare_reconstructions", "export_PLY", "read_ply_points", "evaluation"):
        assert hasattr(api, name), name
    from pixsfm_amd import engine
    assert callable(engine.cloud_nearest) and callable(engine.cloud_voxel_fractions)
