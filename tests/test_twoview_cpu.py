"""CPU: the numpy reference of the two-view estimator (tests/twoview_cases.py) against independent checks -- numpy.roots, the
essential-matrix constraints, the generating poses, finite differences -- and the Python API with the reference in the kernel's
place.  The kernels themselves are held to this reference by tests/test_twoview_lanes_cpu.py and tests/test_twoview_gpu.py."""
import numpy as np
import pytest

import triangulation_cases as tc
import twoview_cases as tv
from pixsfm_amd import synthetic

# 100 x the largest deviations measured over the 256 noise-free samples of test_five_point_solver (written in its docstring)
ROOT_TOL = 100 * 1.9e-9
CONSTRAINT_TOL = 100 * 6.0e-16
# The bound of tests/test_minimal_solvers_cpu.py is C kappa u per solution with C = 600 for this solver, and a solution is
# well-conditioned while that stays within 1e-7 (minimal_solver_ref.CAP): the cap is the tolerance here, where kappa is not
# computed.  (That test measures kappa on the same generator: at most 2e4 over 64 samples, so the bound there is below 2e-9.)
TRUE_E_TOL = 1e-7


def test_sample_hash():
    for n in (5, 6, 300):
        for h in range(50):
            s = tv.sample(0, h, n)
            assert len(set(s)) == 5 and list(s) == sorted(s) and 0 <= s[0] and s[4] < n
    assert tv.sample(0, 3, 300) != tv.sample(1, 3, 300) and tv.sample(0, 3, 300) == tv.sample(0, 3, 300)


def test_five_point_solver():
    """256 random noise-free samples.  Measured: largest deviation of the polynomial's roots from numpy.roots 1.84e-9 (relative to
    1 + |z|), largest constraint residual 4.15e-16 (relative to |E|^3), largest distance of the true E from the nearest solution
    4.0e-12 (unit Frobenius norm).  Before the hypotheses were polished on the cubic constraints the last two were 3.95e-6 and
    6.83e-5: that was the arithmetic of the elimination to det B(z), not the problem's conditioning -- kappa u is at most 2e-12
    on this generator (tests/test_minimal_solvers_cpu.py), and the unpolished solver missed it by a factor of up to 6e7."""
    rec, Rs, ts = tv.noise_free_samples(256, seed=1)
    E, valid, det = tv.five_point(rec, details=True)
    assert det["ok"].all() and not np.isnan(E[valid]).any()
    worst = np.zeros(3)
    for b in range(len(rec)):
        nr = np.roots(det["c"][b][::-1])
        nr = np.sort(nr[np.abs(nr.imag) <= 1e-7 * (1 + np.abs(nr.real))].real)
        assert len(nr) == det["n_roots"][b]
        z = det["roots"][b, :len(nr)]
        assert (np.diff(z) >= 0).all()
        worst[0] = max(worst[0], np.abs((z - nr) / (1 + np.abs(nr))).max())
        Et = tv.essential_of_pose(Rs[b], ts[b])
        Et /= np.linalg.norm(Et)
        near = np.inf
        for k in np.flatnonzero(valid[b]):
            M = E[b, k].reshape(3, 3)
            n3 = np.linalg.norm(M) ** 3
            worst[1] = max(worst[1], abs(np.linalg.det(M)) / n3, np.abs(2 * M @ M.T @ M - np.trace(M @ M.T) * M).max() / n3)
            Mn = M / np.linalg.norm(M)
            near = min(near, np.linalg.norm(Mn - Et), np.linalg.norm(Mn + Et))
        worst[2] = max(worst[2], near)
    print("roots %.3e, constraints %.3e, true E %.3e" % tuple(worst))
    assert worst[0] <= ROOT_TOL and worst[1] <= CONSTRAINT_TOL and worst[2] <= TRUE_E_TOL


def test_degenerate_samples_give_no_hypothesis_and_no_nan():
    rng = np.random.default_rng(2)
    one = rng.uniform(-0.3, 0.3, 4)
    coincident = np.tile(one, (5, 1))
    s = np.linspace(-1, 1, 5)[:, None]
    collinear = np.concatenate([np.array([0.1, -0.2]) + s * np.array([0.3, 0.1]), np.array([-0.1, 0.05]) + s * np.array([0.2, -0.25])], 1)
    E, valid = tv.five_point(np.stack([coincident, collinear]))
    assert not valid.any() and not np.isnan(E).any()


def test_horn_returns_the_generating_pose():
    rng = np.random.default_rng(3)
    for _ in range(50):
        q, t = tv.random_relative_pose(rng)
        R, t = synthetic.qvec_to_rotmat(q), t / np.linalg.norm(t)
        tt, Ra, Rb = tv.horn(rng.uniform(0.5, 3.0) * rng.choice([-1.0, 1.0]) * tv.essential_of_pose(R, t))
        poses = [(Ra, tt), (Ra, -tt), (Rb, tt), (Rb, -tt)]
        assert min(max(np.abs(Rx - R).max(), np.abs(tx - t).max()) for Rx, tx in poses) <= 1e-13
        for Rx in (Ra, Rb):
            assert np.abs(Rx @ Rx.T - np.eye(3)).max() <= 1e-13 and abs(np.linalg.det(Rx) - 1) <= 1e-13
        # the generating pose is the one that sees the points in front of both cameras
        x1 = rng.uniform(-0.3, 0.3, (20, 2))
        X2 = (np.concatenate([x1, np.ones((20, 1))], 1) * rng.uniform(2, 12, (20, 1))) @ R.T + 2.0 * t
        rec = np.concatenate([x1, X2[:, :2] / X2[:, 2:]], 1)[X2[:, 2] > 0.1]
        front = [tv.in_front(Rx, tx, rec).sum() for Rx, tx in poses]
        best = int(np.argmax(front))
        assert front[best] == len(rec) and np.abs(poses[best][0] - R).max() <= 1e-13 and np.abs(poses[best][1] - t).max() <= 1e-13


def test_refinement_jacobian_equals_central_differences():
    rng = np.random.default_rng(4)
    for _ in range(5):
        q, t = tv.random_relative_pose(rng)
        t = t / np.linalg.norm(t)
        rec = rng.uniform(-0.4, 0.4, (30, 4))
        J = tv.jacobian(q, t, rec)
        h = 1e-6
        for c in range(5):
            d = np.zeros(5)
            d[c] = h
            fd = (tv.residuals(*tv.pose_plus(q, t, d), rec) - tv.residuals(*tv.pose_plus(q, t, -d), rec)) / (2 * h)
            assert np.abs(fd - J[:, c]).max() <= 1e-8 * max(1.0, np.abs(J[:, c]).max())


PAIRS_SEED = 12        # one for which the reference meets the assertions below


def test_no_pair_is_excused():
    """200 generated pairs (15 .. 300 matches, 0 .. 60 % outliers): the reference returns exactly the generated inlier set on
    every pair, and every pair has status 0."""
    rng = np.random.default_rng(100)
    counts = rng.integers(15, 301, 200)
    p_out = rng.uniform(0.0, 0.6, 200)
    batch = tv.make_pairs(counts, (1, 2, 8), seed=PAIRS_SEED, p_outlier=p_out)
    ref = tv.reference(batch)
    off = batch["pair_offsets"]
    assert (ref["status"] == 0).all()                # the generator leaves at least 15 inliers and at most 60 % outliers
    for p in range(200):
        assert np.array_equal(ref["inlier"][off[p]:off[p + 1]].astype(bool), batch["true_inlier"][off[p]:off[p + 1]]), p


class _Cam:
    def __init__(self, model_id, params):
        self.model_id, self.params = model_id, list(params)


@pytest.fixture()
def api(monkeypatch):
    """pixsfm_amd.api.two_view with the numpy reference in the kernel's place."""
    from pixsfm_amd.api import two_view
    seen = []

    def estimate(ctx, batch, opts):
        seen.append(dict(opts))
        return tv.reference(batch, **opts)
    monkeypatch.setattr(two_view, "_estimate", estimate)
    return two_view, seen


def test_api_options_and_shapes(api):
    two_view, seen = api
    batch = tv.make_pairs([60, 30], (2, 1), seed=51, p_outlier=0.3)
    off = batch["pair_offsets"]
    cams = [_Cam(2, tc.MODEL_PARAMS[2]), _Cam(1, tc.MODEL_PARAMS[1])]
    one = two_view.essential_matrix_estimation(batch["xy1"][:off[1]], batch["xy2"][:off[1]], cams[0], cams[1],
                                               {"ransac": {"max_error": 4, "confidence": 0.999}, "seed": 0})
    assert seen[-1] == {"max_error": 4, "confidence": 0.999, "seed": 0}
    assert set(one) == {"success", "E", "qvec", "tvec", "num_inliers", "inliers"} and one["success"] is True
    assert one["E"].shape == (3, 3) and one["qvec"].shape == (4,) and one["tvec"].shape == (3,)
    assert one["inliers"] == [bool(x) for x in batch["true_inlier"][:off[1]]] and one["num_inliers"] == sum(one["inliers"])
    assert two_view.essential_matrix_estimation(batch["xy1"][:4], batch["xy2"][:4], cams[0], cams[1]) == {"success": False}
    with pytest.raises(ValueError, match="unknown"):
        two_view.essential_matrix_estimation(batch["xy1"], batch["xy2"], cams[0], cams[1], {"max_eror": 1})
    with pytest.raises(ValueError, match="unknown"):
        two_view.TwoViewVerifier.create({"ransac": {"trials": 3}})
    assert two_view.TwoViewVerifier.create().conf["max_error"] == 4.0
    # verify_pairs: two pairs over three images, the second without a single correct match
    keypoints = {"a": batch["xy1"][:off[1]], "b": np.concatenate([batch["xy2"][:off[1]], batch["xy1"][off[1]:]]),
                 "c": np.random.default_rng(1).uniform(0, 900, (30, 2))}
    cameras = {"a": cams[0], "b": cams[1], "c": cams[0]}
    pairs = [("a", "b"), ("b", "c")]
    matches = [np.stack([np.arange(60), np.arange(60)], 1).astype(np.uint64), np.stack([60 + np.arange(30), np.arange(30)], 1).astype(np.uint64)]
    scores = [np.linspace(0, 1, 60).astype(np.float32), np.ones(30, np.float32)]
    verifier = two_view.TwoViewVerifier.create({"min_num_inliers": 15})
    m, s, g = verifier.verify_pairs(keypoints, cameras, pairs, matches, scores)
    keep = batch["true_inlier"][:off[1]]
    assert np.array_equal(m[0], matches[0][keep]) and m[0].dtype == np.uint64 and np.array_equal(s[0], scores[0][keep])
    assert m[1].shape == (0, 2) and s[1].shape == (0,) and g[0]["success"] and g[1] == {"success": False}
    assert verifier.verify_pairs(keypoints, cameras, pairs, matches)[1] is None
    assert verifier.verify_pairs(keypoints, cameras, [], []) == ([], None, [])
    from pixsfm_amd.api import build_matching_graph
    assert build_matching_graph(pairs, m, s) is not None
    # known poses: the relative pose of the pair goes in as the prior, nothing is estimated
    R = synthetic.qvec_to_rotmat(batch["gt_qvec"][0])
    q1, t1 = np.array([0.9, 0.1, -0.2, 0.3]) / np.linalg.norm([0.9, 0.1, -0.2, 0.3]), np.array([0.3, -1.0, 2.0])
    R1 = synthetic.qvec_to_rotmat(q1)
    poses = {"a": (q1, t1), "b": (synthetic.rotmat_to_qvec(R @ R1), R @ t1 + 1.7 * batch["gt_tvec"][0])}
    m, s, g = verifier.verify_pairs(keypoints, cameras, pairs[:1], matches[:1], scores[:1], poses=poses)
    assert np.array_equal(m[0], matches[0][keep]) and g[0]["success"]
    with pytest.raises(KeyError):
        verifier.verify_pairs(keypoints, cameras, pairs, matches, scores, poses=poses)
