"""GPU: geometric (reprojection-error) bundle adjustment -- pxr_ba_geom_eval / pxr_ba_solve_geometric (csrc/pxr_ba_geom.hip,
the geometric branch of csrc/pxr_ba_solve.hip) and the API on top of them.

References.  Values and Jacobians: pxo.world_to_pixel.  Trajectories: the oracle's restated Ceres loop (pxo.ba_solve) on the
RAMP form of the problem, on which its featuremetric residual IS the reprojection residual (tests/geom_cases.py; the bridge
itself is pinned in tests/test_geom_ba_cpu.py).  Optimum: scipy.optimize.least_squares through tests/scipy_ba.py.
Tolerances are the ones the featuremetric solver is held to on its exact-order path: tests/test_ba_eval_gpu.py (TOL),
tests/test_ba_solve_gpu.py (_assert_same), tests/test_ba_inner_gpu.py (nested loops: end points at 1e-4),
tests/test_ba_pcg_gpu.py (tight conjugate gradients), tests/test_third_party_solver.py (scipy)."""
import copy

import numpy as np
import pytest

import geom_cases
from test_ba_eval_gpu import TOL, _relerr
from test_ba_solve_gpu import _assert_same, _gauge

pytestmark = pytest.mark.gpu

CAUCHY = ("cauchy", 1.0)


def _problem(ctx, prob):
    from pixsfm_amd.engine import GeometricBAProblem
    return GeometricBAProblem(ctx, geom_cases.geometric_dict(prob))


def _solve(ctx, prob, gauge, loss=CAUCHY, **opt_kw):
    from pixsfm_amd.engine import lm_options, make_loss
    ba = _problem(ctx, prob)
    s = ba.solve(make_loss(loss[0], [loss[1]]), *gauge, options=lm_options(**opt_kw))
    return s, ba.params()


# ---- 1. records and Jacobians, all 11 camera models ---------------------------------------------------------------------------------
def _model_problem(model):
    """The scenes tests/test_ba_eval_gpu.py (models 0-4) and tests/test_camera_models_ext.py (5-10) evaluate, plus noisy keypoints."""
    from pixsfm_amd import synthetic
    if model <= 4:
        prob = synthetic.make_ba_problem(n_cams=5, n_points=67, obs_per_point=3, seed=10 + model, model=model)
    else:
        from test_camera_models_ext import _problem as ext_problem
        prob = ext_problem(model, seed=30 + model)
    prob = {k: v for k, v in prob.items() if k not in ("patches", "refs")}
    prob["obs_xy"] = prob["centers"] + np.random.default_rng(model).normal(0.0, 0.7, prob["centers"].shape)
    return prob


@pytest.mark.parametrize("model", list(range(11)))
def test_records_and_jacobians_match_the_oracles_projection(ctx, model):
    import pxo
    from pixsfm_amd.engine import make_loss
    prob = _model_problem(model)
    assert len(prob["obs_image"]) % 64 != 0                                # a ragged last wavefront
    ba = _problem(ctx, prob)
    rec, res = ba.eval()
    rec, res, P = rec.download(), res.download(), ba.projection_jacobian().download()
    n = len(res)
    K = pxo.lib().pxo_camera_num_params(model)
    xy, J = np.empty((n, 2)), np.zeros((n, 2, 22))
    for i in range(n):
        im, pt = prob["obs_image"][i], prob["obs_point"][i]
        cam = prob["image_camera"][im]
        xy[i], Jq, Jt, JX, Jk = pxo.world_to_pixel(model, prob["cam_params"][cam][:K], prob["qvec"][im], prob["tvec"][im], prob["xyz"][pt])
        J[i, :, 0:4], J[i, :, 4:7], J[i, :, 7:10], J[i, :, 10:10 + K] = Jq, Jt, JX, Jk
    r = xy - prob["obs_xy"]
    print("model %d: res %.2e  s %.2e  xy %.2e  P %.2e" % (model, _relerr(res, r), _relerr(rec[:, 0], (r * r).sum(1)),
                                                           _relerr(rec[:, 6:8], xy), _relerr(P, J)))
    assert _relerr(res, r) < TOL
    assert _relerr(rec[:, 0], (r * r).sum(1)) < TOL
    assert _relerr(rec[:, 4:6], r) < TOL and np.array_equal(rec[:, 4:6], res)
    assert _relerr(rec[:, 6:8], xy) < TOL
    assert np.array_equal(rec[:, 1:4], np.tile([1.0, 0.0, 1.0], (n, 1)))      # exactly
    assert _relerr(P, J) < TOL
    cost = ba.cost(make_loss(*("cauchy", [1.0])))
    want = geom_cases.robust_cost(prob, CAUCHY)
    assert abs(cost - want) < 1e-10 * want
    assert np.abs(ba.reprojection_errors() - np.hypot(r[:, 0], r[:, 1])).max() < TOL * np.abs(r).max()


# ---- 2. against the featuremetric kernel on the device ---------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [2, 4])
def test_records_equal_the_featuremetric_kernels_on_ramp_patches(ctx, model):
    """BAProblem.eval (the exact-order kernel, float64 3-channel ramp arena, l2_normalize off, zero references) and
    GeometricBAProblem.eval give the same records: 1e-10 relative per column (absolute for the column that is exactly 0)."""
    from pixsfm_amd.engine import BAProblem, PatchArena, interp_cfg
    prob = geom_cases.make_case(n_cams=6, n_points=50, obs_per_point=4, seed=20 + model, model=model, channels=3)
    arena = PatchArena.from_numpy(ctx, prob["patches"], prob["corners"], prob["scales"])
    feat = BAProblem(ctx, arena, prob).eval(interp_cfg(l2_normalize=False), with_jacobian=True)[0].download()
    geo = _problem(ctx, prob).eval()[0].download()
    for col in range(8):
        scale = max(np.abs(geo[:, col]).max(), 1.0 if col == 2 else 1e-300)
        err = np.abs(feat[:, col] - geo[:, col]).max() / scale
        print("column %d: %.2e" % (col, err))
        assert err < 1e-10, col
    arena.close()


# ---- 3. trajectory against the oracle -------------------------------------------------------------------------------------------------
def _assert_inner_same(s_gpu, pg, s_cpu, po, trajectory):
    """With inner iterations the nested LMs stop on Ceres' 1e-6 relative tolerances and may differ by one inner iteration between
    two implementations: end points at 1e-4 (tests/test_ba_inner_gpu.py:50-56), the outer decisions equal while descending."""
    if trajectory:
        assert s_gpu["iterations"] == s_cpu["iterations"] and s_gpu["num_successful"] == s_cpu["num_successful"]
        assert s_gpu["termination"] == s_cpu["termination"]
    assert abs(s_gpu["initial_cost"] - s_cpu["initial_cost"]) < 1e-10 * s_cpu["initial_cost"]
    assert abs(s_gpu["final_cost"] - s_cpu["final_cost"]) < 1e-4 * max(s_cpu["final_cost"], 1e-9)
    for a, b, name in zip(pg, po, ("qvec", "tvec", "cam", "xyz")):
        b = np.asarray(b)
        assert np.abs(a[:, :b.shape[1]] - b).max() < 1e-4 * max(1.0, np.abs(b).max()), name


def _report(tag, s, so, pg, po):
    d = [np.abs(a[:, :np.asarray(b).shape[1]] - b).max() for a, b in zip(pg, po)]
    print("%s: gpu it %d/%d term %d cost %.12e -> %.12e | oracle it %d/%d term %d cost %.12e -> %.12e | rel final %.2e | dq %.1e dt %.1e dk %.1e dX %.1e"
          % (tag, s["iterations"], s["num_successful"], s["termination"], s["initial_cost"], s["final_cost"], so["iterations"],
             so["num_successful"], so["termination"], so["initial_cost"], so["final_cost"],
             abs(s["final_cost"] - so["final_cost"]) / so["final_cost"], *d))


@pytest.mark.parametrize("inner", [False, True])
@pytest.mark.parametrize("model", [2, 0, 4])
def test_default_gauge_trajectory_matches_the_oracle(ctx, model, inner):
    prob = geom_cases.make_case(n_cams=6, n_points=60, obs_per_point=4, seed=40 + model, model=model)
    gauge = _gauge(prob)
    for max_it, trajectory in ((7, True), (30, False)):
        kw = dict(max_iterations=max_it, use_inner_iterations=inner, linear_solver="direct")
        s, pg = _solve(ctx, prob, gauge, **kw)
        kw.pop("linear_solver")
        so, po = geom_cases.oracle_solve(prob, CAUCHY, gauge, **kw)
        _report("model %d inner %d it %d" % (model, inner, max_it), s, so, pg, po)
        assert s["linear_solver"] == 1
        if inner:
            _assert_inner_same(s, pg, so, po, trajectory)
        else:
            _assert_same(s, pg, so, po, ptol=1e-6 if trajectory else 1e-4, trajectory=trajectory)
        assert s["final_cost"] < s["initial_cost"]
    assert s["final_cost"] < 0.5 * s["initial_cost"]                      # the 30-iteration run


@pytest.mark.parametrize("tracks", [2, 4, 9, 20])
def test_inner_iterations_over_track_lengths_and_parameterisations(ctx, tracks):
    """Tracks of 2 / 4 (one pass of the 8-lane groups), 9 and 20 observations (two and three passes, the tail read from global
    memory); a few constant points, a second constant pose, constant tvec components, the principal point refined and the extra
    parameters held, one camera shared by all images."""
    n_cams = max(7, tracks + 4)
    prob = geom_cases.make_case(n_cams=n_cams, n_points=36, obs_per_point=tracks, seed=60 + tracks, model=3, shared_camera=True)
    pose_const, tmask, cmask, ptc = _gauge(prob, refine_focal=True, refine_pp=True, refine_extra=False)
    pose_const[3] = 1
    tmask[2] = 0b101
    ptc[::7] = 1
    gauge = (pose_const, tmask, cmask, ptc)
    for inner in (True, False):
        kw = dict(max_iterations=5, use_inner_iterations=inner)
        s, pg = _solve(ctx, prob, gauge, linear_solver="direct", **kw)
        so, po = geom_cases.oracle_solve(prob, CAUCHY, gauge, **kw)
        _report("tracks %d inner %d" % (tracks, inner), s, so, pg, po)
        if inner:
            _assert_inner_same(s, pg, so, po, True)
        else:
            _assert_same(s, pg, so, po)
        q, t, k, X = pg
        assert np.array_equal(X[::7], prob["xyz"][::7])                   # constant points untouched
        assert np.array_equal(t[3], prob["tvec"][3]) and np.array_equal(t[0], prob["tvec"][0])
        assert t[2][0] == prob["tvec"][2][0] and t[2][2] == prob["tvec"][2][2] and t[2][1] != prob["tvec"][2][1]
        assert np.array_equal(k[0, 3:5], prob["cam_params"][0, 3:5]) and k[0, 0] != prob["cam_params"][0, 0]
        assert s["final_cost"] < s["initial_cost"]


@pytest.mark.parametrize("shared_camera", [False, True])
def test_tight_cg_takes_the_direct_geometric_steps(ctx, shared_camera):
    """The iterative Schur solver under the tight options of tests/test_ba_pcg_gpu.py:40-46 against the direct geometric solve."""
    prob = geom_cases.make_case(n_cams=24, n_points=600, obs_per_point=4, seed=5, shared_camera=shared_camera, ramp=False)
    gauge = _gauge(prob)
    tight = dict(linear_solver="iterative", eta=0.0, linear_r_tolerance=1e-13, max_linear_solver_iterations=2000)
    for iters in (1, 4):
        sd, pd = _solve(ctx, prob, gauge, max_iterations=iters, linear_solver="direct")
        si, pi = _solve(ctx, prob, gauge, max_iterations=iters, **tight)
        print("iters %d: direct %.12e iterative %.12e (initial %.6e), cg %d" % (iters, sd["final_cost"], si["final_cost"],
                                                                               sd["initial_cost"], si["linear_iterations"]))
        assert sd["linear_solver"] == 1 and si["linear_solver"] == 2 and si["linear_iterations"] > 0
        assert si["iterations"] == sd["iterations"] and si["num_successful"] == sd["num_successful"]
        assert abs(si["final_cost"] - sd["final_cost"]) < 1e-8 * sd["initial_cost"]


def test_auto_selection_follows_the_image_count(ctx):
    out = {}
    for n_img in (1000, 1001):
        prob = geom_cases.make_case(n_cams=n_img, n_points=700, obs_per_point=5, seed=3, ramp=False)
        s, _ = _solve(ctx, prob, _gauge(prob), max_iterations=2)
        out[n_img] = s
    assert out[1000]["linear_solver"] == 1 and out[1001]["linear_solver"] == 2
    assert out[1001]["final_cost"] < out[1001]["initial_cost"]


@pytest.mark.parametrize("n_points", [2047, 2048, 2049, 4100])
def test_point_structure_built_on_the_device_equals_the_host_lists(ctx, monkeypatch, n_points):
    """The per-point offsets, variable flags and their number come from a two-launch prefix sum over chunks of 2048 points
    (k_pt_scan_partials / k_pt_scan_apply over csrc/pxr_scan.h): one chunk short of full, exactly full, a second chunk of one
    point, and three chunks.  PXR_BA_SETUP_HOST=1 builds the same structure with host_lists; the bound is the one
    tests/test_ba_solve_gpu.py::test_device_built_observation_lists_equal_the_host_ones holds the two paths to."""
    prob = geom_cases.make_case(n_cams=8, n_points=n_points, obs_per_point=3, seed=n_points, ramp=False)
    gauge = _gauge(prob)
    gauge[3][::7] = 1                                                       # constant points: the flags and their count
    s_dev, p_dev = _solve(ctx, prob, gauge, max_iterations=2, linear_solver="direct")
    monkeypatch.setenv("PXR_BA_SETUP_HOST", "1")
    s_host, p_host = _solve(ctx, prob, gauge, max_iterations=2, linear_solver="direct")
    monkeypatch.delenv("PXR_BA_SETUP_HOST")
    print("%d points: cost %.15e (device lists) %.15e (host lists)" % (n_points, s_dev["final_cost"], s_host["final_cost"]))
    assert s_host["iterations"] == s_dev["iterations"] and s_host["num_successful"] == s_dev["num_successful"] >= 1
    assert abs(s_host["final_cost"] - s_dev["final_cost"]) <= 1e-9 * abs(s_dev["final_cost"])
    assert all(np.abs(a - b).max() <= 1e-9 * max(1.0, np.abs(b).max()) for a, b in zip(p_host, p_dev))
    assert np.array_equal(p_dev[3][::7], prob["xyz"][::7])                  # constant points untouched


def test_non_finite_initial_evaluation_is_a_failed_solve_not_an_error(ctx):
    """[upstream] "Initial residual and Jacobian evaluation failed": termination FAILURE, the call itself succeeds and the
    parameters stay where they were -- the semantics of pxr_ba_solve."""
    prob = geom_cases.make_case(n_cams=6, n_points=30, obs_per_point=3, seed=8, ramp=False)
    prob["obs_xy"] = prob["obs_xy"].copy()
    prob["obs_xy"][7, 0] = np.nan
    s, (q, t, k, X) = _solve(ctx, prob, _gauge(prob), max_iterations=5, use_inner_iterations=True)
    assert s["termination"] == 2 and s["iterations"] == 0 and not np.isfinite(s["initial_cost"])
    assert np.array_equal(t, prob["tvec"]) and np.array_equal(X, prob["xyz"])


# ---- 4. the optimum against third-party code ------------------------------------------------------------------------------------------
SCENES = {   # name: (make_case arguments, loss, a, gauge changes) -- one camera shared by all images, focal length + extra parameters refined
    "cauchy": (dict(n_cams=6, n_points=40, obs_per_point=4, seed=42, model=2, shared_camera=True), "cauchy", 1.0, {}),
    "huber_constant_points": (dict(n_cams=6, n_points=40, obs_per_point=3, seed=43, model=3, shared_camera=True), "huber", 1.0, dict(const_points=5)),
    # (OPENCV with all four distortion coefficients free is not determined by six views of 45 noisy points: scipy itself does not
    #  settle there -- its two runs end 5e-6 apart in cost --, so the soft_l1 scene refines RADIAL's two coefficients)
    "soft_l1": (dict(n_cams=6, n_points=45, obs_per_point=4, seed=44, model=3, shared_camera=True), "soft_l1", 1.0, {}),
    "trivial": (dict(n_cams=6, n_points=40, obs_per_point=4, seed=45, model=2, shared_camera=True), "trivial", 1.0, {}),
}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_gpu_geometric_ba_ends_at_scipys_optimum(ctx, name):
    import pxo
    import scipy_ba
    from test_third_party_solver import _rel
    kw, loss, a, g = SCENES[name]
    prob = geom_cases.make_case(**kw)
    gauge = _gauge(prob)
    if g.get("const_points"):
        gauge[3][::g["const_points"]] = 1
    sp = scipy_ba.ScipyBA(prob, gauge, cfg=pxo.cfg(l2_normalize=False))
    xa, ca, xs, cs, _ = scipy_ba.solve(sp, loss, a)
    p = sp.unpack(xs)
    geom_cases.assert_inside(prob, p["qvec"], p["tvec"], p["cam_params"], p["xyz"], what="scipy's solution")
    s, (q, t, k, X) = _solve(ctx, prob, gauge, loss=(loss, a), max_iterations=100)
    rel = _rel(sp.pack(q, t, k[:, :12], X), xs)
    print("%s: rel %.3e  cost gpu %.15e scipy %.15e (%.2e)  iterations %d termination %d" % (
        name, rel, s["final_cost"], cs, abs(s["final_cost"] - cs) / cs, s["iterations"], s["termination"]))
    assert rel < 1e-6, (name, rel)
    assert abs(s["final_cost"] - cs) < 1e-9 * cs, (name, s["final_cost"], cs)


# ---- 5. determinism and collectives -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inner", [False, True])
def test_two_solves_are_bit_identical(ctx, inner):
    assert ctx.deterministic
    prob = geom_cases.make_case(n_cams=8, n_points=300, obs_per_point=5, seed=9, ramp=False)
    gauge = _gauge(prob)
    (s0, p0), (s1, p1) = (_solve(ctx, prob, gauge, max_iterations=6, use_inner_iterations=inner, linear_solver="direct") for _ in range(2))
    assert s0["accumulation"] == 1 and s1["accumulation"] == 1
    assert s0["initial_cost"] == s1["initial_cost"] and s0["final_cost"] == s1["final_cost"] and s0["iterations"] == s1["iterations"]
    assert s0["final_cost"] < s0["initial_cost"]
    for a, b in zip(p0, p1):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("inner", [False, True])
def test_forced_native_collective_equals_the_plain_solve_bit_for_bit(inner):
    from pixsfm_amd import PixsfmHipError
    from pixsfm_amd.engine import Context
    prob = geom_cases.make_case(n_cams=6, n_points=120, obs_per_point=4, seed=17, ramp=False)
    gauge = _gauge(prob)
    out = []
    for forced in (False, True):
        c = Context(0)
        if forced:
            try:
                c.comm_init(Context.comm_unique_id(), 0, 1)
            except PixsfmHipError as e:
                c.close()
                pytest.skip("RCCL cannot be loaded: %s" % e)
            c.comm_force(True)
        s, p = _solve(c, prob, gauge, max_iterations=6, use_inner_iterations=inner)
        calls, nbytes = c.comm_stats()
        out.append((s, p, calls, nbytes))
        if forced:
            c.comm_destroy()
        c.close()
    (s0, p0, calls0, _), (s1, p1, calls1, bytes1) = out
    assert calls0 == 0 and calls1 >= 2 * s1["iterations"] and bytes1 > 0
    assert s1["iterations"] == s0["iterations"] and s1["num_successful"] == s0["num_successful"]
    assert s1["initial_cost"] == s0["initial_cost"] and s1["final_cost"] == s0["final_cost"]
    for a, b in zip(p0, p1):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("inner", [False, True])
def test_two_rank_partition_on_one_gpu(ctx, inner):
    """The multi-rank branch (points sharded with their observations and keypoints, cameras replicated, all-reduce of the reduced
    camera system through a caller-supplied callback) with two solver instances on ONE GPU: two host threads, an in-process sum
    (the pattern of tests/test_ba_solve_gpu.py::test_two_rank_partition_on_one_gpu).  Deterministic default: the one-rank bits."""
    import ctypes as C
    import threading
    from pixsfm_amd.engine import Context, GeometricBAProblem, lm_options, make_loss
    from pixsfm_amd.parallel import shard_ba_problem
    prob = geom_cases.make_case(n_cams=6, n_points=64, obs_per_point=4, seed=91, ramp=False)
    prob["obs_patch"] = np.arange(len(prob["obs_xy"]), dtype=np.int64)      # (shard_ba_problem slices by it; not used otherwise)
    gauge = _gauge(prob)
    opts = dict(max_iterations=6, use_inner_iterations=inner)
    s_ref, ref = _solve(ctx, prob, gauge, **opts)
    world = 2
    barrier, stage, results = threading.Barrier(world), {}, [None] * world

    def worker(rank):
        c = Context(0)
        shard, pt_ids = shard_ba_problem(prob, rank, world)
        shard["obs_xy"] = prob["obs_xy"][shard["obs_ids"]]
        b = GeometricBAProblem(c, geom_cases.geometric_dict(shard))

        def allreduce(ptr, count):
            buf = np.empty(count)
            c.sync()
            c.lib.pxr_memcpy_d2h(c.handle, buf.ctypes.data, C.c_void_p(ptr), count * 8)
            stage[rank] = buf
            barrier.wait()
            tot = stage[0] + stage[1]
            barrier.wait()
            c.lib.pxr_memcpy_h2d(c.handle, C.c_void_p(ptr), tot.ctypes.data, count * 8)

        s = b.solve(make_loss(*("cauchy", [1.0])), gauge[0], gauge[1], gauge[2], gauge[3][pt_ids], options=lm_options(**opts),
                    allreduce=allreduce)
        results[rank] = (s, b.params(), pt_ids)
        c.sync()

    th = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join(timeout=120) for t in th]
    assert all(r is not None for r in results)
    for s, (q, t, k, X), pt_ids in results:
        assert s["iterations"] == s_ref["iterations"] and s["num_successful"] == s_ref["num_successful"]
        assert s["final_cost"] == s_ref["final_cost"] and s["initial_cost"] == s_ref["initial_cost"]
        assert np.array_equal(q, ref[0]) and np.array_equal(t, ref[1]) and np.array_equal(k, ref[2])
        assert np.array_equal(X, ref[3][pt_ids])


# ---- 6. the API end to end --------------------------------------------------------------------------------------------------------------
def _noisy_reconstruction(seed=3, **kw):
    from pixsfm_amd.api.reconstruction import Point2D, reconstruction_from_flat
    prob = geom_cases.make_case(n_cams=6, n_points=50, obs_per_point=4, seed=seed, ramp=False, **kw)
    rec, _ = reconstruction_from_flat(dict(prob, centers=prob["obs_xy"], obs_patch=np.arange(len(prob["obs_xy"]))))
    rec.images[2].points2D.append(Point2D([10.0, 20.0]))                   # a point2D without a 3D point: no observation
    return rec


def _mean_reprojection_error(rec):
    import pxo
    e = []
    for im in rec.images.values():
        cam = rec.cameras[im.camera_id]
        for p in im.points2D:
            if p.has_point3D():
                xy = pxo.world_to_pixel(cam.model_id, cam.params, im.qvec, im.tvec, rec.points3D[p.point3D_id].xyz, jac=False)[0]
                e.append(np.hypot(*(xy - p.xy)))
    return float(np.mean(e))


def _state(rec):
    return ([rec.images[i].qvec.copy() for i in sorted(rec.images)], [rec.images[i].tvec.copy() for i in sorted(rec.images)],
            [rec.cameras[c].params.copy() for c in sorted(rec.cameras)], [rec.points3D[p].xyz.copy() for p in sorted(rec.points3D)])


def _same_bits(a, b):
    return all(np.array_equal(x, y) for u, v in zip(a, b) for x, y in zip(u, v))


def test_api_refine_run_callbacks_and_multilevel():
    from pixsfm_amd.api import BundleAdjuster, GeometricBundleOptimizer, default_problem_setup
    rec = _noisy_reconstruction()
    rec_run, rec_cb, rec_abort, rec_ml = (copy.deepcopy(rec) for _ in range(4))
    before = _mean_reprojection_error(rec)
    q0, t0, k0, _ = _state(rec)
    adj = BundleAdjuster.create({"strategy": "geometric", "optimizer": {"solver": {"max_num_iterations": 12}}})
    out = adj.refine(rec)
    summ = out["summary"]
    after = _mean_reprojection_error(rec)
    print("mean reprojection error %.4f -> %.4f px, %d iterations" % (before, after, summ.num_iterations))
    assert set(out) == {"summary"} and after < before
    assert summ.num_residuals_reduced == 2 * rec.num_observations()
    q1, t1, k1, _ = _state(rec)
    assert np.array_equal(q1[0], q0[0] / np.linalg.norm(q0[0])) and np.array_equal(t1[0], t0[0])       # the constant pose (NormalizeQvec only)
    assert t1[1][0] == t0[1][0] and not np.array_equal(t1[1], t0[1])                                  # constant tvec component
    for a, b in zip(k0, k1):
        assert np.array_equal(a[1:3], b[1:3]) and a[0] != b[0]                                        # principal point held, focal refined
    # the optimizer class on a copy: the same bits
    opt = GeometricBundleOptimizer(copy.deepcopy(adj.conf["optimizer"]), default_problem_setup(rec_run))
    assert opt.run(rec_run) is True
    assert _same_bits(_state(rec), _state(rec_run))
    assert opt.summary().num_residuals_reduced == summ.num_residuals_reduced
    # solver.callbacks: one call after the initial evaluation and one per iteration
    seen = []
    options = copy.deepcopy(adj.conf["optimizer"])
    options["solver"]["callbacks"] = [lambda it: seen.append((it.iteration, it.cost))]
    opt = GeometricBundleOptimizer(options, default_problem_setup(rec_cb))
    opt.run(rec_cb)
    n_it = len(opt.summary().iterations) - 1
    assert [i for i, _ in seen] == list(range(n_it + 1)) and n_it >= 2
    assert _same_bits(_state(rec), _state(rec_cb))                                                    # observing changes nothing
    # "abort" at iteration 2: the parameters of the last accepted step, i.e. of a solve limited to 2 iterations
    options = copy.deepcopy(adj.conf["optimizer"])
    options["solver"]["callbacks"] = [lambda it: 1 if it.iteration == 2 else 0]
    opt = GeometricBundleOptimizer(options, default_problem_setup(rec_abort))
    opt.run(rec_abort)
    rec_two = copy.deepcopy(_noisy_reconstruction())
    options = copy.deepcopy(adj.conf["optimizer"])
    options["solver"]["max_num_iterations"] = 2
    GeometricBundleOptimizer(options, default_problem_setup(rec_two)).run(rec_two)
    assert len(opt.summary().iterations) == 3 and _same_bits(_state(rec_abort), _state(rec_two))
    # the adjuster's own callbacks (main.py:63) reach the solver too
    adj.callbacks = [lambda it: seen.append("adjuster")]
    # refine_multilevel hands over a feature set and the setup positionally: both ignored (main.py:299-303)
    class Manager:
        num_levels = 2

        def fset(self, level):
            return object()
    outs = adj.refine_multilevel(rec_ml, Manager())
    assert len(outs["summary"]) == 2 and "adjuster" in seen
    first, second = outs["summary"]
    # the second level starts where the first ended (the mean error is not the objective -- the robust cost is)
    assert abs(second.initial_cost - first.final_cost) <= 1e-9 * first.final_cost and second.final_cost <= second.initial_cost
    assert first.initial_cost == summ.initial_cost and first.final_cost == summ.final_cost
    assert _mean_reprojection_error(rec_ml) < before


def test_api_outside_image_enters_with_a_constant_pose():
    from pixsfm_amd.api import BundleAdjuster, BundleAdjustmentSetup
    rec = _noisy_reconstruction(seed=4)
    ids = rec.reg_image_ids()
    setup = BundleAdjustmentSetup()
    setup.add_images(ids[:-1])
    setup.set_constant_pose(ids[0])
    setup.set_constant_tvec(ids[1], [0])
    for p in rec.point3D_ids():
        setup.add_variable_point(p)                                       # the observations from the last image come back
    q0, t0, _, X0 = _state(rec)
    before = _mean_reprojection_error(rec)
    out = BundleAdjuster.create({"strategy": "geometric"}).refine(rec, problem_setup=setup)
    q1, t1, _, X1 = _state(rec)
    assert out["summary"].num_residuals_reduced == 2 * rec.num_observations()     # all of them, the outside image's included
    # outside the setup: a constant pose (the solver normalises every quaternion it is handed, like Image::NormalizeQvec: the
    # rotation is the same, the last bits of q may not be)
    assert np.abs(q1[-1] - q0[-1]).max() <= 4 * np.finfo(np.float64).eps and np.array_equal(t1[-1], t0[-1])
    assert not np.array_equal(q1[2], q0[2]) and not np.array_equal(X1[0], X0[0])
    assert _mean_reprojection_error(rec) < before


# ---- 7. size ------------------------------------------------------------------------------------------------------------------------------
def test_one_million_observations():
    """200 cameras x 200k points x 5 observations from seeded noise (no arena: 16 MB of keypoints)."""
    import pxo
    from pixsfm_amd import synthetic
    from pixsfm_amd.engine import Context, GeometricBAProblem, lm_options, make_loss
    rng = np.random.default_rng(11)
    n_cam, n_pts, per = 200, 200_000, 5
    q_gt, t_gt = synthetic.ring_cameras(n_cam, rng=rng)
    k = np.zeros((n_cam, 12)); k[:, :4] = [1200.0, 500, 500, 0.02]
    X_gt = rng.uniform(-1, 1, (n_pts, 3))
    obs_point = np.repeat(np.arange(n_pts, dtype=np.int32), per)
    # five distinct cameras per point: a random start and four distinct positive strides
    obs_image = ((rng.integers(0, n_cam, n_pts)[:, None] + np.cumsum(rng.integers(1, n_cam // per, (n_pts, per)), 1)) % n_cam).astype(np.int32).reshape(-1)
    # vectorised SIMPLE_RADIAL projection of the generator (synthetic.project, model 2)
    R = np.stack([synthetic.qvec_to_rotmat(q) for q in q_gt])
    p = np.einsum("nij,nj->ni", R[obs_image], X_gt[obs_point]) + t_gt[obs_image]
    u, v = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
    rad = 1.0 + 0.02 * (u * u + v * v)
    obs_xy = np.stack([1200.0 * u * rad + 500, 1200.0 * v * rad + 500], 1) + rng.normal(0, 0.5, (len(u), 2))
    prob = dict(obs_image=obs_image, obs_point=obs_point, obs_xy=obs_xy, image_camera=np.arange(n_cam, dtype=np.int32),
                qvec=q_gt, tvec=t_gt + rng.normal(0, 0.01, t_gt.shape), cam_model=np.full(n_cam, 2, np.int32), cam_params=k,
                xyz=X_gt + rng.normal(0, 0.01, X_gt.shape))
    c = Context(0)
    ba = GeometricBAProblem(c, prob)
    rec = ba.eval()[0].download()
    pick = rng.choice(len(obs_image), 512, replace=False)
    for i in pick:
        im, pt = obs_image[i], obs_point[i]
        xy = pxo.world_to_pixel(2, k[im][:4], prob["qvec"][im], prob["tvec"][im], prob["xyz"][pt], jac=False)[0]
        r = xy - obs_xy[i]
        assert np.abs(rec[i, 6:8] - xy).max() < TOL * np.abs(xy).max() and np.abs(rec[i, 4:6] - r).max() < TOL * max(1.0, np.abs(r).max())
        assert abs(rec[i, 0] - r @ r) <= TOL * max(r @ r, 1.0) and rec[i, 1:4].tolist() == [1.0, 0.0, 1.0]
    s = ba.solve(make_loss("cauchy", [1.0]), *_gauge(prob), options=lm_options(max_iterations=5, use_inner_iterations=True))
    print("1M observations: %d iterations (%d successful), cost %.6e -> %.6e, %.1f ms (+ %.1f ms set-up), solver %d"
          % (s["iterations"], s["num_successful"], s["initial_cost"], s["final_cost"], s["total_ms"], s["setup_ms"], s["linear_solver"]))
    assert s["linear_solver"] == 1                                        # 200 images: the direct solver
    assert s["num_successful"] >= 1 and s["final_cost"] < s["initial_cost"]
    assert np.isfinite(ba.reprojection_errors()).all()
    c.close()
