"""One SHA-256 per case over the result of a solve.  BA: the refined q, t, k, X and the non-timing fields of the summary; keypoint
adjustment (the ka_* cases): the refined keypoints and the non-timing fields of every sub-problem's summary.

A refactor of the LM driver or of the KA solve must leave every line of this output unchanged: run it before and after on the same machine and
compare.  Only the public engine API is used, and the seeded generators the tests use (pixsfm_amd.synthetic, tests/geom_cases).

  python tools/ba_solve_fingerprint.py            # prints "<case> <sha256>" per line
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "pixel-perfect-sfm_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

FIELDS = ("iterations", "num_successful", "termination", "initial_cost", "final_cost", "final_radius", "linear_iterations",
          "linear_solver", "accumulation")
TIGHT_CG = dict(linear_solver="iterative", eta=0.0, linear_r_tolerance=1e-13, max_linear_solver_iterations=2000)


def digest(summary, params):
    h = hashlib.sha256()
    for a in params:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    for f in FIELDS:
        v = summary[f]
        h.update(np.float64(v).tobytes() if isinstance(v, float) else np.int64(v).tobytes())
    return h.hexdigest()


def gauge(prob, cam_mask=0b0110, const_points=()):
    n_img, n_cam, n_pts = len(prob["image_camera"]), len(prob["cam_model"]), len(prob["xyz"])
    pose_const = np.zeros(n_img, np.uint8); pose_const[0] = 1
    tmask = np.zeros(n_img, np.uint8); tmask[1] = 1
    point_const = np.zeros(n_pts, np.uint8); point_const[list(const_points)] = 1
    return pose_const, tmask, np.full(n_cam, cam_mask, np.uint16), point_const


def featuremetric(prob, g, env=None, forced=False, **opts):
    from pixsfm_amd.engine import BAProblem, Context, PatchArena, interp_cfg, lm_options, make_loss
    env = env or {}
    ctx = arena = None
    try:
        os.environ.update(env)
        ctx = Context(0)
        if forced:
            ctx.comm_init(Context.comm_unique_id(), 0, 1)
            ctx.comm_force(True)
        arena = PatchArena.from_numpy(ctx, prob["patches"], prob["corners"], prob["scales"])
        ba = BAProblem(ctx, arena, prob)
        s = ba.solve(interp_cfg(), make_loss("cauchy", [0.25]), *g, options=lm_options(**opts))
        return digest(s, ba.params())
    finally:
        for k in env:
            os.environ.pop(k, None)
        if arena is not None:
            arena.close()
        if ctx is not None:
            if forced:
                ctx.comm_destroy()
            ctx.close()


def geometric(prob, g, **opts):
    import geom_cases
    from pixsfm_amd.engine import Context, GeometricBAProblem, lm_options, make_loss
    ctx = Context(0)
    try:
        ba = GeometricBAProblem(ctx, geom_cases.geometric_dict(prob))
        s = ba.solve(make_loss("cauchy", [1.0]), *g, options=lm_options(**opts))
        return digest(s, ba.params())
    finally:
        ctx.close()


KA_FIELDS = ("iterations", "num_successful", "termination", "initial_cost", "final_cost", "linear_iterations")


def keypoint(prob, env, bound, l2_normalize=True, loss_a=0.25):
    """a deterministic pxr_ka_solve of one of tests/test_ka_gpu.py's problems"""
    from pixsfm_amd.engine import Context, PatchArena, interp_cfg, lm_options, make_loss
    from pixsfm_amd.ka_engine import KAProblem
    ctx = arena = None
    try:
        os.environ.update(env)
        ctx = Context(0)
        assert ctx.deterministic
        arena = PatchArena.from_numpy(ctx, prob["patches"], prob["corners"], prob["scales"])
        ka = KAProblem(ctx, arena, prob)
        total, per = ka.solve(interp_cfg(l2_normalize=l2_normalize), make_loss("cauchy", [loss_a]), bound=bound,
                              options=lm_options(parameter_tolerance=1e-5), per_problem=True)
        h = hashlib.sha256(np.ascontiguousarray(ka.keypoints(), dtype=np.float64).tobytes())
        for s in per:
            for f in KA_FIELDS:
                h.update(np.float64(s[f]).tobytes() if isinstance(s[f], float) else np.int64(s[f]).tobytes())
        return h.hexdigest()
    finally:
        for k in env:
            os.environ.pop(k, None)
        if arena is not None:
            arena.close()
        if ctx is not None:
            ctx.close()


def ka_cases():
    from pixsfm_amd import synthetic_ka
    # 30 sub-problems on a grid of 5 resident workgroups, active bounds (test_two_phase_launch_gives_the_one_phase_results_bit_for_bit)
    many = synthetic_ka.make_ka_problem(n_tracks=90, track_len=5, seed=17, max_kps_per_problem=15, sigma=1.5)
    yield "ka_one_launch", lambda: keypoint(many, {"PXR_KA_TWO_LAUNCH": "0", "PXR_KA_TWO_PHASE_RESIDENT": "5"}, 1.5)
    yield "ka_two_launches_resident_5", lambda: keypoint(many, {"PXR_KA_TWO_LAUNCH": "2", "PXR_KA_TWO_PHASE_RESIDENT": "5"}, 1.5)
    # raw features 300x unit norm: the fixed-point grid is rescaled between launches (test_two_launches_with_a_fixed_point_rescale_in_between)
    raw = dict(synthetic_ka.make_ka_problem(n_tracks=90, track_len=5, seed=23, max_kps_per_problem=15, sigma=1.5))
    raw["patches"] = (raw["patches"].astype(np.float32) * 300.0).astype(np.float16)
    yield "ka_rescale_300x", lambda: keypoint(raw, {"PXR_KA_TWO_LAUNCH": "2", "PXR_KA_TWO_PHASE_RESIDENT": "5"}, 3.0,
                                              l2_normalize=False, loss_a=0.25 * 300.0)
    # one label group of 300 keypoints as chunks of whole tracks (test_chunked_label_group_takes_the_decisions_of_one_problem)
    group = synthetic_ka.make_ka_problem(n_tracks=60, track_len=5, seed=21, max_kps_per_problem=100000, sigma=1.5)
    yield "ka_chunked_label_group", lambda: keypoint(dict(group, node_track=group["track_of_node"]), {}, 1.5)


def cases():
    import geom_cases
    from pixsfm_amd import synthetic
    small = synthetic.make_ba_problem(n_cams=7, n_points=300, obs_per_point=4, seed=21)
    shared = synthetic.make_ba_problem(n_cams=7, n_points=300, obs_per_point=4, seed=22, shared_camera=True)
    perm = np.random.default_rng(5).permutation(len(small["obs_image"]))
    shuffled = dict(small, obs_image=small["obs_image"][perm], obs_point=small["obs_point"][perm], obs_patch=small["obs_patch"][perm])
    n_img = len(small["image_camera"])
    points_only = (np.ones(n_img, np.uint8), np.zeros(n_img, np.uint8), np.full(len(small["cam_model"]), 0xfff, np.uint16),
                   np.zeros(len(small["xyz"]), np.uint8))
    geo = geom_cases.make_case(n_cams=7, n_points=300, obs_per_point=4, seed=23, ramp=False)
    g, it = gauge(small, const_points=(3, 17)), 5
    yield "fm_direct", lambda: featuremetric(small, g, max_iterations=it)
    yield "fm_direct_inner", lambda: featuremetric(small, g, max_iterations=it, use_inner_iterations=True)
    yield "fm_iterative_unshared", lambda: featuremetric(small, g, max_iterations=it, **TIGHT_CG)
    yield "fm_iterative_shared", lambda: featuremetric(shared, gauge(shared), max_iterations=it, **TIGHT_CG)
    yield "fm_iterative_inexact_inner", lambda: featuremetric(shared, gauge(shared), max_iterations=it, linear_solver="iterative",
                                                              use_inner_iterations=True)
    yield "geometric_inner", lambda: geometric(geo, gauge(geo), max_iterations=it, use_inner_iterations=True)
    yield "points_only", lambda: featuremetric(small, points_only, max_iterations=it)
    yield "no_jacobi_scaling", lambda: featuremetric(small, g, max_iterations=it, jacobi_scaling=0)
    yield "setup_host", lambda: featuremetric(small, g, env={"PXR_BA_SETUP_HOST": "1"}, max_iterations=it, use_inner_iterations=True)
    yield "unordered_observations", lambda: featuremetric(shuffled, g, max_iterations=it, use_inner_iterations=True)
    yield "forced_collective", lambda: featuremetric(small, g, forced=True, max_iterations=it, use_inner_iterations=True)
    yield "forced_collective_iterative", lambda: featuremetric(shared, gauge(shared), forced=True, max_iterations=it, **TIGHT_CG)
    yield from ka_cases()


if __name__ == "__main__":
    for name, run in cases():
        print("%-28s %s" % (name, run()), flush=True)
