"""One SHA-256 per case over the result of a BA solve: the refined q, t, k, X and the non-timing fields of the summary.

A refactor of the LM driver must leave every line of this output unchanged: run it before and after on the same machine and
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


if __name__ == "__main__":
    for name, run in cases():
        print("%-28s %s" % (name, run()), flush=True)
