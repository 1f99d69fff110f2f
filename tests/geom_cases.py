"""Geometric (reprojection-error) BA cases and the bridge that lets the featuremetric oracle check them.

The oracle (oracle/pxo_solve.c) has no reprojection cost of its own.  It IS one when it is handed RAMP patches: give every
observation a float64 patch whose texel (row j, column i) holds

    ((x0 + i + .5) / sx - x_obs,  (y0 + j + .5) / sy - y_obs)          (FeaturePatch::ToImageCoordinates)

zero references and l2_normalize=False.  Catmull-Rom interpolation reproduces linear functions exactly, so the oracle's
featuremetric residual at a projection (x, y) is (x - x_obs, y - y_obs) -- the reprojection residual -- as long as the 4 x 4
stencil stays inside the patch, i.e. the projection is at least 2 texels away from the border.  Every case handed out here is
therefore checked: the reprojection errors at the initial parameters (make_case) and at the oracle's solution (oracle_solve)
must be below patch_size / 2 - 3 pixels (13 px for 32 x 32 patches centred on the keypoint).  A case that violates the bound
is a broken case: fix the case, never skip it.

A track of n observations needs a scene of at least n cameras (a point is seen once per image).
"""
import numpy as np

PATCH_SIZE = 32
RAMP_LOSS = ("cauchy", 1.0)


def margin(patch_size=PATCH_SIZE):
    """Largest reprojection error (px, scale 1) for which the ramp equivalence holds."""
    return patch_size / 2.0 - 3.0


def ramp_patches(obs_xy, scales, patch_size=PATCH_SIZE, channels=2):
    """(patches (n, ps, ps, channels) float64, corners (n, 2) int32): ramp patches centred on the observed keypoints.  Channels
    beyond the second are zero (pxr_ba_eval wants 1, 3, 64 or 128 channels: use 3)."""
    obs_xy = np.asarray(obs_xy, dtype=np.float64)
    scales = np.asarray(scales, dtype=np.float64)
    n = len(obs_xy)
    corners = np.floor(obs_xy * scales - patch_size / 2.0).astype(np.int32)      # extractor.py:192-193
    ii = np.arange(patch_size, dtype=np.float64)
    xs = (corners[:, 0:1] + ii[None, :] + 0.5) / scales[:, 0:1] - obs_xy[:, 0:1]  # (n, ps): by column
    ys = (corners[:, 1:2] + ii[None, :] + 0.5) / scales[:, 1:2] - obs_xy[:, 1:2]  # (n, ps): by row
    patches = np.zeros((n, patch_size, patch_size, channels), dtype=np.float64)
    patches[..., 0] = xs[:, None, :]
    patches[..., 1] = ys[:, :, None]
    return patches, corners


def reprojection(prob, qvec=None, tvec=None, cam_params=None, xyz=None):
    """(n_obs, 2) pxo.world_to_pixel of every observation at the given (default: the problem's) parameters."""
    import pxo
    q = prob["qvec"] if qvec is None else qvec
    t = prob["tvec"] if tvec is None else tvec
    k = prob["cam_params"] if cam_params is None else cam_params
    X = prob["xyz"] if xyz is None else xyz
    out = np.empty((len(prob["obs_image"]), 2))
    for i, (im, pt) in enumerate(zip(prob["obs_image"], prob["obs_point"])):
        cam = prob["image_camera"][im]
        m = int(prob["cam_model"][cam])
        K = pxo.lib().pxo_camera_num_params(m)
        out[i] = pxo.world_to_pixel(m, np.asarray(k[cam])[:K], q[im], t[im], X[pt], jac=False)[0]
    return out


def reprojection_errors(prob, *params):
    r = reprojection(prob, *params) - prob["obs_xy"]
    return np.hypot(r[:, 0], r[:, 1])


def assert_inside(prob, *params, what=""):
    e = reprojection_errors(prob, *params)
    ps = prob["patches"].shape[1] if "patches" in prob else PATCH_SIZE
    assert np.isfinite(e).all() and e.max() < margin(ps), \
        "broken case (%s): reprojection error %.2f px leaves the ramp's linear zone (%.1f px)" % (what, e.max(), margin(ps))
    return e


def as_ramp_problem(prob, obs_xy, patch_size=PATCH_SIZE, channels=2):
    """A copy of a flat problem dict (synthetic.make_ba_problem layout) turned into its ramp form: obs_xy added, patches /
    corners / obs_patch / refs replaced.  Checked at the initial parameters."""
    out = {k: v for k, v in prob.items() if k not in ("patches", "corners", "refs", "obs_patch")}
    n = len(prob["obs_image"])
    out["obs_xy"] = np.ascontiguousarray(obs_xy, dtype=np.float64)
    out["scales"] = np.ones((n, 2))
    out["patches"], out["corners"] = ramp_patches(out["obs_xy"], out["scales"], patch_size, channels)
    out["obs_patch"] = np.arange(n, dtype=np.int64)
    out["refs"] = np.zeros((len(prob["xyz"]), channels))
    assert_inside(out, what="initial parameters")
    return out


def make_case(n_cams=6, n_points=40, obs_per_point=4, seed=0, model=2, keypoint_noise=0.6, shared_camera=False, channels=2,
              patch_size=PATCH_SIZE, ramp=True, **kw):
    """A synthetic scene (perturbed poses / points as make_ba_problem makes them) whose observed keypoints are the true
    projections plus seeded Gaussian noise of `keypoint_noise` px, in ramp form.  ramp=False: without the patches (a case that
    is not handed to the oracle -- 16 KB per observation saved); the initial errors are checked all the same."""
    from pixsfm_amd import synthetic
    assert obs_per_point <= n_cams, "a track of n observations needs a scene of at least n cameras"
    # (the featuremetric content of the generator is not used: the smallest it can render)
    base = synthetic.make_ba_problem(n_cams=n_cams, n_points=n_points, obs_per_point=obs_per_point, seed=seed, model=model,
                                     shared_camera=shared_camera, channels=1, patch_size=2, dtype=np.float64, **kw)
    rng = np.random.default_rng(1000 + seed)
    obs_xy = base["centers"] + rng.normal(0.0, keypoint_noise, base["centers"].shape)
    if ramp:
        return as_ramp_problem(base, obs_xy, patch_size, channels)
    out = {k: v for k, v in base.items() if k not in ("patches", "corners", "scales", "refs", "obs_patch")}
    out["obs_xy"] = obs_xy
    assert_inside(out, what="initial parameters")
    return out


# the generator's own parameter sets (synthetic.make_ba_problem), by COLMAP model id; the six others come from EXT
_BASE_PARAMS = {0: [1200.0, 500, 500], 1: [1200.0, 1180.0, 500, 500], 2: [1200.0, 500, 500, 0.02], 3: [1200.0, 500, 500, 0.02, -0.01],
                4: [1200.0, 1180.0, 500, 500, 0.02, -0.01, 1e-3, -5e-4]}
_TWO_FOCALS = (1, 4, 5, 6, 7, 10)


def model_params(model, pinhole):
    """The initial parameters of a camera of any of the eleven models: the parameter set the suite already uses for the model
    (the generator's for 0-4, EXT of tests/test_camera_models_ext.py for 5-10) with the distortion terms scaled by 0.05 -- FOV's
    omega set to 0.02, as in that file's _problem -- and focal length(s) and principal point of `pinhole` (fx, fy, cx, cy)."""
    if model in _BASE_PARAMS:
        k = np.array(_BASE_PARAMS[model], dtype=np.float64)
    else:
        from test_camera_models_ext import EXT
        k = np.array(EXT[model], dtype=np.float64)
    nf = 4 if model in _TWO_FOCALS else 3
    k[nf:] = 0.02 if model == 7 else k[nf:] * 0.05
    k[:nf] = pinhole if nf == 4 else [pinhole[0], pinhole[2], pinhole[3]]
    return k


def make_model_case(models, n_cams=6, n_points=90, obs_per_point=4, seed=0, keypoint_noise=0.7, shared_camera=False, ramp=True,
                    channels=2, patch_size=PATCH_SIZE):
    """A case for any of the eleven camera models; `models`: one id, or a list with one id per camera.  The scene is
    synthetic.make_ba_problem's PINHOLE scene (its perturbed poses and points) with cam_model / cam_params replaced by
    model_params; the observed keypoints are the projections AT THESE INITIAL PARAMETERS (pxo.world_to_pixel: the generator
    projects five models only) plus seeded Gaussian noise of `keypoint_noise` px.  ramp as in make_case."""
    from pixsfm_amd import synthetic
    assert obs_per_point <= n_cams, "a track of n observations needs a scene of at least n cameras"
    base = synthetic.make_ba_problem(n_cams=n_cams, n_points=n_points, obs_per_point=obs_per_point, seed=seed, model=1,
                                     shared_camera=shared_camera, channels=1, patch_size=2, dtype=np.float64, rot_deg=0.1)
    n_cam = len(base["cam_model"])
    models = [int(models)] * n_cam if np.isscalar(models) else [int(m) for m in models]
    assert len(models) == n_cam, "one model per camera"
    cam_params = np.zeros((n_cam, base["cam_params"].shape[1]))
    for c, m in enumerate(models):
        k = model_params(m, base["cam_params"][c, :4])
        cam_params[c, :len(k)] = k
    out = {k: v for k, v in base.items() if k not in ("patches", "corners", "scales", "refs", "obs_patch", "centers")}
    out["cam_model"] = np.array(models, dtype=np.int32)
    out["cam_params"] = cam_params
    rng = np.random.default_rng(1000 + seed)
    obs_xy = reprojection(out)
    obs_xy = obs_xy + rng.normal(0.0, keypoint_noise, obs_xy.shape)
    if ramp:
        return as_ramp_problem(out, obs_xy, patch_size, channels)
    out["obs_xy"] = obs_xy
    assert_inside(out, what="initial parameters")
    return out


def make_decoupled_case(models, nv, points_per_image=30, seed=0, keypoint_noise=0.7, ramp=False, channels=2, patch_size=PATCH_SIZE):
    """A scene whose reduced camera system is BLOCK DIAGONAL once images 0, 1, 2 are constant: 3 + nv images with one camera each
    (`models`: one id, or one per camera), nv * points_per_image points, point p observed in images 0, 1, 2 and in image
    3 + p % nv only -- no point is seen by two of the images 3 ... (make_model_case with every point in every image, filtered)."""
    n_cams = 3 + nv
    full = make_model_case(models, n_cams=n_cams, n_points=nv * points_per_image, obs_per_point=n_cams, seed=seed,
                           keypoint_noise=keypoint_noise, ramp=False)
    img, pt = np.asarray(full["obs_image"]), np.asarray(full["obs_point"])
    keep = (img < 3) | (img == 3 + pt % nv)
    out = dict(full)
    for key in ("obs_image", "obs_point", "obs_xy"):
        out[key] = np.ascontiguousarray(np.asarray(full[key])[keep])
    assert len(out["obs_image"]) == 4 * nv * points_per_image
    assert_inside(out, what="initial parameters")
    return as_ramp_problem(out, out["obs_xy"], patch_size, channels) if ramp else out


def geometric_dict(prob):
    """What engine.GeometricBAProblem takes."""
    return {k: prob[k] for k in ("obs_image", "obs_point", "obs_xy", "image_camera", "qvec", "tvec", "cam_model", "cam_params", "xyz")}


def oracle_eval(prob, loss=RAMP_LOSS, want_J=False):
    """(cost, r (n_obs, 2), J | None) of the oracle's featuremetric evaluation of the ramp problem."""
    import pxo
    cost, r, J = pxo.ba_eval_batch(prob, pxo.cfg(l2_normalize=False), pxo.loss(*loss), want_r=True, want_J=want_J)
    return cost, r[:, :2], J


def oracle_solve(prob, loss, gauge, **opt_kw):
    """pxo.ba_solve on the ramp problem = the oracle's geometric BA.  Checked at its solution."""
    import pxo
    s, q, t, k, X = pxo.ba_solve(prob, pxo.cfg(l2_normalize=False), pxo.loss(*loss), *gauge, pxo.lm_options(**opt_kw))
    assert_inside(prob, q, t, k, X, what="the oracle's solution")
    return s, (q, t, k, X)


def robust_cost(prob, loss, *params):
    """1/2 sum rho(|r|^2) from pxo.world_to_pixel and pxo.loss_eval."""
    import pxo
    e = reprojection_errors(prob, *params)
    ls = pxo.loss(*loss)
    return 0.5 * sum(pxo.loss_eval(ls, float(s))[0] for s in e * e)
