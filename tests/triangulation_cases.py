"""Helper of the triangulation tests (not collected): a numpy reference of the per-track estimator, written from its
specification (include/pixsfm_hip.h) and not from the kernel, an undistortion driven by the oracle's
camera models, and a geometry-only scene generator.

    solve(S)  = (sum_S (I - d d^t))^-1 sum_S (I - d d^t) c        closed-form symmetric 3 x 3 (adjugate)
    score(X)  : cos_i = d_i . (X - c_i) / |X - c_i|,  inlier_i = cos_i >= cos(max_angle_error)
    1 hypotheses over pairs a < b in lexicographic order (all P = n (n - 1) / 2, or floor(h P / max_hypotheses)), skipped when
      d_a . d_b > cos(min_tri_angle) or a / b is no inlier of X = solve({a, b})
    2 the largest (inlier count, -sum_inliers (1 - cos_i), -hypothesis index)
    3 X' = solve(inliers); kept with its inliers if it has at least as many
    4 final = angular inlier and pixel error <= max_reproj_error; if that removed any and >= 2 remain: X = solve(final), no re-scoring
    5 kept if |final| >= max(2, min_track_len) and the largest angle between rays X - c_i over pairs of final inliers >= min_tri_angle
"""
import functools

import numpy as np

import pxo
from pixsfm_amd import synthetic

DEFAULTS = dict(min_tri_angle=1.5, max_angle_error=2.0, max_reproj_error=4.0, min_track_len=2, max_hypotheses=256)

# the parameter sets of the undistortion checks: tests/test_camera_models_ext.py::EXT at full strength for the six less common
# models (restated: that file is a test module), moderate radial / tangential terms for models 2-4
MODEL_PARAMS = {
    0: [1200.0, 500, 480],
    1: [1200.0, 1180, 500, 480],
    2: [1200.0, 500, 480, 0.05],
    3: [1200.0, 500, 480, 0.05, -0.02],
    4: [1200.0, 1180, 500, 480, 0.05, -0.02, 1e-3, -5e-4],
    5: [1200.0, 1180, 500, 480, 0.02, -0.01, 0.003, -0.001],
    6: [1200.0, 1180, 500, 480, 0.05, -0.02, 1e-3, -5e-4, 0.01, 0.02, -0.01, 0.005],
    7: [1200.0, 1180, 500, 480, 0.9],
    8: [1200.0, 500, 480, 0.03],
    9: [1200.0, 500, 480, 0.03, -0.01],
    10: [1200.0, 1180, 500, 480, 0.03, -0.01, 1e-3, -5e-4, 0.004, -0.002, 1e-3, 2e-3],
}
SINGLE_FOCAL = (0, 2, 3, 8, 9)


# ---- undistortion ------------------------------------------------------------------------------------------------------------
def image_to_world(model, k, x, y, max_iters=32):
    """Newton on the oracle's world_to_image with its analytic Juv from the pinhole normalisation; (u, v, ok, steps)."""
    k = np.asarray(k, dtype=np.float64)
    fx, fy, cx, cy = (k[0], k[0], k[1], k[2]) if model in SINGLE_FOCAL else (k[0], k[1], k[2], k[3])
    u, v = (x - cx) / fx, (y - cy) / fy
    if model <= 1:
        return u, v, True, 0
    for it in range(max_iters):
        if not (np.isfinite(u) and np.isfinite(v)):
            return np.nan, np.nan, False, it
        xy, J, _ = pxo.world_to_image(model, k, u, v)
        r = xy - (x, y)
        det = J[0, 0] * J[1, 1] - J[0, 1] * J[1, 0]
        if not np.isfinite(det) or det == 0.0:
            return np.nan, np.nan, False, it
        du, dv = (J[1, 1] * r[0] - J[0, 1] * r[1]) / det, (J[0, 0] * r[1] - J[1, 0] * r[0]) / det
        u, v = u - du, v - dv
        if not du * du + dv * dv < np.inf:
            return np.nan, np.nan, False, it
        if du * du + dv * dv < 1e-20:
            return u, v, bool(np.isfinite(u) and np.isfinite(v)), it + 1
    return np.nan, np.nan, False, max_iters


def polar_grid(n_radii=13, n_angles=8, r_max=1.0):
    """(u, v) on n_radii radii 0 .. r_max (0 included) x n_angles angles."""
    r = np.linspace(0.0, r_max, n_radii)
    a = 2 * np.pi * (np.arange(n_angles) + 0.25) / n_angles
    return np.stack([np.outer(r, np.cos(a)).ravel(), np.outer(r, np.sin(a)).ravel()], 1)


def rays_of(problem):
    """World-frame rays of every observation of a flat problem: (d (n, 3) unit bearings, c (n, 3) centres, valid (n,))."""
    n = len(problem["obs_image"])
    d, c, valid = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, bool)
    R = [synthetic.qvec_to_rotmat(q) for q in problem["qvec"]]
    for i in range(n):
        im = problem["obs_image"][i]
        cam = problem["image_camera"][im]
        u, v, ok, _ = image_to_world(int(problem["cam_model"][cam]), problem["cam_params"][cam], *problem["obs_xy"][i])
        if ok:
            b = R[im].T @ np.array([u, v, 1.0])
            d[i], c[i] = b / np.linalg.norm(b), -R[im].T @ problem["tvec"][im]
            valid[i] = bool(np.isfinite(d[i]).all() and np.isfinite(c[i]).all())
    return d, c, valid


# ---- the estimator -------------------------------------------------------------------------------------------------------------
def solve(d, c, idx):
    """solve(S) for the rays idx of (d, c): adjugate of the symmetric 3 x 3, the sums in index order."""
    A = np.zeros(6)
    b = np.zeros(3)
    for i in idx:
        di, ci = d[i], c[i]
        A += [1.0 - di[0] * di[0], -(di[0] * di[1]), -(di[0] * di[2]), 1.0 - di[1] * di[1], -(di[1] * di[2]), 1.0 - di[2] * di[2]]
        b += ci - di * (di[0] * ci[0] + di[1] * ci[1] + di[2] * ci[2])
    a00, a01, a02, a11, a12, a22 = A
    c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
    c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
    det = a00 * c00 + a01 * c01 + a02 * c02
    with np.errstate(all="ignore"):
        return np.array([(c00 * b[0] + c01 * b[1] + c02 * b[2]) / det, (c01 * b[0] + c11 * b[1] + c12 * b[2]) / det,
                         (c02 * b[0] + c12 * b[1] + c22 * b[2]) / det])


def cosines(d, c, X):
    w = X - c
    with np.errstate(all="ignore"):
        return (d[:, 0] * w[:, 0] + d[:, 1] * w[:, 1] + d[:, 2] * w[:, 2]) / np.sqrt(w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1] + w[:, 2] * w[:, 2])


@functools.lru_cache(maxsize=None)
def _pairs(n):
    return np.triu_indices(n, 1)            # lexicographic (a < b)


def hypothesis_pairs(n, max_hypotheses):
    """Pair numbers of the hypotheses of a track with n valid observations."""
    P = n * (n - 1) // 2
    if P <= max_hypotheses:
        return np.arange(P, dtype=np.int64)
    return np.array([h * P // max_hypotheses for h in range(max_hypotheses)], dtype=np.int64)


def triangulate_track(d, c, reproj, **options):
    """The estimator on the VALID rays (d, c) of one track.  reproj(X) -> pixel error of every valid observation against X.
    Returns dict(status, X, inlier (mask over the valid rays), err, margin): margin = the smallest relative distance of any
    compared quantity to its threshold (cos vs cos(max_angle_error) in every scoring, d_a.d_b and the acceptance cosine vs
    cos(min_tri_angle), pixel errors vs max_reproj_error)."""
    o = {**DEFAULTS, **options}
    cos_tri, cos_err = np.cos(np.deg2rad(o["min_tri_angle"])), np.cos(np.deg2rad(o["max_angle_error"]))
    n = len(d)
    out = dict(status=1, X=None, inlier=np.zeros(n, bool), err=np.full(n, np.nan), margin=np.inf)
    if n < 2:
        return out
    margin = [np.inf]

    def near(values, threshold):
        v = np.asarray(values, dtype=np.float64)
        v = v[np.isfinite(v)]
        if len(v):
            margin[0] = min(margin[0], float(np.abs(v - threshold).min() / abs(threshold)))

    ia, ib = _pairs(n)
    best = None
    for h, p in enumerate(hypothesis_pairs(n, o["max_hypotheses"])):
        a, b = ia[p], ib[p]
        dab = d[a, 0] * d[b, 0] + d[a, 1] * d[b, 1] + d[a, 2] * d[b, 2]
        near(dab, cos_tri)
        if dab > cos_tri:
            continue
        X = solve(d, c, (a, b))
        cs = cosines(d, c, X)
        near(cs, cos_err)
        inl = cs >= cos_err
        if not (inl[a] and inl[b]):
            continue
        key = (int(inl.sum()), -float(np.cumsum(1.0 - cs[inl])[-1]), -h)      # (cumsum: the sum in index order)
        if best is None or key > best[0]:
            best = (key, X, inl)
    out["margin"] = margin[0]
    if best is None:
        out["status"] = 2
        return out
    _, X, inl = best
    X1 = solve(d, c, np.flatnonzero(inl))
    cs1 = cosines(d, c, X1)
    near(cs1, cos_err)
    inl1 = cs1 >= cos_err
    if inl1.sum() >= inl.sum():
        X, inl = X1, inl1
    err = reproj(X)
    near(err[inl], o["max_reproj_error"])
    with np.errstate(invalid="ignore"):
        final = inl & (err <= o["max_reproj_error"])
    if final.sum() < inl.sum() and final.sum() >= 2:
        X = solve(d, c, np.flatnonzero(final))
    out["status"], out["margin"] = 3, margin[0]
    if final.sum() < max(2, o["min_track_len"]) or not np.isfinite(X).all():
        return out
    w = X - c[final]
    e = w / np.linalg.norm(w, axis=1)[:, None]
    G = e @ e.T
    lowest = G[np.triu_indices(len(e), 1)].min()          # the widest pair
    near(lowest, cos_tri)
    out["margin"] = margin[0]
    if not lowest <= cos_tri:
        return out
    out.update(status=0, X=X, inlier=final, err=reproj(X))
    return out


def reference(problem, **options):
    """The estimator on every track of a flat problem (the dict engine.TriangulationProblem takes).  Returns dict(xyz (NaN
    without a point), status, n_inliers, obs_inlier, obs_err (NaN where no point exists), margin (per track))."""
    d, c, valid = rays_of(problem)
    off = np.asarray(problem["track_offsets"])
    T = len(off) - 1
    res = dict(xyz=np.full((T, 3), np.nan), status=np.zeros(T, np.int32), n_inliers=np.zeros(T, np.int32),
               obs_inlier=np.zeros(len(valid), np.uint8), obs_err=np.full(len(valid), np.nan), margin=np.full(T, np.inf))
    for t in range(T):
        obs = np.arange(off[t], off[t + 1])[valid[off[t]:off[t + 1]]]

        def reproj(X, obs=obs):
            e = np.empty(len(obs))
            for j, i in enumerate(obs):
                e[j] = np.hypot(*(project(problem, problem["obs_image"][i], X) - problem["obs_xy"][i]))
            return e
        r = triangulate_track(d[obs], c[obs], reproj, **options)
        res["status"][t], res["margin"][t] = r["status"], r["margin"]
        if r["status"] == 0:
            res["xyz"][t] = r["X"]
            res["n_inliers"][t] = r["inlier"].sum()
            res["obs_inlier"][obs] = r["inlier"]
            res["obs_err"][obs] = r["err"]
    return res


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def look_at_pose(centre):
    """World-to-camera (qvec, tvec) of a camera at `centre` looking at the origin (the construction of synthetic.ring_cameras)."""
    centre = np.asarray(centre, dtype=np.float64)
    z = -centre / np.linalg.norm(centre)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    return synthetic.rotmat_to_qvec(R), -R @ centre


def pad_params(params_list):
    out = np.zeros((len(params_list), 12))
    for i, p in enumerate(params_list):
        out[i, :len(p)] = p
    return out


def project(problem, image, X):
    cam = problem["image_camera"][image]
    m = int(problem["cam_model"][cam])
    return pxo.world_to_pixel(m, problem["cam_params"][cam][:pxo.lib().pxo_camera_num_params(m)], problem["qvec"][image],
                              problem["tvec"][image], X, jac=False)[0]


def make_scene(lengths, n_cams=96, models=(2,), seed=0, sigma=0.5, p_outlier=0.2, arc=24):
    """A geometry-only scene: ring cameras of radius 10 (camera i has model models[i % len(models)] with MODEL_PARAMS), one
    track per entry of `lengths` around a point in [-1, 1]^3, observed through the oracle's world_to_pixel with Gaussian
    keypoint noise sigma; in tracks of >= 4 views an observation is an outlier with probability p_outlier: displaced by
    100-300 px in a random direction.  A track of up to `arc` views picks its cameras among `arc` neighbours on the ring (no
    two rays of a short track face each other), a longer one among all (every camera once before any twice).
    Returns the flat problem dict + gt_xyz (n_tracks, 3) and true_inlier (n_obs,)."""
    rng = np.random.default_rng(seed)
    q, t = synthetic.ring_cameras(n_cams, rng=rng)
    problem = dict(qvec=q, tvec=t, image_camera=np.arange(n_cams, dtype=np.int32) % len(models),
                   cam_model=np.array(models, dtype=np.int32), cam_params=pad_params([MODEL_PARAMS[m] for m in models]))
    offsets, obs_image, obs_xy, true_inlier = [0], [], [], []
    gt = rng.uniform(-1, 1, (len(lengths), 3))
    for ti, L in enumerate(lengths):
        if L <= min(arc, n_cams):
            cams = (rng.integers(n_cams) + rng.choice(min(arc, n_cams), L, replace=False)) % n_cams
        else:
            cams = np.concatenate([rng.permutation(n_cams) for _ in range(-(-L // n_cams))])[:L]
        for im in cams:
            xy = project(problem, im, gt[ti]) + rng.normal(0, sigma, 2)
            bad = L >= 4 and rng.random() < p_outlier
            if bad:
                a = rng.uniform(0, 2 * np.pi)
                xy = xy + rng.uniform(100, 300) * np.array([np.cos(a), np.sin(a)])
            obs_image.append(im); obs_xy.append(xy); true_inlier.append(not bad)
        offsets.append(len(obs_image))
    problem.update(track_offsets=np.array(offsets, dtype=np.int64), obs_image=np.array(obs_image, dtype=np.int32),
                   obs_xy=np.array(obs_xy, dtype=np.float64).reshape(-1, 2), gt_xyz=gt, true_inlier=np.array(true_inlier, dtype=bool))
    return problem


def status_scene():
    """Three tracks that end with status 1, 2 and 3: one view; two views with 0.5 degrees of parallax; three views of which
    two are nearly parallel (0.5 degrees) and the third, 60 degrees away, is off by 40 px across the epipolar line -- its
    hypotheses survive the 2-degree angular test and every member then fails the 4 px reprojection filter."""
    ang = np.deg2rad([0.0, 0.5, 60.0])
    poses = [look_at_pose([10 * np.cos(a), 0.0, 10 * np.sin(a)]) for a in ang]
    problem = dict(qvec=np.array([p[0] for p in poses]), tvec=np.array([p[1] for p in poses]),
                   image_camera=np.zeros(3, np.int32), cam_model=np.array([2], np.int32), cam_params=pad_params([MODEL_PARAMS[2]]))
    X = np.array([0.05, -0.02, 0.03])
    xy = [project(problem, i, X) for i in range(3)]
    problem.update(track_offsets=np.array([0, 1, 3, 6], np.int64), obs_image=np.array([0, 0, 1, 0, 1, 2], np.int32),
                   obs_xy=np.array([xy[0], xy[0], xy[1], xy[0], xy[1], xy[2] + [0.0, 40.0]]))
    return problem
