"""Global mapping: the numpy (float64) statement of the two specifications of include/pixsfm_hip.h --
pxr_rotation_averaging and pxr_global_positioning -- the synthetic scenes the tests share, and the figures the GPU and lane tests
are bounded by.  Nothing here touches a GPU.  The references handle the two pinhole models (closed-form undistortion)."""
import functools

import numpy as np

RADIUS = 10.0            # of the camera ring: the "scene radius" of the bounds below
FOCAL = 1200.0
WIDTH, HEIGHT = 1600, 1200

# ---- what the reference itself reaches against ground truth on the two scenes (measured by test_global_mapping_cpu.py, which
# asserts that they still hold): max rotation error in degrees, max centre error after a similarity alignment.  The conditions of
# the issue are 1 degree and 2 % of the ring radius (0.2); the seeds were chosen, on the reference alone, so that it sits about a
# factor of three inside both (seeds 1 .. 89 of the 100-image ring give 0.06 .. 0.25 for the centres).
SCENES = {
    "ring40": dict(n_images=40, nb=8, n_points=600, seed=1),
    "ring100": dict(n_images=100, nb=6, n_points=1500, seed=62),
}
REFERENCE_ERRORS = {
    "ring40": dict(max_rotation_deg=0.1024, max_centre=0.04465, iterations=24),
    "ring100": dict(max_rotation_deg=0.2177, max_centre=0.06670, iterations=26),
}
# ---- the largest difference between the kernels' source run lane by lane on the CPU and the reference, over boundary_batch() at
# every size (test_global_mapping_lanes_cpu.py prints them): rotations as quaternion components, centres / points / weights
# absolute.  The tests allow 100 times these, and never more than CAP = 1e-6 of the scene radius (for quaternions and weights,
# which are of order 1: 1e-6).
MEASURED = dict(qvec=3.4e-16, pair_angle=8.9e-16, centre=7.2e-13, xyz=7.7e-13, obs_weight=8.3e-13, pair_weight=5.8e-12)
CAP = 1e-6


def bound(key):
    cap = CAP * (RADIUS if key in ("centre", "xyz") else 1.0)
    return min(100.0 * MEASURED[key], cap)


# ---- quaternions (w, x, y, z), vectorised over the leading axes ---------------------------------------------------------------------
def qmul(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    w = a[..., 0] * b[..., 0] - a[..., 1] * b[..., 1] - a[..., 2] * b[..., 2] - a[..., 3] * b[..., 3]
    x = a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0] + a[..., 2] * b[..., 3] - a[..., 3] * b[..., 2]
    y = a[..., 0] * b[..., 2] - a[..., 1] * b[..., 3] + a[..., 2] * b[..., 0] + a[..., 3] * b[..., 1]
    z = a[..., 0] * b[..., 3] + a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1] + a[..., 3] * b[..., 0]
    return np.stack([w, x, y, z], axis=-1)


def qconj(a):
    return np.asarray(a, dtype=np.float64) * np.array([1.0, -1.0, -1.0, -1.0])


def qcanonical(q):
    q = np.asarray(q, dtype=np.float64)
    s = np.where(q[..., :1] < 0.0, -1.0, 1.0) / np.linalg.norm(q, axis=-1, keepdims=True)
    return q * s


def qlog(q):
    q = np.asarray(q, dtype=np.float64)
    q = q * np.where(q[..., :1] < 0.0, -1.0, 1.0)
    s = np.linalg.norm(q[..., 1:], axis=-1)
    k = np.where(s > 1e-12, 2.0 * np.arctan2(s, q[..., 0]) / np.where(s > 1e-12, s, 1.0), 2.0)
    return q[..., 1:] * k[..., None]


def qexp(om):
    om = np.asarray(om, dtype=np.float64)
    th = np.linalg.norm(om, axis=-1)
    big = th > 1e-12
    k = np.where(big, np.sin(0.5 * th) / np.where(big, th, 1.0), 0.5)
    return np.concatenate([np.where(big, np.cos(0.5 * th), 1.0)[..., None], om * k[..., None]], axis=-1)


def qrot(q):
    """Rotation matrices (..., 3, 3) of unit quaternions, COLMAP's convention."""
    q = np.asarray(q, dtype=np.float64)
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    w, a, b, c = (q[..., k] for k in range(4))
    R = np.stack([1 - 2 * (b * b + c * c), 2 * (a * b - w * c), 2 * (a * c + w * b),
                  2 * (a * b + w * c), 1 - 2 * (a * a + c * c), 2 * (b * c - w * a),
                  2 * (a * c - w * b), 2 * (b * c + w * a), 1 - 2 * (a * a + b * b)], axis=-1)
    return R.reshape(q.shape[:-1] + (3, 3))


def rotmat_to_qvec(R):
    """One 3 x 3 rotation -> unit quaternion with w >= 0."""
    from pixsfm_amd.synthetic import rotmat_to_qvec as impl
    return qcanonical(impl(np.asarray(R, dtype=np.float64)))


# ---- rotation averaging -----------------------------------------------------------------------------------------------------------
def rotation_averaging_reference(n_images, pair_image, pair_qvec, pair_weight, l1_iterations=20, max_iterations=40, min_angle=1e-3,
                                 sigma=5.0, tolerance=1e-10):
    """dict(qvec, root, iterations, pair_angle), or None where the C entry point returns PXR_EINVAL for the graph (images not
    connected to the root over pairs of positive weight)."""
    n = int(n_images)
    pim = np.asarray(pair_image, dtype=np.int64).reshape(-1, 2)
    w = np.asarray(pair_weight, dtype=np.float64).reshape(-1)
    pq = np.asarray(pair_qvec, dtype=np.float64).reshape(-1, 4)
    pq = pq / np.linalg.norm(pq, axis=1, keepdims=True)
    P = len(pim)
    sum_w = np.zeros(n)
    for p in range(P):                     # in pair order, i before j: the order of the host code
        sum_w[pim[p, 0]] += w[p]
        sum_w[pim[p, 1]] += w[p]
    root = int(np.argmax(sum_w))           # the first of equals
    q = np.zeros((n, 4))
    q[root, 0] = 1.0
    in_tree = np.zeros(n, bool)
    in_tree[root] = True
    for _ in range(n - 1):
        leaves = (in_tree[pim[:, 0]] != in_tree[pim[:, 1]]) & (w > 0.0) if P else np.zeros(0, bool)
        if not leaves.any():
            return None
        best = int(np.argmax(np.where(leaves, w, -1.0)))          # the lowest index of equals
        i, j = pim[best]
        if in_tree[i]:
            q[j] = qcanonical(qmul(pq[best], q[i]))
            in_tree[j] = True
        else:
            q[i] = qcanonical(qmul(qconj(pq[best]), q[j]))
            in_tree[i] = True
    m = n - 1
    sig = np.radians(sigma)
    iterations = 0
    for it in range(max_iterations if m > 0 else 0):
        e = qlog(qmul(qmul(qconj(q[pim[:, 1]]), pq), q[pim[:, 0]]))
        th = np.linalg.norm(e, axis=1)
        rho = w / np.maximum(th, min_angle) if it < l1_iterations else w / (1.0 + (th / sig) ** 2)
        L, b = np.zeros((n, n)), np.zeros((n, 3))
        np.add.at(L, (pim[:, 0], pim[:, 0]), rho)
        np.add.at(L, (pim[:, 1], pim[:, 1]), rho)
        np.add.at(L, (pim[:, 0], pim[:, 1]), -rho)
        np.add.at(L, (pim[:, 1], pim[:, 0]), -rho)
        np.add.at(b, pim[:, 1], rho[:, None] * e)
        np.add.at(b, pim[:, 0], -rho[:, None] * e)
        keep = np.arange(n) != root
        om = np.zeros((n, 3))
        om[keep] = np.linalg.solve(L[np.ix_(keep, keep)], b[keep])
        q[keep] = qcanonical(qmul(q[keep], qexp(om[keep])))
        iterations = it + 1
        if it >= l1_iterations and np.linalg.norm(om, axis=1).max() < tolerance:
            break
    angle = np.linalg.norm(qlog(qmul(qmul(qconj(q[pim[:, 1]]), pq), q[pim[:, 0]])), axis=1) if P else np.zeros(0)
    return dict(qvec=q, root=root, iterations=iterations, pair_angle=angle)


# ---- global positioning -----------------------------------------------------------------------------------------------------------
def world_rays(scene, qvec):
    """(unit rays (n_obs, 3), ok (n_obs,)) of the observations under the rotations qvec; pinhole models only."""
    img = np.asarray(scene["obs_image"], dtype=np.int64)
    cam = np.asarray(scene["image_camera"], dtype=np.int64)[img]
    model = np.asarray(scene["cam_model"], dtype=np.int64)[cam]
    assert np.isin(model, (0, 1)).all(), "the reference undistorts SIMPLE_PINHOLE and PINHOLE only"
    k = np.asarray(scene["cam_params"], dtype=np.float64).reshape(len(scene["cam_model"]), -1)
    k = np.concatenate([k, np.zeros((len(k), 4))], axis=1)[cam]
    simple = model == 0
    fx, fy = k[:, 0], np.where(simple, k[:, 0], k[:, 1])
    cx, cy = np.where(simple, k[:, 1], k[:, 2]), np.where(simple, k[:, 2], k[:, 3])
    xy = np.asarray(scene["obs_xy"], dtype=np.float64).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        u, v = (xy[:, 0] - cx) / fx, (xy[:, 1] - cy) / fy
        inv = 1.0 / np.sqrt(u * u + v * v + 1.0)
        R = qrot(qvec)[img]
        d = (R[:, 0, :] * u[:, None] + R[:, 1, :] * v[:, None] + R[:, 2, :]) * inv[:, None]
    ok = np.isfinite(d).all(axis=1)
    return np.where(ok[:, None], d, 0.0), ok


def _adjugate_inverse(A):
    """(inverse by the adjugate, determinant) of symmetric 3 x 3 matrices (T, 3, 3): the formula of the kernel."""
    s0, s1, s2, s3, s4, s5 = A[:, 0, 0], A[:, 0, 1], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2], A[:, 2, 2]
    c00, c01, c02 = s3 * s5 - s4 * s4, s2 * s4 - s1 * s5, s1 * s4 - s2 * s3
    c11, c12, c22 = s0 * s5 - s2 * s2, s1 * s2 - s0 * s4, s0 * s3 - s1 * s1
    det = s0 * c00 + s1 * c01 + s2 * c02
    adj = np.stack([c00, c01, c02, c01, c11, c12, c02, c12, c22], axis=-1).reshape(-1, 3, 3)
    return adj, det


def _robust(d, v, sigma, cheirality):
    n2 = (v * v).sum(axis=1)
    dv = (d * v).sum(axis=1)
    pv = v - d * dv[:, None]
    good = (n2 > 0.0) & np.isfinite(n2)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.sqrt((pv * pv).sum(axis=1) / np.where(good, n2, 1.0)) / sigma
    w = np.where(good, 1.0 / (1.0 + s * s), 0.0)
    if cheirality:
        w = np.where(dv > 0.0, w, 0.0)
    return w


def global_positioning_reference(scene, qvec, pair_image, pair_dir, pair_weight, root, iterations=8, cheirality_from=2, sigma_obs=1.0,
                                 sigma_pair=3.0, min_det=1e-12):
    """dict(centre, xyz (NaN where the status is 1), track_status, obs_weight, pair_weight, status (0 ok / 1 degenerate), rounds)."""
    off = np.asarray(scene["track_offsets"], dtype=np.int64)
    img = np.asarray(scene["obs_image"], dtype=np.int64)
    n, T, N = len(scene["image_camera"]), len(off) - 1, len(img)
    track = np.repeat(np.arange(T), np.diff(off))
    d, ok = world_rays(scene, qvec)
    Pm = np.eye(3)[None] - d[:, :, None] * d[:, None, :]
    pim = np.asarray(pair_image, dtype=np.int64).reshape(-1, 2)
    b = np.asarray(pair_dir, dtype=np.float64).reshape(-1, 3)
    pw = np.asarray(pair_weight, dtype=np.float64).reshape(-1)
    w0 = pw / pw.max() if len(pw) and pw.max() > 0.0 else np.zeros(len(pw))
    Pp = np.eye(3)[None] - b[:, :, None] * b[:, None, :]
    w, robust = ok.astype(np.float64), np.ones(len(pw))
    centre = np.zeros((n, 3))
    keep = np.repeat(np.arange(n) != root, 3)
    so, sp = np.radians(sigma_obs), np.radians(sigma_pair)
    out = dict(centre=centre, xyz=np.full((T, 3), np.nan), track_status=np.ones(T, np.int32), obs_weight=w, pair_weight=w0 * robust,
               status=0, rounds=0)
    r3, c3 = np.meshgrid(np.arange(3), np.arange(3), indexing="ij")
    for it in range(iterations):
        A = np.zeros((T, 3, 3))
        np.add.at(A, track, w[:, None, None] * Pm)
        adj, det = _adjugate_inverse(A)
        valid = det > min_det
        Ainv = np.where(valid[:, None, None], adj / np.where(valid, det, 1.0)[:, None, None], 0.0)
        S = np.zeros((3 * n, 3 * n))
        use = valid[track] & (w > 0.0)
        B = np.where(use[:, None, None], w[:, None, None] * Pm, 0.0)
        np.add.at(S, (3 * img[:, None, None] + r3[None], 3 * img[:, None, None] + c3[None]), B)
        for t in np.flatnonzero(valid):
            o = np.arange(off[t], off[t + 1])
            o = o[use[o]]
            M = np.einsum("aij,jk,bkl->abil", B[o], Ainv[t], B[o])
            rows = 3 * img[o][:, None, None, None] + r3[None, None]
            cols = 3 * img[o][None, :, None, None] + c3[None, None]
            np.subtract.at(S, (np.broadcast_to(rows, M.shape), np.broadcast_to(cols, M.shape)), M)
        wp = w0 * robust
        Bp = wp[:, None, None] * Pp
        for (a, c), sgn in (((0, 0), 1.0), ((1, 1), 1.0), ((0, 1), -1.0), ((1, 0), -1.0)):
            np.add.at(S, (3 * pim[:, a, None, None] + r3[None], 3 * pim[:, c, None, None] + c3[None]), sgn * Bp)
        g = np.zeros((n, 3))
        np.add.at(g, pim[:, 1], wp[:, None] * b)
        np.add.at(g, pim[:, 0], -wp[:, None] * b)
        g, h = g.reshape(-1), wp.sum()
        if keep.any():
            Sk = S[np.ix_(keep, keep)]
            try:
                np.linalg.cholesky(Sk)
            except np.linalg.LinAlgError:
                out["status"] = 1
                return out
            y = np.linalg.solve(Sk, g[keep])
            gy = g[keep] @ y
            if not (gy > 0.0 and np.isfinite(gy)):
                out["status"] = 1
                return out
            centre = np.zeros(3 * n)
            centre[keep] = h * y / gy
            centre = centre.reshape(n, 3)
        rhs = np.zeros((T, 3))
        np.add.at(rhs, track, np.einsum("aij,aj->ai", B, centre[img]))
        X = np.einsum("tij,tj->ti", Ainv, rhs)
        cheir = it >= cheirality_from
        w = np.where(valid[track] & ok, _robust(d, X[track] - centre[img], so, cheir), 0.0)
        robust = _robust(b, centre[pim[:, 1]] - centre[pim[:, 0]], sp, cheir) if len(pim) else robust
        out.update(centre=centre, xyz=np.where(valid[:, None], X, np.nan), track_status=np.where(valid, 0, 1).astype(np.int32),
                   obs_weight=w, pair_weight=w0 * robust, rounds=it + 1)
    return out


def pair_directions(qvec, pair_image, pair_tvec):
    """b_p = -R_j^t t_p / |t_p|: the baseline direction in the world, parallel to c_j - c_i."""
    t = np.asarray(pair_tvec, dtype=np.float64).reshape(-1, 3)
    t = t / np.linalg.norm(t, axis=1, keepdims=True)
    Rj = qrot(np.asarray(qvec)[np.asarray(pair_image, dtype=np.int64).reshape(-1, 2)[:, 1]])
    return -np.einsum("pji,pj->pi", Rj, t)


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
def _small_rotation(rng, sigma, size=None):
    """Quaternion(s) of a rotation by a normal rotation vector of `sigma` radians per axis."""
    return qexp(rng.normal(0.0, sigma, (3,) if size is None else (size, 3)))


def ring_poses(n_images, rng, wobble=0.1):
    """(qvec, tvec, centres): cameras on a ring of RADIUS in the x-z plane looking at the origin, each with an extra rotation of about
    `wobble` radians per axis."""
    ang = 2.0 * np.pi * np.arange(n_images) / n_images
    c = np.stack([RADIUS * np.cos(ang), np.zeros(n_images), RADIUS * np.sin(ang)], axis=1)
    q = np.zeros((n_images, 4))
    for k in range(n_images):
        z = -c[k] / np.linalg.norm(c[k])
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])           # rows: the camera's axes in the world
        q[k] = qmul(_small_rotation(rng, wobble), rotmat_to_qvec(R))
    q = qcanonical(q)
    t = -np.einsum("kij,kj->ki", qrot(q), c)
    return q, t, c


def project(q, t, X):
    x = np.einsum("kij,kj->ki", qrot(q), X) + t
    return np.stack([FOCAL * x[:, 0] / x[:, 2] + WIDTH / 2, FOCAL * x[:, 1] / x[:, 2] + HEIGHT / 2], axis=1)


def noisy_pairs(rng, q, c, pairs, rot_noise_deg=0.1, dir_noise_deg=1.0, outlier_share=0.1):
    """(pair_qvec, pair_tvec, pair_weight, is_outlier) of the pairs (P, 2) under the ground truth (q, c): R_p = R_j R_i^t with
    rot_noise_deg per axis, the baseline direction with dir_noise_deg per axis, outlier_share of the pairs replaced by a uniformly
    random rotation and direction, weights uniform in [50, 200]."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    P = len(pairs)
    i, j = pairs[:, 0], pairs[:, 1]
    pq = qmul(_small_rotation(rng, np.radians(rot_noise_deg), P), qmul(q[j], qconj(q[i])))
    base = c[j] - c[i]
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    base = np.einsum("pij,pj->pi", qrot(_small_rotation(rng, np.radians(dir_noise_deg), P)), base)
    pt = -np.einsum("pij,pj->pi", qrot(q[j]), base)              # t_p with b_p = -R_j^t t_p
    weight = rng.uniform(50.0, 200.0, P)
    bad = np.zeros(P, bool)
    bad[rng.permutation(P)[:int(round(outlier_share * P))]] = True
    rq = rng.normal(size=(P, 4))
    rt = rng.normal(size=(P, 3))
    pq = np.where(bad[:, None], rq / np.linalg.norm(rq, axis=1, keepdims=True), pq)
    pt = np.where(bad[:, None], rt / np.linalg.norm(rt, axis=1, keepdims=True), pt)
    return qcanonical(pq), pt, weight, bad


@functools.lru_cache(maxsize=None)
def ring_scene(n_images, nb, n_points, seed, noise_px=0.5, outlier_obs=0.05, outlier_pairs=0.1):
    """The scene of the issue: a ring of n_images cameras, n_points points uniform in [-2, 2]^3 each seen by nb consecutive images,
    keypoint noise, outlier_obs of the observations replaced by uniformly random image points; pairs between images up to nb - 1
    apart (noisy_pairs).  Arrays are shared between tests: do not write to them."""
    rng = np.random.default_rng(seed)
    q, t, c = ring_poses(n_images, rng)
    X = rng.uniform(-2.0, 2.0, (n_points, 3))
    first = rng.integers(0, n_images, n_points)
    obs_image = ((first[:, None] + np.arange(nb)[None]) % n_images).reshape(-1)
    obs_point = np.repeat(np.arange(n_points), nb)
    xy = project(q[obs_image], t[obs_image], X[obs_point]) + rng.normal(0.0, noise_px, (len(obs_image), 2))
    bad = np.zeros(len(xy), bool)
    bad[rng.permutation(len(xy))[:int(round(outlier_obs * len(xy)))]] = True
    xy = np.where(bad[:, None], rng.uniform(0.0, 1.0, xy.shape) * [WIDTH, HEIGHT], xy)
    pairs = np.array([(i, (i + k) % n_images) for k in range(1, nb) for i in range(n_images)], np.int32)
    pq, pt, pw, pbad = noisy_pairs(rng, q, c, pairs, outlier_share=outlier_pairs)
    return dict(track_offsets=np.arange(0, len(xy) + 1, nb, dtype=np.int64), obs_image=obs_image.astype(np.int32), obs_xy=xy,
                obs_is_outlier=bad, image_camera=np.zeros(n_images, np.int32), cam_model=np.array([0], np.int32),
                cam_params=np.array([[FOCAL, WIDTH / 2, HEIGHT / 2]]), qvec_gt=q, tvec_gt=t, centre_gt=c, xyz_gt=X,
                pair_image=pairs, pair_qvec=pq, pair_tvec=pt, pair_weight=pw, pair_is_outlier=pbad)


BOUNDARY_LENGTHS = (2, 3, 15, 16, 17, 33, 300)


@functools.lru_cache(maxsize=None)
def boundary_batch(n_images, seed=11):
    """One scene that meets every edge of the kernels at once, over n_images ring cameras: tracks of 2, 3, 15, 16, 17, 33 and 300
    observations (the 16-lane group and its strides; longer than the ring, so images repeat inside them), sixty tracks of six, a
    track seen twice by one image, a track of three parallel rays (one keypoint of one image three times, so that they are parallel under any rotations), a NaN keypoint and one far outside the image, pairs of zero weight
    and duplicate pairs, and a last image that has pairs but no observation.  Returns the scene dict of ring_scene plus `special`
    (indices of the named tracks / observations).  Do not write to the arrays."""
    rng = np.random.default_rng(seed)
    q, t, c = ring_poses(n_images, rng)
    seen = n_images - 1                                            # the last image observes nothing
    tracks, points = [], []
    for L in BOUNDARY_LENGTHS + (6,) * 60:
        s = int(rng.integers(0, seen))
        tracks.append([(s + k) % seen for k in range(L)])
        points.append(rng.uniform(-2.0, 2.0, 3))
    twice = len(tracks)
    tracks.append([1, 1, 2, 3])
    points.append(rng.uniform(-2.0, 2.0, 3))
    parallel = len(tracks)
    tracks.append([2, 2, 2])                                       # one ray three times: parallel whatever the rotations are
    points.append(None)
    obs_image = np.concatenate(tracks).astype(np.int32)
    off = np.concatenate([[0], np.cumsum([len(x) for x in tracks])]).astype(np.int64)
    xy = np.zeros((len(obs_image), 2))
    direction = np.array([0.05, 0.02, -1.0]) / np.linalg.norm([0.05, 0.02, -1.0])
    for k, (tr, X) in enumerate(zip(tracks, points)):
        sl = slice(off[k], off[k + 1])
        if X is None:                                              # the image of the point at infinity along `direction`
            r = np.einsum("kij,j->ki", qrot(q[tr]), direction)
            xy[sl] = np.stack([FOCAL * r[:, 0] / r[:, 2] + WIDTH / 2, FOCAL * r[:, 1] / r[:, 2] + HEIGHT / 2], axis=1)
        else:
            xy[sl] = project(q[tr], t[tr], np.tile(X, (len(tr), 1))) + rng.normal(0.0, 0.5, (len(tr), 2))
    nan_obs, far_obs = int(off[10]) + 2, int(off[12]) + 1          # members of two tracks of six
    xy[nan_obs] = np.nan
    xy[far_obs] = [-5000.0, 9000.0]
    pairs = np.array([(i, (i + k) % n_images) for k in (1, 2, 3) for i in range(n_images)] + [(k, k + 1) for k in range(5)], np.int32)
    pq, pt, pw, pbad = noisy_pairs(rng, q, c, pairs, outlier_share=0.05)
    pw[n_images:2 * n_images:7] = 0.0                              # zero weights among the pairs two apart: the ring stays connected
    return dict(track_offsets=off, obs_image=obs_image, obs_xy=xy, image_camera=(np.arange(n_images) % 2).astype(np.int32),
                cam_model=np.array([0, 1], np.int32), cam_params=np.array([[FOCAL, WIDTH / 2, HEIGHT / 2, 0.0], [FOCAL, FOCAL, WIDTH / 2, HEIGHT / 2]]),
                qvec_gt=q, tvec_gt=t, centre_gt=c, pair_image=pairs, pair_qvec=pq, pair_tvec=pt, pair_weight=pw, pair_is_outlier=pbad,
                special=dict(twice=twice, parallel=parallel, nan_obs=nan_obs, far_obs=far_obs, empty_image=n_images - 1))


POSITIONING_SIZES = (22, 23, 65)       # 3 (n - 1) = 63, 66, 192: the Cholesky's 64-column block edge
LAPLACIAN_SIZES = (64, 65, 66)         # n - 1 = 63, 64, 65


@functools.lru_cache(maxsize=None)
def solved(name, n_images=None):
    """(scene, rotation-averaging reference, pair directions under its rotations, positioning reference) of ring_scene(**SCENES[name])
    or, with name "boundary", of boundary_batch(n_images): computed once, shared, read-only."""
    scene = boundary_batch(n_images) if name == "boundary" else ring_scene(**SCENES[name])
    ra = rotation_averaging_reference(len(scene["image_camera"]), scene["pair_image"], scene["pair_qvec"], scene["pair_weight"])
    b = pair_directions(ra["qvec"], scene["pair_image"], scene["pair_tvec"])
    gp = global_positioning_reference(scene, ra["qvec"], scene["pair_image"], b, scene["pair_weight"], ra["root"])
    return scene, ra, b, gp


# ---- the low-parallax ring of the mapper tests ----------------------------------------------------------------------------------------
def initial_pair_candidates(scene, min_num_inliers=100, min_tri_angle=16.0):
    """The image pairs of a mapping_cases.ring_scene that pass IncrementalMapper's initial-pair criteria under ground truth: at
    least min_num_inliers common points seen under a median angle of at least min_tri_angle degrees (host numpy)."""
    from pixsfm_amd.api.mapping import median_triangulation_angle
    from pixsfm_amd.synthetic import qvec_to_rotmat
    names, out = scene["names"], []
    centre = {nm: -qvec_to_rotmat(scene["poses"][nm][0]).T @ scene["poses"][nm][1] for nm in names}
    for a in range(len(names)):
        for b in range(a + 1, len(names)):
            common = np.intersect1d(scene["owner"][names[a]], scene["owner"][names[b]])
            common = common[common >= 0]
            if len(common) >= min_num_inliers and median_triangulation_angle(scene["X"][common], centre[names[a]], centre[names[b]]) >= min_tri_angle:
                out.append((names[a], names[b]))
    return out


@functools.lru_cache(maxsize=None)
def low_parallax_ring(n_points=600, seed=0):
    """The smallest ring (in steps of ten images, mapping_cases.ring_scene, six views per point) on which no pair passes the
    initial-pair criteria: (scene, n_images)."""
    import mapping_cases as mc
    for n_images in range(20, 101, 10):
        scene = mc.ring_scene(n_images=n_images, n_points=n_points, seed=seed)
        if not initial_pair_candidates(scene):
            return scene, n_images
    raise AssertionError("no ring up to 100 images defeats the initial-pair criteria")


# ---- errors against ground truth --------------------------------------------------------------------------------------------------
def rotation_errors_deg(qvec, qvec_gt, root):
    """Angle between R_k and R_k^gt R_root^gt^t (the estimate's world frame is the root's camera frame) per image, degrees."""
    rel = qmul(qvec_gt, qconj(qvec_gt[root])[None])
    return np.degrees(np.linalg.norm(qlog(qmul(qvec, qconj(rel))), axis=1))


def similarity_align(src, dst):
    """src mapped onto dst by the least-squares similarity (Umeyama): (aligned src, scale, R, t)."""
    ms, md = src.mean(axis=0), dst.mean(axis=0)
    a, b = src - ms, dst - md
    U, sv, Vt = np.linalg.svd(b.T @ a / len(src))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    R = U @ D @ Vt
    s = (sv * np.diag(D)).sum() / (a * a).sum() * len(src)
    return s * src @ R.T + (md - s * R @ ms), s, R, md - s * R @ ms


# ---- comparisons the lane and GPU tests share ----------------------------------------------------------------------------------
def untouched(out):
    return all((np.asarray(v) == -9).all() for v in out.values())


def compare_rotavg(got, ref, show=print):
    """The differences {key: max abs}; integer outputs asserted equal."""
    assert got["root"] == ref["root"] and got["iterations"] == ref["iterations"], (got["root"], got["iterations"], ref["root"], ref["iterations"])
    diff = dict(qvec=float(np.abs(got["qvec"] - ref["qvec"]).max()), pair_angle=float(np.abs(got["pair_angle"] - ref["pair_angle"]).max()))
    show("rotation averaging: " + ", ".join("%s %.3e" % kv for kv in diff.items()))
    return diff


def compare_positioning(got, ref, show=print):
    assert got["status"] == ref["status"] == 0 and got["rounds"] == ref["rounds"]
    assert np.array_equal(got["track_status"], ref["track_status"])
    ok = ref["track_status"] == 0
    assert (got["xyz"][~ok] == -9).all(), "a point was written for a track of status 1"
    assert np.array_equal(got["obs_weight"] == 0.0, ref["obs_weight"] == 0.0), "the rejected observations differ"
    assert np.array_equal(got["pair_weight"] == 0.0, ref["pair_weight"] == 0.0), "the rejected pairs differ"
    diff = dict(centre=float(np.abs(got["centre"] - ref["centre"]).max()), xyz=float(np.abs(got["xyz"][ok] - ref["xyz"][ok]).max()),
                obs_weight=float(np.abs(got["obs_weight"] - ref["obs_weight"]).max()),
                pair_weight=float(np.abs(got["pair_weight"] - ref["pair_weight"]).max()))
    show("global positioning: " + ", ".join("%s %.3e" % kv for kv in diff.items()))
    return diff


def within_bounds(diff):
    for k, v in diff.items():
        assert v <= bound(k), "%s differs by %.3e, bound %.3e" % (k, v, bound(k))


# ---- bad inputs ---------------------------------------------------------------------------------------------------------------------
def bad_rotation_inputs(scene):
    """(name, key, replacement array, word of the error message) per class of PXR_EINVAL of pxr_rotation_averaging."""
    n, pim, pq, pw = len(scene["image_camera"]), scene["pair_image"], scene["pair_qvec"], scene["pair_weight"]

    def put(a, idx, v):
        a = np.array(a, copy=True)
        a[idx] = v
        return a
    half = np.array([(i, i + 1) for i in range(n // 2 - 1)] + [(i, i + 1) for i in range(n // 2, n - 1)], np.int32)
    return [("pair index", "pair_image", put(pim, (3, 1), n), "outside"), ("negative index", "pair_image", put(pim, (0, 0), -1), "outside"),
            ("self pair", "pair_image", put(pim, 2, pim[2, 0]), "itself"), ("negative weight", "pair_weight", put(pw, 1, -1.0), "weight"),
            ("NaN weight", "pair_weight", put(pw, 4, np.nan), "weight"), ("zero qvec", "pair_qvec", put(pq, 5, 0.0), "qvec"),
            ("NaN qvec", "pair_qvec", put(pq, (6, 2), np.nan), "qvec"), ("two components", "pair_image", half, "not connected")]


def bad_positioning_inputs(scene, pair_dir):
    """(name, key, replacement, word) per class of PXR_EINVAL of pxr_global_positioning; key "root" replaces the root."""
    n, off, img = len(scene["image_camera"]), scene["track_offsets"], scene["obs_image"]
    pim, pw = scene["pair_image"], scene["pair_weight"]

    def put(a, idx, v):
        a = np.array(a, copy=True)
        a[idx] = v
        return a
    return [("offsets not monotone", "track_offsets", put(off, 3, off[5]), "monotone"), ("offsets end", "track_offsets", put(off, -1, off[-1] - 1), "ends at"),
            ("offsets start", "track_offsets", put(off, 0, 1), "not 0"),
            ("image index", "obs_image", put(img, 7, n), "image outside"), ("camera index", "image_camera", put(scene["image_camera"], 2, 2), "camera outside"),
            ("pair index", "pair_image", put(pim, (3, 0), n), "pair 3 names"), ("self pair", "pair_image", put(pim, 2, pim[2, 1]), "itself"),
            ("NaN direction", "pair_dir", put(pair_dir, (1, 1), np.nan), "unit vector"), ("long direction", "pair_dir", put(pair_dir, 4, 2.0 * pair_dir[4]), "unit vector"),
            ("negative weight", "pair_weight", put(pw, 1, -1.0), "weight"), ("infinite weight", "pair_weight", put(pw, 0, np.inf), "weight"),
            ("root", "root", n, "root"), ("negative root", "root", -1, "root")]
