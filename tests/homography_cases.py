"""Helper of the homography tests (not collected): a numpy reference of the per-pair estimator, written from its specification
(include/pixsfm_hip.h) and not from the kernel, and generators of planar, rotation-only and general image pairs.

    samples   twoview_cases.sample with k = 4: the hash of section 19, four distinct indices in ascending order
    solver    the 8 x 9 DLT system, null vector by Gauss-Jordan with full pivoting, Frobenius norm 1, third components positive
    score     squared forward transfer error in the normalised plane of image 2 (+inf behind), inlier iff err <= thr^2;
              key (count, -sum min(err, thr^2), -h)
    stop      after every round: samples done >= clamp(log(1 - confidence) / log(1 - w^4), min_num_trials, max_num_trials),
              w = max(best count, need) / n capped at 1 -- the floor `need` is what ends a pair without a homography
    LO        Levenberg-Marquardt on the inliers' transfer residuals over the eight entries beside the largest, re-normalise,
              classify, repeat
    rotation  H with det > 0 -> Gram-Schmidt on its rows -> quaternion -> Levenberg-Marquardt over three parameters -> count

The solver runs on all samples of a round at once (arrays with a leading sample axis): every element sees the operations the
specification states, in its order, so a sample's numbers do not depend on the round it is in.
"""
import functools

import numpy as np

import abspose_cases as ac
import pxo
import triangulation_cases as tc
import twoview_cases as tv
from pixsfm_amd import synthetic

DEFAULTS = dict(tv.DEFAULTS)
LDS_MATCHES = tv.LDS_MATCHES
IMAGE = tv.IMAGE
PIVOT_TOL, ROW_TOL = 1e-12, 1e-12

sample = functools.partial(tv.sample, k=4)       # (tv.sample is abspose_cases.sample with k = 5 preset; k = 4 here)


def need_inliers(o, n):
    return max(o["min_num_inliers"], int(np.ceil(o["min_inlier_ratio"] * n)))


def trials_needed(o, max_trials, cnt, n):
    """tv.trials_needed's clamp for samples of four, at no fewer inliers than the success rule asks for: w = max(cnt, need) / n
    capped at 1, all-inlier probability (w w) (w w)."""
    eff = max(cnt, need_inliers(o, n))
    need = float(max_trials)
    if eff > 0:
        w = min(eff / n, 1.0)
        with np.errstate(all="ignore"):
            x = np.log(1.0 - o["confidence"]) / np.log(1.0 - (w * w) * (w * w))
        if x < need:
            need = x
    return min(max(need, float(o["min_num_trials"])), float(max_trials))


# ---- the four-point solver --------------------------------------------------------------------------------------------------------
def four_point(rec):
    """rec (B, 4, 4): the records (x1, y1, x2, y2) of B samples.  Returns (H (B, 9), ok (B,))."""
    rec = np.asarray(rec, dtype=np.float64)
    B = len(rec)
    ar = np.arange(B)
    with np.errstate(all="ignore"):
        x1, y1, x2, y2 = (rec[:, :, m] for m in range(4))
        zero, one = np.zeros_like(x1), np.ones_like(x1)
        even = np.stack([zero, zero, zero, -x1, -y1, -one, y2 * x1, y2 * y1, y2], 2)
        odd = np.stack([x1, y1, one, zero, zero, zero, -(x2 * x1), -(x2 * y1), -x2], 2)
        A = np.stack([even, odd], 2).reshape(B, 8, 9)
        S = np.abs(A).reshape(B, -1).max(1)
        ok = np.isfinite(S)
        perm = np.tile(np.arange(9), (B, 1))
        for c in range(8):
            blk = np.abs(A[:, c:, c:]).reshape(B, -1)
            at = np.argmax(blk, 1)                       # row-major, the first of equals
            pr, pc = c + at // (9 - c), c + at % (9 - c)
            ok &= blk[ar, at] > PIVOT_TOL * S
            tmp = A[ar, c, :].copy(); A[ar, c, :] = A[ar, pr, :]; A[ar, pr, :] = tmp
            tmp = A[ar, :, c].copy(); A[ar, :, c] = A[ar, :, pc]; A[ar, :, pc] = tmp
            tmp = perm[ar, c].copy(); perm[ar, c] = perm[ar, pc]; perm[ar, pc] = tmp
            p = A[:, c, c].copy()
            A[:, c, c:] = A[:, c, c:] / p[:, None]
            f = A[:, :, c].copy()
            f[:, c] = 0.0
            A[:, :, c + 1:] = A[:, :, c + 1:] - f[:, :, None] * A[:, None, c, c + 1:]
            A[:, :, c] = 0.0
            A[:, c, c] = 1.0
        v = np.zeros((B, 9))
        for r in range(8):
            v[ar, perm[:, r]] = -A[:, r, 8]
        v[ar, perm[:, 8]] = 1.0
        d = np.zeros(B)
        for m in range(9):
            d = d + v[:, m] * v[:, m]
        nrm = np.sqrt(d)
        ok &= (nrm > 0.0) & np.isfinite(nrm)
        H = v / nrm[:, None]
        w = (H[:, 6, None] * x1 + H[:, 7, None] * y1) + H[:, 8, None]
        pos, neg = (w > 0.0).all(1), (w < 0.0).all(1)
        H = np.where(neg[:, None], -H, H)
        ok &= pos | neg
    return H, ok


def transfer(H, rec):
    """Squared forward transfer error of records rec (n, 4) under H (.., 9): (.., n); +inf where the third component is <= 0."""
    H = np.asarray(H)[..., None, :]
    x1, y1 = rec[:, 0], rec[:, 1]
    with np.errstate(all="ignore"):
        X = (H[..., 0] * x1 + H[..., 1] * y1) + H[..., 2]
        Y = (H[..., 3] * x1 + H[..., 4] * y1) + H[..., 5]
        W = (H[..., 6] * x1 + H[..., 7] * y1) + H[..., 8]
        dx, dy = X / W - rec[:, 2], Y / W - rec[:, 3]
        return np.where(W <= 0.0, np.inf, dx * dx + dy * dy)


# ---- refinement ----------------------------------------------------------------------------------------------------------------------
def h_residuals(H, rec):
    """(n, 2) residuals pi(H x1) - x2, or None where a third component is not positive."""
    x1h = np.concatenate([rec[:, :2], np.ones((len(rec), 1))], 1)
    p = x1h @ np.asarray(H).reshape(3, 3).T
    if not ((p[:, 2] > 0.0) & np.isfinite(p[:, 2])).all():
        return None
    return p[:, :2] / p[:, 2:] - rec[:, 2:]


def h_jacobian(H, rec):
    """d residuals / d H: (n, 2, 9), analytic."""
    x1h = np.concatenate([rec[:, :2], np.ones((len(rec), 1))], 1)
    p = x1h @ np.asarray(H).reshape(3, 3).T
    a = x1h / p[:, 2:]
    px, py = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
    J = np.zeros((len(rec), 2, 9))
    J[:, 0, 0:3], J[:, 0, 6:9] = a, -px[:, None] * a
    J[:, 1, 3:6], J[:, 1, 6:9] = a, -py[:, None] * a
    return J


def rot_residuals(q, rec):
    return h_residuals(synthetic.qvec_to_rotmat(q).reshape(9), rec)


def rot_jacobian(q, rec):
    """d residuals / d (rotation tangent) at zero, R(d) = R(2 d) R: (n, 2, 3), analytic."""
    x1h = np.concatenate([rec[:, :2], np.ones((len(rec), 1))], 1)
    p = x1h @ synthetic.qvec_to_rotmat(q).T
    px, py, iw = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2], 1.0 / p[:, 2]
    J = np.zeros((len(rec), 2, 3))
    for c in range(3):
        dp = 2.0 * np.cross(np.eye(3)[c], p)
        J[:, 0, c] = (dp[:, 0] - px * dp[:, 2]) * iw
        J[:, 1, c] = (dp[:, 1] - py * dp[:, 2]) * iw
    return J


def quat_plus(q, d):
    return ac.pose_plus(np.asarray(q, dtype=np.float64), np.zeros(3), np.concatenate([d, np.zeros(3)]))[0]


def lm(x, sums, plus, o):
    """Levenberg-Marquardt with the lambda schedule and the keep / refuse rule of section 19: sums(x) -> (JtJ, Jtr, cost)."""
    H, g, cost = sums(x)
    if not np.isfinite(cost):
        return x
    lam = 1e-4
    for _ in range(o["refine_max_iterations"]):
        try:
            L = np.linalg.cholesky(H + lam * np.diag(np.diag(H)))
            d = -np.linalg.solve(L.T, np.linalg.solve(L, g))
            ok = bool(np.isfinite(d).all())
        except np.linalg.LinAlgError:
            ok = False
        if not ok:
            lam *= 10.0
            if lam > 1e12:
                break
            continue
        x1 = plus(x, d)
        H1, g1, cost1 = sums(x1)
        if cost1 <= cost + 1e-12 * cost:
            x, H, g, cost = x1, H1, g1, cost1
            lam = max(lam * 0.1, 1e-12)
        else:
            lam *= 10.0
            if lam > 1e12:
                break
        if np.linalg.norm(d) <= 1e-12:
            break
    return x


def _sums(res, jac):
    def sums(x):
        r = res(x)
        if r is None:
            return None, None, np.inf
        J = jac(x).reshape(2 * len(r), -1)
        r = r.reshape(-1)
        return J.T @ J, J.T @ r, float(r @ r)
    return sums


def refine_h(H, rec, o):
    """One refinement of a unit-norm H on the records given (the inliers); returns it re-normalised."""
    fixed = int(np.argmax(np.abs(H)))                    # the first of equals
    free = [m for m in range(9) if m != fixed]

    def plus(x, d):
        x1 = x.copy()
        x1[free] = x[free] + d
        return x1
    H1 = lm(np.array(H, dtype=np.float64), _sums(lambda x: h_residuals(x, rec), lambda x: h_jacobian(x, rec)[:, :, free]), plus, o)
    return H1 / np.sqrt(np.cumsum(H1 * H1)[-1])


def rotation_of(H):
    """R0 of H: its sign chosen so that det >= 0, modified Gram-Schmidt on the rows (row 0, row 1, their cross product); None
    where a row's norm is <= ROW_TOL."""
    G = np.asarray(H, dtype=np.float64).reshape(3, 3)
    if np.linalg.det(G) < 0.0:
        G = -G
    n0 = np.sqrt(G[0] @ G[0])
    if not n0 > ROW_TOL:
        return None
    r0 = G[0] / n0
    g1 = G[1] - (G[1] @ r0) * r0
    n1 = np.sqrt(g1 @ g1)
    if not n1 > ROW_TOL:
        return None
    r1 = g1 / n1
    return np.stack([r0, r1, np.cross(r0, r1)])


def refine_rot(q, rec, o):
    return lm(np.array(q, dtype=np.float64), _sums(lambda x: rot_residuals(x, rec), lambda x: rot_jacobian(x, rec)), quat_plus, o)


# ---- the estimator -----------------------------------------------------------------------------------------------------------------
def estimate(xy1, xy2, cam1, cam2, **options):
    """The estimator on one pair; cam = (model, params).  Returns dict(status, H, rot_qvec, n_inliers, n_rot_inliers, n_trials,
    inlier (n,), err (n,), usable (n,))."""
    o = {**DEFAULTS, **options}
    xy1, xy2 = np.asarray(xy1, dtype=np.float64).reshape(-1, 2), np.asarray(xy2, dtype=np.float64).reshape(-1, 2)
    k1, k2 = tv._params(*cam1), tv._params(*cam2)
    N = len(xy1)
    uv1, ok1 = ac.image_to_world(cam1[0], k1, xy1)
    uv2, ok2 = ac.image_to_world(cam2[0], k2, xy2)
    usable = ok1 & ok2 & np.isfinite(xy1).all(1) & np.isfinite(xy2).all(1)
    out = dict(status=1, H=None, rot_qvec=None, n_inliers=0, n_rot_inliers=0, n_trials=0, inlier=np.zeros(N, np.uint8),
               err=np.full(N, np.nan), usable=usable)
    idx = np.flatnonzero(usable)
    n = len(idx)
    if n < 4:
        return out
    rec = np.concatenate([uv1[idx], uv2[idx]], 1)
    thr = o["max_error"] / ac.mean_focal(cam2[0], k2)
    thr2 = thr * thr
    max_trials = -(-o["max_num_trials"] // o["round_size"]) * o["round_size"]
    best, done = None, 0
    while True:
        hs = list(range(done, done + o["round_size"]))
        H, valid = four_point(rec[[list(sample(o["seed"], h, n)) for h in hs]])
        err = transfer(H, rec)                                              # (B, n)
        with np.errstate(invalid="ignore"):
            inl = err <= thr2
        cnt = inl.sum(1)
        tot = np.cumsum(np.where(inl, err, thr2), 1)[:, -1]                 # (cumsum: the sum in index order)
        for b in np.flatnonzero(valid):
            key = (int(cnt[b]), -float(tot[b]), -hs[b])
            if best is None or key > best[0]:
                best = (key, H[b].copy())
        done += o["round_size"]
        if done >= max_trials or done >= trials_needed(o, max_trials, best[0][0] if best else -1, n):
            break
    out["n_trials"] = done
    if best is None:
        out["status"] = 2
        return out
    H = best[1]
    with np.errstate(invalid="ignore"):
        cur = transfer(H, rec) <= thr2
    cur_cnt = int(cur.sum())
    for _ in range(o["lo_rounds"]):
        H1 = refine_h(H, rec[cur], o)
        with np.errstate(invalid="ignore"):
            new = transfer(H1, rec) <= thr2
        if new.sum() < cur_cnt:
            break
        changed = bool((new != cur).any())
        H, cur, cur_cnt = H1, new, int(new.sum())
        if not changed:
            break
    out["status"] = 3
    if cur_cnt < need_inliers(o, n):
        return out
    e2 = transfer(H, rec)
    out.update(status=0, H=H, n_inliers=cur_cnt)
    out["inlier"][idx] = cur
    with np.errstate(invalid="ignore"):
        out["err"][idx] = np.where(np.isfinite(e2), np.sqrt(e2) * (o["max_error"] / thr), np.nan)
    R0 = rotation_of(H)
    if R0 is not None:
        q = synthetic.rotmat_to_qvec(R0)
        q = refine_rot(q / np.linalg.norm(q), rec[cur], o)
        with np.errstate(invalid="ignore"):
            out["n_rot_inliers"] = int((transfer(synthetic.qvec_to_rotmat(q).reshape(9), rec) <= thr2).sum())
        out["rot_qvec"] = -q if q[0] < 0 else q
    return out


NAMES = ("H", "rot_qvec", "status", "n_inliers", "n_rot_inliers", "n_trials", "inlier", "err")


def reference(batch, **options):
    """The estimator on every pair of a batch (the dict engine.HomographyProblem takes).  Arrays like the kernel's outputs; H /
    rot_qvec are NaN where status is not 0."""
    off = np.asarray(batch["pair_offsets"])
    T = len(off) - 1
    res = dict(H=np.full((T, 9), np.nan), rot_qvec=np.full((T, 4), np.nan), status=np.zeros(T, np.int32), n_inliers=np.zeros(T, np.int32),
               n_rot_inliers=np.zeros(T, np.int32), n_trials=np.zeros(T, np.int32), inlier=np.zeros(off[-1], np.uint8),
               err=np.full(off[-1], np.nan))
    for p in range(T):
        c1, c2 = batch["pair_camera"][p]
        r = estimate(batch["xy1"][off[p]:off[p + 1]], batch["xy2"][off[p]:off[p + 1]], (int(batch["cam_model"][c1]), batch["cam_params"][c1]),
                     (int(batch["cam_model"][c2]), batch["cam_params"][c2]), **options)
        for k in ("status", "n_inliers", "n_rot_inliers", "n_trials"):
            res[k][p] = r[k]
        if r["status"] == 0:
            res["H"][p] = r["H"]
            if r["rot_qvec"] is not None:
                res["rot_qvec"][p] = r["rot_qvec"]
        res["inlier"][off[p]:off[p + 1]] = r["inlier"]
        res["err"][off[p]:off[p + 1]] = r["err"]
    return res


# ---- pairs -------------------------------------------------------------------------------------------------------------------------
def transfer_px(H, cam1, cam2, xy1, xy2):
    """Forward transfer error in pixels (the kernel's d_err) of matches under H (normalised plane)."""
    k1, k2 = tv._params(*cam1), tv._params(*cam2)
    uv1, _ = ac.image_to_world(cam1[0], k1, xy1)
    uv2, _ = ac.image_to_world(cam2[0], k2, xy2)
    return np.sqrt(transfer(np.asarray(H).reshape(9), np.concatenate([uv1, uv2], 1))) * ac.mean_focal(cam2[0], k2)


def make_h_pair(kind, n, cam1, cam2, rng, sigma=0.5, p_outlier=0.3, min_outlier_px=20.0):
    """One pair of n matches that a homography explains.  "planar": camera 1 at the origin looks at a random plane n . X = d at
    depth about 6 with a tilted normal, camera 2 is a tv.random_relative_pose: H = R + t n^t / d.  "rotation": t = 0, depths
    2-12: H = R.  An inlier is the true projection plus Gaussian noise of sigma clipped at 3 sigma, on both sides;
    floor(p_outlier n) matches (none in pairs of fewer than 20, never so many that fewer than 15 inliers remain) are outliers:
    their second pixel is uniform in the image, at a forward transfer error of at least min_outlier_px under the true H (None:
    no condition).
    Returns (xy1, xy2, true_inlier, H (3, 3))."""
    W, Hh = IMAGE
    n = int(n)
    while True:                                            # a pose under which enough of the candidates is seen by both
        q, t = tv.random_relative_pose(rng)
        R = synthetic.qvec_to_rotmat(q)
        if kind == "planar":
            nrm = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), 1.0])
            nrm /= np.linalg.norm(nrm)
            d = rng.uniform(5.0, 7.0) * nrm[2]
            Hm = R + np.outer(t, nrm) / d
        else:
            t = np.zeros(3)
            Hm = R.copy()
        pix1, pix2 = np.zeros((0, 2)), np.zeros((0, 2))
        for _ in range(8):
            if len(pix1) >= n:
                break
            m = 2 * n + 16
            cand = np.stack([rng.uniform(0.05 * W, 0.95 * W, m), rng.uniform(0.05 * Hh, 0.95 * Hh, m)], 1)
            uv, ok = ac.image_to_world(cam1[0], cam1[1], cand)
            assert ok.all()
            x1h = np.concatenate([uv, np.ones((m, 1))], 1)
            depth = d / (x1h @ nrm) if kind == "planar" else rng.uniform(2.0, 12.0, m)
            X2 = (x1h * depth[:, None]) @ R.T + t
            with np.errstate(all="ignore"):
                x, y = ac.world_to_image(cam2[0], cam2[1], X2[:, 0] / X2[:, 2], X2[:, 1] / X2[:, 2])
            seen = (depth > 0.5) & (X2[:, 2] > 0.5) & (x >= 0) & (x <= W) & (y >= 0) & (y <= Hh)
            pix1, pix2 = np.concatenate([pix1, cand[seen]]), np.concatenate([pix2, np.stack([x, y], 1)[seen]])
        if len(pix1) >= n:
            pix1, pix2 = pix1[:n], pix2[:n]
            break
    noise = lambda: np.clip(rng.normal(0, sigma, (n, 2)), -3 * sigma, 3 * sigma) if sigma > 0 else np.zeros((n, 2))
    obs1, obs2 = pix1 + noise(), pix2 + noise()
    bad = np.zeros(n, bool)
    if n >= 20:
        bad[rng.permutation(n)[:min(int(p_outlier * n), n - 15)]] = True
    for j in np.flatnonzero(bad):
        while True:
            c = np.array([rng.uniform(0, W), rng.uniform(0, Hh)])
            if min_outlier_px is None or transfer_px(Hm, cam1, cam2, obs1[j:j + 1], c[None])[0] >= min_outlier_px:
                break
        obs2[j] = c
    return obs1, obs2, ~bad, Hm


def make_pairs(kinds, counts, models, seed, sigma=0.5, p_outlier=0.3, min_outlier=20.0):
    """A batch of pairs: pair i is of kinds[i] ("planar", "rotation" or "general") with counts[i] matches, its first camera
    models[i % L], its second models[(i + 1) % L] (tc.MODEL_PARAMS).  A general pair is tv.make_pairs' (depths 2-12, a baseline,
    outliers at a Sampson distance of at least min_outlier px; None: no condition on either kind of outlier).  Returns the batch dict + kind, true_inlier and gt_H (NaN for general
    pairs; normalised plane, Frobenius norm 1, H[2] . x > 0)."""
    rng = np.random.default_rng(seed)
    L = len(models)
    xy1, xy2, inl, gH = [], [], [], []
    for i, (kind, n) in enumerate(zip(kinds, counts)):
        m1, m2 = int(models[i % L]), int(models[(i + 1) % L])
        if kind == "general":
            g = tv.make_pairs([int(n)], (m1, m2), seed=int(rng.integers(1 << 30)), sigma=sigma, p_outlier=p_outlier,
                              min_outlier_sampson=min_outlier)
            a, b, good, Hm = g["xy1"], g["xy2"], g["true_inlier"], np.full((3, 3), np.nan)
        else:
            cam1, cam2 = ((m, np.array(tc.MODEL_PARAMS[m], dtype=np.float64)) for m in (m1, m2))
            a, b, good, Hm = make_h_pair(kind, n, cam1, cam2, rng, sigma=sigma, p_outlier=p_outlier, min_outlier_px=min_outlier)
            Hm = Hm / np.linalg.norm(Hm)
            Hm = Hm if Hm[2, 2] > 0 else -Hm
        xy1.append(a); xy2.append(b); inl.append(good); gH.append(Hm.reshape(9))
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    cat = lambda parts: np.concatenate(parts).reshape(-1, 2) if len(parts) else np.zeros((0, 2))
    T = len(counts)
    return dict(pair_offsets=off, xy1=cat(xy1), xy2=cat(xy2), pair_camera=np.stack([np.arange(T) % L, (np.arange(T) + 1) % L], 1).astype(np.int32),
                cam_model=np.array(models, np.int32), cam_params=tc.pad_params([tc.MODEL_PARAMS[m] for m in models]),
                kind=list(kinds), gt_H=np.array(gH).reshape(-1, 9), true_inlier=np.concatenate(inl) if len(inl) else np.zeros(0, bool))


single = tv.single


def noise_free_samples(B, seed):
    """B samples of four noise-free matches of a plane in the normalised plane: (rec (B, 4, 4), H (B, 9) unit norm, H[8] > 0)."""
    rng = np.random.default_rng(seed)
    rec, Hs = np.zeros((B, 4, 4)), np.zeros((B, 9))
    for b in range(B):
        q, t = tv.random_relative_pose(rng)
        nrm = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), 1.0])
        nrm /= np.linalg.norm(nrm)
        Hm = synthetic.qvec_to_rotmat(q) + np.outer(t, nrm) / (rng.uniform(5.0, 7.0) * nrm[2])
        x1 = rng.uniform(-0.4, 0.4, (4, 2))
        p = np.concatenate([x1, np.ones((4, 1))], 1) @ Hm.T
        rec[b] = np.concatenate([x1, p[:, :2] / p[:, 2:]], 1)
        Hs[b] = (Hm / np.linalg.norm(Hm)).reshape(9)
    return rec, Hs


# ---- hard families of minimal samples (tests/test_minimal_solvers_*.py) ---------------------------------------------------------
def _sample(rng, x1=None, half_field=0.4, baseline=None, affine=False):
    """Four noise-free matches of a plane: (rec (4, 4), H (9,) unit norm, positive third component on the points).  baseline: the
    length of the translation (None: random_relative_pose's); affine: no rotation out of the image plane, a plane facing the
    camera and a translation within it, so that the last row of H is (0, 0, 1) up to 1e-6."""
    q, t = tv.random_relative_pose(rng)
    nrm = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), 1.0])
    if affine:
        ang = rng.uniform(0.02, 0.25)
        q = np.array([np.cos(0.5 * ang), 1e-6 * rng.uniform(-1, 1), 1e-6 * rng.uniform(-1, 1), np.sin(0.5 * ang)])
        q /= np.linalg.norm(q)
        nrm, t = np.array([0.0, 0.0, 1.0]), t * np.array([1.0, 1.0, 1e-6])
    if baseline is not None:
        t = t / np.linalg.norm(t) * baseline
    nrm = nrm / np.linalg.norm(nrm)
    Hm = synthetic.qvec_to_rotmat(q) + np.outer(t, nrm) / (rng.uniform(5.0, 7.0) * nrm[2])
    if x1 is None:
        x1 = rng.uniform(-half_field, half_field, (4, 2))
    p = np.concatenate([x1, np.ones((4, 1))], 1) @ Hm.T
    return np.concatenate([x1, p[:, :2] / p[:, 2:]], 1), (Hm / np.linalg.norm(Hm)).reshape(9)


def _sliver(rng, off):
    """A quadrilateral whose fourth corner sits `off` from the side of the first two."""
    x1 = rng.uniform(-0.4, 0.4, (4, 2))
    d = x1[1] - x1[0]
    x1[3] = x1[0] + rng.uniform(0.2, 0.8) * d + off * np.array([-d[1], d[0]]) / np.linalg.norm(d)
    return x1


# (No sliver at 1e-7: kappa of H is about 4 / off there, 4e7, which puts 63 of 64 samples beyond the 1e-7 cap on C kappa u; no draw of
# such a quadrilateral keeps it under, so the family would pass with nothing judged.)
HARD_FAMILIES = {
    "generic": _sample,
    "narrow field": lambda rng: _sample(rng, half_field=0.005),
    "translation 1e-4": lambda rng: _sample(rng, baseline=1e-4),
    "sliver 1e-3": lambda rng: _sample(rng, x1=_sliver(rng, 1e-3)),
    "sliver 1e-5": lambda rng: _sample(rng, x1=_sliver(rng, 1e-5)),
    "near-affine": lambda rng: _sample(rng, affine=True),
}


def hard_family(name, seed, B=64):
    """B noise-free samples of a family of HARD_FAMILIES: (rec (B, 4, 4), H (B, 9))."""
    rng = np.random.default_rng(seed)
    parts = [HARD_FAMILIES[name](rng) for _ in range(B)]
    return np.array([p[0] for p in parts]), np.array([p[1] for p in parts])


def degenerate_samples(seed=0):
    """(rec (4, 4, 4)): a repeated match, four points on one line, a coordinate that is not a number, three points on one line."""
    rng = np.random.default_rng(seed)
    rec = np.array([_sample(rng)[0] for _ in range(4)])
    rec[0, 1] = rec[0, 0]
    rec[1, :, 1] = rec[1, :, 0]
    rec[1, :, 2:] = rec[1, :, :2]
    rec[2, 0, 2] = np.nan
    rec[3, 2, :2] = 0.5 * (rec[3, 0, :2] + rec[3, 1, :2])
    rec[3, 2, 2:] = 0.5 * (rec[3, 0, 2:] + rec[3, 1, 2:])
    return rec


def eleven_models_pairs():
    """(batch, gt_H): one noise-free planar pair of 40 matches per camera model, its second camera the next model."""
    models = sorted(tc.MODEL_PARAMS)
    rng = np.random.default_rng(37)
    xy1, xy2, gH = [], [], []
    ident = np.array([1.0, 0, 0, 0])
    for i, m in enumerate(models):
        m2 = models[(i + 1) % len(models)]
        q, t = tv.random_relative_pose(rng)
        nrm = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), 1.0])
        nrm /= np.linalg.norm(nrm)
        d = rng.uniform(5.0, 7.0) * nrm[2]
        x1h = np.concatenate([rng.uniform(-0.3, 0.3, (40, 2)), np.ones((40, 1))], 1)
        X1 = x1h * (d / (x1h @ nrm))[:, None]
        k1, k2 = (np.array(tc.MODEL_PARAMS[x], dtype=np.float64) for x in (m, m2))
        xy1.append(np.array([pxo.world_to_pixel(m, k1, ident, np.zeros(3), x, jac=False)[0] for x in X1]))
        xy2.append(np.array([pxo.world_to_pixel(m2, k2, q, t, x, jac=False)[0] for x in X1]))
        Hm = synthetic.qvec_to_rotmat(q) + np.outer(t, nrm) / d
        gH.append((Hm / np.linalg.norm(Hm)).reshape(9))
    L = len(models)
    batch = dict(pair_offsets=np.arange(L + 1, dtype=np.int64) * 40, xy1=np.concatenate(xy1), xy2=np.concatenate(xy2),
                 pair_camera=np.stack([np.arange(L), (np.arange(L) + 1) % L], 1).astype(np.int32), cam_model=np.array(models, np.int32),
                 cam_params=tc.pad_params([tc.MODEL_PARAMS[m] for m in models]))
    return batch, np.array(gH)


# ---- the batch the lane emulation and the GPU are both held to ------------------------------------------------------------------
BOUNDARY_COUNTS = (0, 1, 3, 4, 5, 14, 15, 16, 63, 64, 65, 255, 256, 257, LDS_MATCHES - 1, LDS_MATCHES, LDS_MATCHES + 1, 2 * LDS_MATCHES + 7)
GENERAL_COUNTS = (64, 257)            # pairs without a homography: status 3 after the floored stop rule
POSE_CAP, ERR_CAP = tv.POSE_CAP, tv.ERR_CAP
# 1000 x the largest differences measured between the kernel's source run lane by lane on the CPU and this reference on the
# boundary batch (tests/test_homography_lanes_cpu.py, where the measured values are written down): room for the device's sqrt /
# divide sequences
H_TOL = min(1000 * 3.5e-16, POSE_CAP)          # Frobenius norm of the difference of the unit-norm homographies
ROT_TOL = min(1000 * 2.3e-16, POSE_CAP)        # angle between the rotation-only models, radians
ERR_TOL = min(1000 * 5.7e-13, ERR_CAP)         # pixels, of the per-match transfer errors

BOUNDARY_SEED = 3      # one for which the reference ends at the generated inlier set on every planar and rotation pair of >= 15


def boundary_inputs():
    """The batch of boundary_batch() without its reference (tools/geometry_fingerprint.py)."""
    kinds = ["planar"] * len(BOUNDARY_COUNTS) + ["rotation"] * len(BOUNDARY_COUNTS) + ["general"] * len(GENERAL_COUNTS)
    counts = np.array(list(BOUNDARY_COUNTS) * 2 + list(GENERAL_COUNTS), np.int64)
    order = np.random.default_rng(11).permutation(len(counts))
    assert len(counts) == 38 and len(counts) % 4 != 0
    return make_pairs([kinds[i] for i in order], counts[order], (1, 2, 8), seed=BOUNDARY_SEED, p_outlier=0.3)


@functools.lru_cache(maxsize=None)
def boundary_batch():
    """(batch, reference): a planar and a rotation-only pair of every match count around the minimal sample, min_num_inliers, the
    wavefront, the workgroup and the LDS capacity S, and two general pairs, shuffled -- 38 pairs, not a multiple of 4 -- with
    30 % outliers, a pinhole, a radial and a fisheye camera."""
    batch = boundary_inputs()
    return batch, reference(batch)


def check_reference(batch, ref):
    """What the boundary batch promises of the reference alone: every status, the generated inlier set on every planar and
    rotation pair of >= 15 matches (no pair excused), the floored stop rule on the general pairs."""
    counts = np.diff(batch["pair_offsets"])
    kind = np.array(batch["kind"])
    assert {0, 1, 3}.issubset(set(ref["status"]))
    fits = kind != "general"
    assert (ref["status"][fits & (counts >= 15)] == 0).all() and (ref["status"][fits & (counts < 4)] == 1).all()
    assert (ref["status"][fits & (counts >= 4) & (counts < 15)] == 3).all() and (ref["status"][~fits] == 3).all()
    want = batch["true_inlier"] & np.repeat(fits & (counts >= 15), counts)
    assert np.array_equal(ref["inlier"].astype(bool), want)
    o = dict(DEFAULTS)
    for p in np.flatnonzero(~fits):                       # no model that could pass: the floor's count, not max_num_trials
        assert ref["n_trials"][p] == int(np.ceil(trials_needed(o, 10048, 0, counts[p]) / 64)) * 64 < 2000
    rot = fits & (counts >= 15) & (kind == "rotation")
    pla = fits & (counts >= 15) & (kind == "planar")
    assert np.array_equal(ref["n_rot_inliers"][rot], ref["n_inliers"][rot])
    assert (5 * ref["n_rot_inliers"][pla & (counts >= 63)] < ref["n_inliers"][pla & (counts >= 63)]).all()


def h_distance(H0, H1):
    """Frobenius norm of the difference of two unit-norm homographies (their signs are fixed by the inliers)."""
    return float(np.linalg.norm(np.asarray(H0) - np.asarray(H1)))


def compare(got, ref, report=None):
    """got / ref: dicts of host arrays (NAMES).  Everything discrete is equal, no pair excused; H within H_TOL, the rotation
    within ROT_TOL, errors within ERR_TOL, NaN patterns equal.  Returns (max H difference, max rotation angle, max err diff)."""
    for k in ("status", "n_inliers", "n_rot_inliers", "n_trials", "inlier"):
        assert np.array_equal(got[k], ref[k]), k
    ok = ref["status"] == 0
    assert np.isnan(got["H"][~ok]).all() and np.isnan(got["rot_qvec"][~ok]).all()
    assert np.array_equal(np.isnan(got["rot_qvec"]), np.isnan(ref["rot_qvec"]))
    dH = [h_distance(ref["H"][i], got["H"][i]) for i in np.flatnonzero(ok)]
    zero = np.array([1.0, 0.0, 0.0])              # (pose_distance divides by |t|)
    dR = [ac.pose_distance(ref["rot_qvec"][i], zero, got["rot_qvec"][i], zero)[0] for i in np.flatnonzero(ok & ~np.isnan(ref["rot_qvec"][:, 0]))]
    assert np.array_equal(np.isnan(got["err"]), np.isnan(ref["err"]))
    have = ~np.isnan(ref["err"])
    worst = (max(dH, default=0.0), max(dR, default=0.0), np.abs(got["err"][have] - ref["err"][have]).max() if have.any() else 0.0)
    print("%smax H difference %.3e, max rotation difference %.3e rad, max error difference %.3e px" % (report or "", *worst))
    assert np.abs(np.linalg.norm(got["H"][ok], axis=1) - 1.0).max() <= 1e-12
    q = got["rot_qvec"][ok]
    assert (q[:, 0] >= 0).all() and np.abs(np.linalg.norm(q, axis=1) - 1.0).max() <= 1e-12
    assert worst[0] <= H_TOL and worst[1] <= ROT_TOL and worst[2] <= ERR_TOL
    return worst


# ---- the pairs api.TwoViewClassifier is held to ----------------------------------------------------------------------------------------
CLASSIFIER_SEED = 1
CLASSIFIER_KINDS = ("rotation", "planar", "general") * 4
CLASS_OF_KIND = {"rotation": "PANORAMIC", "planar": "PLANAR", "general": "CALIBRATED"}


@functools.lru_cache(maxsize=None)
def classifier_batch():
    """(batch, homography reference, essential-matrix reference): twelve pairs of 200 matches with 30 % outliers through one
    SIMPLE_PINHOLE camera (f = 1200), four rotation-only, four planar, four general."""
    batch = make_pairs(CLASSIFIER_KINDS, [200] * 12, (0,), seed=CLASSIFIER_SEED, p_outlier=0.3)
    return batch, reference(batch), tv.reference(batch)
