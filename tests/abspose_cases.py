"""Helper of the absolute-pose tests (not collected): a numpy reference of the per-query estimator, written from its
specification (include/pixsfm_hip.h) and not from the kernel, and a generator of queries.

    samples   draw d of sample h = mix(mix(seed + G (h + 1)) + G (d + 1)) mod n (splitmix64's output function, 64-bit wrap-around),
              repeated indices drawn again, the three used in ascending order
    P3P       Grunert: s_2 = u s_1, s_3 = v s_1, u = N(v) / D(v), quartic N^2 - 2 cos(gamma) N D + D^2 M = 0 (in 1 / v where its
              constant coefficient outweighs the leading one); Ferrari's real roots in the order (+,+) (+,-) (-,+) (-,-), three
              guarded Newton steps each; u from the cosine law for a close pair of roots where N / D tends to 0 / 0; three Newton
              steps on the three cosine-law equations in the distances; poses with positive distances only
    score     err = |(u, v) - (X/Z, Y/Z)|^2, inlier iff Z > 0 and err <= (max_error / mean focal)^2;
              key (count, -sum min(err, thr^2), -h, -root)
    stop      after every round: samples done >= clamp(log(1 - confidence) / log(1 - w^3), min_num_trials, max_num_trials)
    LO        Levenberg-Marquardt on the pixel residuals of the inliers (Cauchy weights), classify by pixel error, repeat
"""
import functools

import numpy as np

import pxo
import triangulation_cases as tc
from pixsfm_amd import synthetic

DEFAULTS = dict(max_error=12.0, min_inlier_ratio=0.01, min_num_inliers=4, confidence=0.99999, min_num_trials=64, max_num_trials=4096,
                round_size=64, seed=0, refine_max_iterations=100, refine_loss_scale=1.0, lo_rounds=4)
LDS_CORR = 1024        # PXR_ABSPOSE_LDS_CORR: the staged-in-LDS capacity S of the kernel (include/pixsfm_hip.h)
IMAGE = (1000.0, 960.0)   # width, height around the principal point of tc.MODEL_PARAMS

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15


# ---- samples ---------------------------------------------------------------------------------------------------------------------
def mix(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample(seed, h, n, k=3, max_draws=256):
    """Sample h of an item with n > k usable records: k distinct indices, ascending (pxr_robust.h's sample_distinct<k>; three for
    a query's P3P, five for a pair's essential matrix).  The draw counter is shared by the k indices.  (The kernel's written-out k = 3 form takes
    one more draw for the third index where the second used up all max_draws: never in practice.)"""
    a = mix(seed + G * (h + 1))
    draw, idx = 0, []
    for _ in range(k):
        c, fresh = 0, False
        while not fresh and draw < max_draws:
            draw += 1
            c = mix(a + G * draw) % n
            fresh = c not in idx
        if not fresh:                 # (never in practice: the smallest unused index)
            c = min(x for x in range(k) if x not in idx)
        idx.append(c)
    return tuple(sorted(idx))


# ---- camera models, vectorised (checked against the oracle in tests/test_abspose_cpu.py) ---------------------------------------
def _focal_pp(model, k):
    return (k[0], k[0], k[1], k[2]) if model in tc.SINGLE_FOCAL else (k[0], k[1], k[2], k[3])


def world_to_image(model, k, u, v):
    """COLMAP 3.8 WorldToImage of models 0-4 and 8 on arrays (complex arguments allowed: the complex-step derivative below)."""
    fx, fy, cx, cy = _focal_pp(model, k)
    r2 = u * u + v * v
    if model in (0, 1):
        du = dv = 0.0
    elif model == 2:
        du, dv = u * (k[3] * r2), v * (k[3] * r2)
    elif model == 3:
        rad = k[3] * r2 + k[4] * r2 * r2
        du, dv = u * rad, v * rad
    elif model == 4:
        rad = k[4] * r2 + k[5] * r2 * r2
        du = u * rad + 2.0 * k[6] * u * v + k[7] * (r2 + 2.0 * u * u)
        dv = v * rad + 2.0 * k[7] * u * v + k[6] * (r2 + 2.0 * v * v)
    elif model == 8:
        r = np.sqrt(r2)
        with np.errstate(all="ignore"):
            theta = np.arctan(r)
            thd = theta * (1.0 + k[3] * theta * theta)
            s = np.where(np.abs(r) > 1e-8, thd / np.where(r == 0, 1.0, r), 1.0)
        du, dv = u * s - u, v * s - v
    else:
        raise NotImplementedError("model %d" % model)
    return fx * (u + du) + cx, fy * (v + dv) + cy


def camera_jacobian(model, k, u, v):
    """d(x, y) / d(u, v) by the complex step (exact to rounding): (n, 2, 2)."""
    h = 1e-30
    xu, yu = world_to_image(model, k, u + 1j * h, v + 0j)
    xv, yv = world_to_image(model, k, u + 0j, v + 1j * h)
    return np.stack([np.stack([xu.imag, xv.imag], -1), np.stack([yu.imag, yv.imag], -1)], -2) / h


def image_to_world(model, k, xy, max_iters=32):
    """ImageToWorld as pxr_image_to_world specifies it, on arrays: (uv (n, 2), ok (n,))."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    fx, fy, cx, cy = _focal_pp(model, k)
    with np.errstate(all="ignore"):
        u, v = (xy[:, 0] - cx) / fx, (xy[:, 1] - cy) / fy
        ok = np.isfinite(u) & np.isfinite(v)
        if model > 1:
            live, conv = ok.copy(), np.zeros(len(u), bool)
            for _ in range(max_iters):
                if not live.any():
                    break
                x, y = world_to_image(model, k, u, v)
                J = camera_jacobian(model, k, u, v)
                rx, ry = x - xy[:, 0], y - xy[:, 1]
                det = J[:, 0, 0] * J[:, 1, 1] - J[:, 0, 1] * J[:, 1, 0]
                live &= np.isfinite(det) & (np.abs(det) > 0)
                du, dv = (J[:, 1, 1] * rx - J[:, 0, 1] * ry) / det, (J[:, 0, 0] * ry - J[:, 1, 0] * rx) / det
                u, v = np.where(live, u - du, u), np.where(live, v - dv, v)
                step2 = du * du + dv * dv
                live &= np.isfinite(step2)
                conv |= live & (step2 < 1e-20)
                live &= ~conv
            ok = conv & np.isfinite(u) & np.isfinite(v)
    uv = np.stack([u, v], 1)
    uv[~ok] = np.nan
    return uv, ok


def mean_focal(model, k):
    return k[0] if model in tc.SINGLE_FOCAL else 0.5 * (k[0] + k[1])


# ---- P3P -------------------------------------------------------------------------------------------------------------------------
def _polish(v, B, C, D, E):
    """Three Newton steps on the monic quartic, each kept only where it does not raise |f| (at a double root f' vanishes with f and
    an unguarded step can land anywhere)."""
    f = (((v + B) * v + C) * v + D) * v + E
    for _ in range(3):
        d = ((4.0 * v + 3.0 * B) * v + 2.0 * C) * v + D
        if d == 0.0:
            break
        vn = v - f / d
        fn = (((vn + B) * vn + C) * vn + D) * vn + E
        if not abs(fn) <= abs(f):
            break
        v, f = vn, fn
    return v


LEAD_TOL = 1e-12       # the quartic's leading coefficient counts as zero below this fraction of the sum of the coefficients' magnitudes
PAIR_TOL = 1e-3        # two roots of the quartic are a close pair within this fraction of their size
SMALL_D = 1e-3         # of a close pair, u is taken from the cosine law and not from N(v) / D(v) where |D(v)| is below this fraction of its terms
DISC_TOL = 1e-7        # a quadratic factor's discriminant counts as zero down to minus this fraction of its terms
DISTANCE_NEWTON = 3    # Newton steps on the three cosine-law equations in the distances (ABS_DISTANCE_NEWTON)


def polish_distances(s, ha, hb, hg, a2, b2, c2):
    """DISTANCE_NEWTON Newton steps on the three cosine-law equations (s2 - s3)^2 + 2 s2 s3 (1 - cos alpha) = a^2, (s1 - s3)^2 +
    2 s1 s3 (1 - cos beta) = b^2, (s1 - s2)^2 + 2 s1 s2 (1 - cos gamma) = c^2 from s = (s1, s2, s3), with ha = 1 - cos alpha = |f2 -
    f3|^2 / 2 and so on (a narrow field of view has cosines that round away what separates them from 1): the 3 x 3 system of
    each step by Cramer's rule, a step skipped where the determinant vanishes or the step is not finite."""
    s1, s2, s3 = s
    for _ in range(DISTANCE_NEWTON):
        d23, d13, d12 = s2 - s3, s1 - s3, s1 - s2
        F1 = d23 * d23 + 2.0 * s2 * s3 * ha - a2
        F2 = d13 * d13 + 2.0 * s1 * s3 * hb - b2
        F3 = d12 * d12 + 2.0 * s1 * s2 * hg - c2
        j12, j13 = 2.0 * (d23 + s3 * ha), 2.0 * (s2 * ha - d23)
        j21, j23 = 2.0 * (d13 + s3 * hb), 2.0 * (s1 * hb - d13)
        j31, j32 = 2.0 * (d12 + s2 * hg), 2.0 * (s1 * hg - d12)
        det = j12 * j23 * j31 + j13 * j21 * j32
        d1 = (j12 * j23 * F3 + j13 * j32 * F2 - j23 * j32 * F1) / det
        d2 = (j23 * j31 * F1 + j13 * j21 * F3 - j13 * j31 * F2) / det
        d3 = (j12 * j31 * F2 + j21 * j32 * F1 - j12 * j21 * F3) / det
        if det != 0.0 and np.isfinite(d1) and np.isfinite(d2) and np.isfinite(d3):
            s1, s2, s3 = s1 - d1, s2 - d2, s3 - d3
    return s1, s2, s3


def p3p(uv, X, details=None):
    """The poses [(root, R, t)] of three correspondences (uv (3, 2) normalised image points, X (3, 3)).  details: a dict that
    receives the quartic's ascending coefficients A."""
    with np.errstate(all="ignore"):
        f = np.concatenate([uv, np.ones((3, 1))], 1)
        f = f / np.sqrt(uv[:, :1] ** 2 + uv[:, 1:] ** 2 + 1.0)
        e1, e2, e3 = X[1] - X[0], X[2] - X[0], X[2] - X[1]
        c2, b2, a2 = e1 @ e1, e2 @ e2, e3 @ e3
        cr = np.cross(e1, e2)
        cr2 = cr @ cr
        if not (cr2 > 1e-12 * c2 * b2) or not np.isfinite(cr2):
            return []
        w1, w3 = e1 / np.sqrt(c2), cr / np.sqrt(cr2)
        w2 = np.cross(w3, w1)
        ca, cb, cg = f[1] @ f[2], f[0] @ f[2], f[0] @ f[1]
        da, db, dg = f[1] - f[2], f[0] - f[2], f[0] - f[1]
        ha, hb, hg = 0.5 * (da @ da), 0.5 * (db @ db), 0.5 * (dg @ dg)
        k1, k2 = (a2 - c2) / b2, c2 / b2
        N = np.array([k1 + 1.0, -2.0 * k1 * cb, k1 - 1.0])
        D = np.array([2.0 * cg, -2.0 * ca])
        M = np.array([1.0 - k2, 2.0 * k2 * cb, -k2])
        A = np.convolve(N, N) - 2.0 * cg * np.append(np.convolve(N, D), 0.0) + np.convolve(np.convolve(D, D), M)
        scale = np.abs(A).sum()
        if details is not None:
            details["A"] = A
        rev = abs(A[0]) > abs(A[4])               # the quartic of w = 1 / v has the larger leading coefficient
        if rev:
            A = A[::-1]
        if not (abs(A[4]) > LEAD_TOL * scale) or not np.isfinite(scale):
            return []
        B, C, Dq, E = A[3] / A[4], A[2] / A[4], A[1] / A[4], A[0] / A[4]
        p = C - 0.375 * B * B
        q = Dq - 0.5 * B * C + 0.125 * B ** 3
        r = E - 0.25 * B * Dq + 0.0625 * B * B * C - (3.0 / 256.0) * B ** 4
        c1, c0 = 0.25 * p * p - r, -0.125 * q * q
        Q, R = (p * p - 3.0 * c1) / 9.0, (2.0 * p ** 3 - 9.0 * p * c1 + 27.0 * c0) / 54.0
        if R * R < Q ** 3:
            m = -2.0 * np.sqrt(Q) * np.cos((np.arccos(R / np.sqrt(Q ** 3)) + 2.0 * np.pi) / 3.0) - p / 3.0
        else:
            Aa = -np.copysign(np.cbrt(abs(R) + np.sqrt(R * R - Q ** 3)), R)
            m = Aa + (Q / Aa if Aa != 0.0 else 0.0) - p / 3.0
        for _ in range(2):
            fm, dm = ((m + p) * m + c1) * m + c0, (3.0 * m + 2.0 * p) * m + c1
            if dm != 0.0:
                m -= fm / dm
        if not (m > 0.0) or not np.isfinite(m):
            return []
        sq = np.sqrt(2.0 * m)
        tq = q / (2.0 * sq)
        if not np.isfinite(tq):
            return []
        d1, d2, off = -2.0 * m - 2.0 * p - 4.0 * tq, -2.0 * m - 2.0 * p + 4.0 * tq, 0.25 * B
        roots = [np.nan] * 4
        low = -DISC_TOL * (2.0 * m + 2.0 * abs(p) + 4.0 * abs(tq))         # a double root's discriminant may round below zero
        if d1 >= low:
            sd = np.sqrt(max(d1, 0.0))
            roots[0], roots[1] = 0.5 * (sq + sd) - off, 0.5 * (sq - sd) - off
        if d2 >= low:
            sd = np.sqrt(max(d2, 0.0))
            roots[2], roots[3] = 0.5 * (-sq + sd) - off, 0.5 * (-sq - sd) - off
        roots = [_polish(v, B, C, Dq, E) if np.isfinite(v) else np.nan for v in roots]
        out = []
        for root, v in enumerate(roots):
            if not (v > 0.0) or not np.isfinite(v):
                continue
            twin = -1                             # the first other root within PAIR_TOL of this one
            for j in range(3, -1, -1):
                if j != root and abs(roots[j] - v) <= PAIR_TOL * v:
                    twin = j
            if rev:
                v = 1.0 / v
            g = 1.0 + v * (v - 2.0 * cb)
            den = D[0] + D[1] * v
            if twin < 0 or abs(den) > SMALL_D * (abs(D[0]) + abs(D[1] * v)):
                u = (N[0] + (N[1] + N[2] * v) * v) / den
            else:     # a close pair where N / D tends to 0 / 0: both roots of the cosine law in u are solutions, one for each of the pair
                h = np.sqrt(max(cg * cg - 1.0 + k2 * g, 0.0))
                u = cg + h if root < twin else cg - h
            if not (u > 0.0) or not np.isfinite(u) or not (g > 0.0):
                continue
            s1 = np.sqrt(b2 / g)
            s1, s2, s3 = polish_distances((s1, u * s1, v * s1), ha, hb, hg, a2, b2, c2)
            if not (s1 > 0.0 and s2 > 0.0 and s3 > 0.0):
                continue
            Q1, Q2, Q3 = s1 * f[0], s2 * f[1], s3 * f[2]
            g1, g2 = Q2 - Q1, Q3 - Q1
            crc = np.cross(g1, g2)
            n1, n3 = np.sqrt(g1 @ g1), np.sqrt(crc @ crc)
            if not (n1 > 0.0) or not (n3 > 0.0):
                continue
            cc1, cc3 = g1 / n1, crc / n3
            cc2 = np.cross(cc3, cc1)
            Rm = np.outer(cc1, w1) + np.outer(cc2, w2) + np.outer(cc3, w3)
            t = Q1 - Rm @ X[0]
            if np.isfinite(t).all():
                out.append((root, Rm, t))
        return out


# ---- refinement --------------------------------------------------------------------------------------------------------------------
def quat_mul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def pose_plus(q, t, d):
    """QuaternionManifold::Plus of Ceres on q (delta is a half angle, applied on the left), t + d; q re-normalised."""
    nd = np.linalg.norm(d[:3])
    q1 = q.copy()
    if nd != 0.0:
        q1 = quat_mul(np.concatenate([[np.cos(nd)], np.sin(nd) / nd * d[:3]]), q)
    return q1 / np.linalg.norm(q1), t + d[3:]


def pixel_errors(model, k, q, t, xy, X):
    """Pixel error of every correspondence under (q, t); NaN behind the camera."""
    p = X @ synthetic.qvec_to_rotmat(q).T + t
    with np.errstate(all="ignore"):
        x, y = world_to_image(model, k, p[:, 0] / p[:, 2], p[:, 1] / p[:, 2])
        e = np.sqrt((x - xy[:, 0]) ** 2 + (y - xy[:, 1]) ** 2)
    e[~(p[:, 2] > 0)] = np.nan
    return e


def normal_equations(model, k, q, t, xy, X, scale):
    R = synthetic.qvec_to_rotmat(q)
    pr = X @ R.T
    p = pr + t
    if not (p[:, 2] > 0).all():
        return None, None, np.inf
    iz = 1.0 / p[:, 2]
    u, v = p[:, 0] * iz, p[:, 1] * iz
    x, y = world_to_image(model, k, u, v)
    Juv = camera_jacobian(model, k, u, v)
    res = np.stack([x - xy[:, 0], y - xy[:, 1]], 1)
    s = (res * res).sum(1)
    b = scale * scale
    rho0, rho1 = b * np.log1p(s / b), 1.0 / (1.0 + s / b)
    A = np.stack([Juv[:, :, 0] * iz[:, None], Juv[:, :, 1] * iz[:, None],
                  -(Juv[:, :, 0] * p[:, None, 0] + Juv[:, :, 1] * p[:, None, 1]) * (iz * iz)[:, None]], 2)        # (n, 2, 3)
    Jr = 2.0 * np.cross(pr[:, None, :], A)                                 # p(d) = R(2 d) pr + t: A . (2 e_c x pr) = 2 (pr x A)_c
    J = np.concatenate([Jr, A], 2)
    H = np.einsum("n,nij,nik->jk", rho1, J, J)
    g = np.einsum("n,nij,ni->j", rho1, J, res)
    return H, g, float(rho0.sum())


def refine(model, k, q, t, xy, X, o):
    """Levenberg-Marquardt on the correspondences given (the inliers)."""
    H, g, cost = normal_equations(model, k, q, t, xy, X, o["refine_loss_scale"])
    if not np.isfinite(cost):
        return q, t
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
        q1, t1 = pose_plus(q, t, d)
        H1, g1, cost1 = normal_equations(model, k, q1, t1, xy, X, o["refine_loss_scale"])
        if cost1 <= cost + 1e-12 * cost:
            q, t, H, g, cost = q1, t1, H1, g1, cost1
            lam = max(lam * 0.1, 1e-12)
        else:
            lam *= 10.0
            if lam > 1e12:
                break
        if np.linalg.norm(d) <= 1e-12:
            break
    return q, t


# ---- the estimator -----------------------------------------------------------------------------------------------------------------
def trials_needed(o, max_trials, cnt, n, k=3):
    """Trials the stop rule asks for at cnt inliers among n, for samples of k (3 or 5; each kernel's own association of w^k)."""
    assert k in (3, 5)
    need = float(max_trials)
    if cnt > 0:
        w = cnt / n
        p_all_inliers = w * w * w if k == 3 else (w * w) * (w * w) * w
        with np.errstate(all="ignore"):
            x = np.log(1.0 - o["confidence"]) / np.log(1.0 - p_all_inliers)
        if x < need:
            need = x
    return min(max(need, float(o["min_num_trials"])), float(max_trials))


def estimate(xy, xyz, model, params, **options):
    """The estimator on one query.  Returns dict(status, qvec, tvec, n_inliers, n_trials, inlier (n,), err (n,), usable (n,))."""
    o = {**DEFAULTS, **options}
    xy, xyz = np.asarray(xy, dtype=np.float64).reshape(-1, 2), np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    k = np.asarray(params, dtype=np.float64)
    N = len(xy)
    uv_all, ok = image_to_world(model, k, xy)
    usable = ok & np.isfinite(xy).all(1) & np.isfinite(xyz).all(1)
    out = dict(status=1, qvec=None, tvec=None, n_inliers=0, n_trials=0, inlier=np.zeros(N, np.uint8), err=np.full(N, np.nan), usable=usable)
    idx = np.flatnonzero(usable)
    n = len(idx)
    if n < 4:
        return out
    uv, X, px = uv_all[idx], xyz[idx], xy[idx]
    thr = o["max_error"] / mean_focal(model, k)
    thr2 = thr * thr
    max_trials = -(-o["max_num_trials"] // o["round_size"]) * o["round_size"]

    def score(R, t):
        pz = R[2, 0] * X[:, 0] + R[2, 1] * X[:, 1] + R[2, 2] * X[:, 2] + t[2]
        with np.errstate(all="ignore"):
            iz = 1.0 / pz
            du = uv[:, 0] - (R[0, 0] * X[:, 0] + R[0, 1] * X[:, 1] + R[0, 2] * X[:, 2] + t[0]) * iz
            dv = uv[:, 1] - (R[1, 0] * X[:, 0] + R[1, 1] * X[:, 1] + R[1, 2] * X[:, 2] + t[1]) * iz
            e2 = du * du + dv * dv
            inl = (pz > 0.0) & (e2 <= thr2)
        return inl, np.where(inl, e2, thr2)

    best, done = None, 0
    while True:
        for h in range(done, done + o["round_size"]):
            s = sample(o["seed"], h, n)
            for root, R, t in p3p(uv[list(s)], X[list(s)]):
                inl, e = score(R, t)
                key = (int(inl.sum()), -float(np.cumsum(e)[-1]), -h, -root)        # (cumsum: the sum in index order)
                if best is None or key > best[0]:
                    best = (key, R, t, inl)
        done += o["round_size"]
        if done >= max_trials or done >= trials_needed(o, max_trials, best[0][0] if best else -1, n):
            break
    out["n_trials"] = done
    if best is None:
        out["status"] = 2
        return out
    _, R, t, cur = best
    q = synthetic.rotmat_to_qvec(R)
    q = q / np.linalg.norm(q)
    cur_cnt = int(cur.sum())
    for _ in range(o["lo_rounds"]):
        q1, t1 = refine(model, k, q.copy(), t.copy(), px[cur], X[cur], o)
        with np.errstate(invalid="ignore"):
            new = pixel_errors(model, k, q1, t1, px, X) <= o["max_error"]
        if new.sum() < cur_cnt:
            break
        changed = bool((new != cur).any())
        q, t, cur, cur_cnt = q1, t1, new, int(new.sum())
        if not changed:
            break
    err = pixel_errors(model, k, q, t, px, X)
    with np.errstate(invalid="ignore"):
        fin = err <= o["max_error"]
    out["status"] = 3
    if fin.sum() < max(o["min_num_inliers"], int(np.ceil(o["min_inlier_ratio"] * n))):
        return out
    if q[0] < 0:
        q = -q
    out.update(status=0, qvec=q, tvec=t, n_inliers=int(fin.sum()))
    out["inlier"][idx] = fin
    out["err"][idx] = err
    return out


def reference(batch, **options):
    """The estimator on every query of a batch (the dict engine.AbsolutePoseProblem takes).  Arrays like the kernel's outputs;
    qvec / tvec are NaN where status is not 0."""
    off = np.asarray(batch["query_offsets"])
    T = len(off) - 1
    res = dict(qvec=np.full((T, 4), np.nan), tvec=np.full((T, 3), np.nan), status=np.zeros(T, np.int32), n_inliers=np.zeros(T, np.int32),
               n_trials=np.zeros(T, np.int32), inlier=np.zeros(off[-1], np.uint8), err=np.full(off[-1], np.nan))
    for qi in range(T):
        cam = batch["query_camera"][qi]
        m = int(batch["cam_model"][cam])
        r = estimate(batch["xy"][off[qi]:off[qi + 1]], batch["xyz"][off[qi]:off[qi + 1]], m,
                     batch["cam_params"][cam][:pxo.lib().pxo_camera_num_params(m)], **options)
        res["status"][qi], res["n_inliers"][qi], res["n_trials"][qi] = r["status"], r["n_inliers"], r["n_trials"]
        if r["status"] == 0:
            res["qvec"][qi], res["tvec"][qi] = r["qvec"], r["tvec"]
        res["inlier"][off[qi]:off[qi + 1]] = r["inlier"]
        res["err"][off[qi]:off[qi + 1]] = r["err"]
    return res


def pose_distance(q0, t0, q1, t1):
    """(rotation angle in radians, |dt| / |t|) between two poses."""
    q0, q1 = np.asarray(q0) / np.linalg.norm(q0), np.asarray(q1) / np.linalg.norm(q1)
    r = quat_mul(q0 * [1.0, -1.0, -1.0, -1.0], q1)                 # the relative rotation; atan2 of its two parts resolves small angles
    ang = 2.0 * np.arctan2(np.linalg.norm(r[1:]), abs(r[0]))
    return ang, float(np.linalg.norm(np.asarray(t0) - t1) / np.linalg.norm(t0))


# ---- queries -----------------------------------------------------------------------------------------------------------------------
def random_pose(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    if q[0] < 0:
        q = -q
    return q, rng.uniform(-3, 3, 3)


def make_queries(counts, models, seed, sigma=0.5, p_outlier=0.3, min_outlier_shift=40.0):
    """A batch of queries: query i has counts[i] correspondences and camera i % len(models) (tc.MODEL_PARAMS).  The 3D points
    sit at depths 2-20 in front of a random pose, spread over the image; an inlier is the true projection plus Gaussian noise
    of sigma clipped at 3 sigma; floor(p_outlier n) correspondences (p_outlier: a number or one per query; none in queries
    of fewer than 8, and never so many that fewer than 6 inliers remain: a false pose needs its three sample points and chance
    hits, and three chance hits within 12 px have probability ~1e-10) are outliers, uniform in the image but at least min_outlier_shift px (None: no
    condition) from its true projection.  Returns the batch dict + gt_qvec, gt_tvec, true_inlier."""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, dtype=np.int64)
    p_out = np.broadcast_to(np.asarray(p_outlier, dtype=np.float64), counts.shape)
    cam_model = np.array(models, np.int32)
    cam_params = tc.pad_params([tc.MODEL_PARAMS[m] for m in models])
    xy, xyz, inl, gq, gt = [], [], [], [], []
    W, H = IMAGE
    for i, n in enumerate(counts):
        m = int(cam_model[i % len(models)])
        k = np.array(tc.MODEL_PARAMS[m], dtype=np.float64)
        q, t = random_pose(rng)
        R = synthetic.qvec_to_rotmat(q)
        pix = np.stack([rng.uniform(0.05 * W, 0.95 * W, n), rng.uniform(0.05 * H, 0.95 * H, n)], 1)
        uv, ok = image_to_world(m, k, pix)
        assert ok.all()
        depth = rng.uniform(2.0, 20.0, n)
        X = (np.concatenate([uv, np.ones((n, 1))], 1) * depth[:, None] - t) @ R            # R^t (p - t)
        noise = np.clip(rng.normal(0, sigma, (n, 2)), -3 * sigma, 3 * sigma) if sigma > 0 else np.zeros((n, 2))
        obs = pix + noise
        bad = np.zeros(n, bool)
        if n >= 8:
            bad[rng.permutation(n)[:min(int(p_out[i] * n), n - 6)]] = True
        for j in np.flatnonzero(bad):
            while True:
                c = np.array([rng.uniform(0, W), rng.uniform(0, H)])
                if min_outlier_shift is None or np.linalg.norm(c - pix[j]) >= min_outlier_shift:
                    break
            obs[j] = c
        xy.append(obs); xyz.append(X); inl.append(~bad); gq.append(q); gt.append(t)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    cat = lambda parts, w: np.concatenate(parts).reshape(-1, w) if len(parts) else np.zeros((0, w))
    return dict(query_offsets=off, xy=cat(xy, 2), xyz=cat(xyz, 3), query_camera=(np.arange(len(counts)) % len(models)).astype(np.int32),
                cam_model=cam_model, cam_params=cam_params, gt_qvec=np.array(gq).reshape(-1, 4), gt_tvec=np.array(gt).reshape(-1, 3),
                true_inlier=np.concatenate(inl) if len(inl) else np.zeros(0, bool))


def single(batch, qi):
    """Query qi of a batch as a batch of its own."""
    off = batch["query_offsets"]
    s = slice(off[qi], off[qi + 1])
    return dict(batch, query_offsets=np.array([0, off[qi + 1] - off[qi]], np.int64), xy=batch["xy"][s], xyz=batch["xyz"][s],
                query_camera=batch["query_camera"][qi:qi + 1])


def collinear_query(n=12, seed=3):
    """A query whose 3D points lie on one line: every sample is degenerate (status 2)."""
    rng = np.random.default_rng(seed)
    X = np.array([0.3, -0.2, 6.0]) + np.outer(rng.uniform(-2, 2, n), [1.0, 0.5, 0.2])
    k = np.array(tc.MODEL_PARAMS[1])
    xy = np.stack([k[0] * X[:, 0] / X[:, 2] + k[2], k[1] * X[:, 1] / X[:, 2] + k[3]], 1)
    return xy, X


def eleven_models_queries():
    """(batch, gt_qvec, gt_tvec): one noise-free query of 40 correspondences per camera model."""
    models = sorted(tc.MODEL_PARAMS)
    rng = np.random.default_rng(31)
    xy, xyz, gq, gt = [], [], [], []
    for m in models:
        q, t = random_pose(rng)
        p = np.concatenate([rng.uniform(-0.3, 0.3, (40, 2)), np.ones((40, 1))], 1) * rng.uniform(2, 20, (40, 1))
        X = (p - t) @ synthetic.qvec_to_rotmat(q)
        k = np.array(tc.MODEL_PARAMS[m], dtype=np.float64)
        xy.append(np.array([pxo.world_to_pixel(m, k, q, t, x, jac=False)[0] for x in X]))
        xyz.append(X); gq.append(q); gt.append(t)
    batch = dict(query_offsets=np.arange(len(models) + 1, dtype=np.int64) * 40, xy=np.concatenate(xy), xyz=np.concatenate(xyz),
                 query_camera=np.arange(len(models), dtype=np.int32), cam_model=np.array(models, np.int32),
                 cam_params=tc.pad_params([tc.MODEL_PARAMS[m] for m in models]))
    return batch, gq, gt


# ---- hard families of minimal samples (tests/test_minimal_solvers_*.py) ---------------------------------------------------------
def _from_camera_points(rng, P):
    """A noise-free sample whose points sit at P (3, 3) in the camera's frame, under a random pose: (uv, X, R, t)."""
    q, t = random_pose(rng)
    R = synthetic.qvec_to_rotmat(q)
    return P[:, :2] / P[:, 2:], (P - t) @ R, R, t


def _points(rng, half_field=0.4, depth=(2.0, 20.0)):
    return np.concatenate([rng.uniform(-half_field, half_field, (3, 2)), np.ones((3, 1))], 1) * rng.uniform(*depth, (3, 1))


def _nearly_collinear(rng, off):
    uv = rng.uniform(-0.4, 0.4, (3, 2))
    d = uv[1] - uv[0]
    uv[2] = uv[0] + rng.uniform(0.2, 0.8) * d + off * np.array([-d[1], d[0]]) / np.linalg.norm(d)
    return np.concatenate([uv, np.ones((3, 1))], 1) * rng.uniform(2.0, 20.0, (3, 1))


def _equilateral(rng, jitter):
    """A triangle with equal sides in a plane facing the camera, its centre on the optical axis; every coordinate moved by up to jitter."""
    r, d, th = rng.uniform(0.5, 2.0), rng.uniform(4.0, 10.0), rng.uniform(0, 2 * np.pi) + 2 * np.pi / 3 * np.arange(3)
    return np.stack([r * np.cos(th), r * np.sin(th), np.full(3, d)], 1) + jitter * rng.uniform(-1, 1, (3, 3))


def _two_equal_distances(rng):
    f = np.concatenate([rng.uniform(-0.4, 0.4, (3, 2)), np.ones((3, 1))], 1)
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    s = rng.uniform(2.0, 20.0)
    return f * np.array([s, s, rng.uniform(2.0, 20.0)])[:, None]


def _leading_ratio(P):
    det = {}
    p3p(P[:, :2] / P[:, 2:], P, det)
    return det["A"][4] / np.abs(det["A"]).sum()


def _small_leading_coefficient(rng, target):
    """Points whose quartic has A4 = target x (sum of |A_k|), to a few per cent: A4 is 4 c^2 / b^2 (cos^2 of the triangle's angle at
    point 1 - cos^2 alpha), so the first point slides along its ray until that angle meets the angle of view of the other two."""
    while True:
        P = _points(rng)
        ray, grid = P[0] / P[0, 2], np.linspace(1.0, 40.0, 100)
        val = np.array([_leading_ratio(np.vstack([ray * z, P[1:]])) for z in grid]) - target
        k = np.flatnonzero(np.sign(val[:-1]) * np.sign(val[1:]) < 0)
        if not len(k):
            continue
        lo, hi = grid[k[0]], grid[k[0] + 1]
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            same = np.sign(_leading_ratio(np.vstack([ray * mid, P[1:]])) - target) == np.sign(val[k[0]])
            lo, hi = (mid, hi) if same else (lo, mid)
        P = np.vstack([ray * lo, P[1:]])
        if abs(_leading_ratio(P) / target - 1.0) < 0.1:
            return P


HARD_FAMILIES = {
    "generic": _points,
    "distant": lambda rng: _points(rng, depth=(1000.0, 1001.0)),
    "narrow field": lambda rng: _points(rng, half_field=0.005),
    "nearly collinear 1e-3": lambda rng: _nearly_collinear(rng, 1e-3),
    "nearly collinear 1e-5": lambda rng: _nearly_collinear(rng, 1e-5),
    "nearly collinear 1e-7": lambda rng: _nearly_collinear(rng, 1e-7),
    "equilateral": lambda rng: _equilateral(rng, 0.0),
    "equilateral 1e-3": lambda rng: _equilateral(rng, 1e-3),
    "equilateral 1e-6": lambda rng: _equilateral(rng, 1e-6),
    "equilateral 1e-9": lambda rng: _equilateral(rng, 1e-9),
    "two equal distances": _two_equal_distances,
    "A4 above LEAD_TOL": lambda rng: _small_leading_coefficient(rng, rng.choice([-1.0, 1.0]) * rng.uniform(1.5, 10.0) * LEAD_TOL),
    "A4 below LEAD_TOL": lambda rng: _small_leading_coefficient(rng, rng.choice([-1.0, 1.0]) * rng.uniform(0.1, 0.7) * LEAD_TOL),
}
# (both A4 families are solved: where |A0| > |A4| the quartic of 1 / v is the one that LEAD_TOL applies to)


def hard_family(name, seed, B=64):
    """B noise-free samples of a family of HARD_FAMILIES: (uv (B, 3, 2), X (B, 3, 3), R (B, 3, 3), t (B, 3))."""
    rng = np.random.default_rng(seed)
    parts = [_from_camera_points(rng, HARD_FAMILIES[name](rng)) for _ in range(B)]
    return tuple(np.array([p[k] for p in parts]) for k in range(4))


def degenerate_samples(seed=0):
    """(uv (3, 3, 2), X (3, 3, 3)): two coincident correspondences, three world points on one line, a coordinate that is not a number."""
    uv, X, _, _ = hard_family("generic", seed, 3)
    uv[0, 1], X[0, 1] = uv[0, 0], X[0, 0]
    X[1, 2] = X[1, 0] + 0.75 * (X[1, 1] - X[1, 0])
    X[2, 0, 1] = np.nan
    return uv, X


# ---- the batch the lane emulation and the GPU are both held to ------------------------------------------------------------------
BOUNDARY_COUNTS = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, LDS_CORR - 1, LDS_CORR, LDS_CORR + 1, 2 * LDS_CORR + 7)
POSE_TOL = 1e-7        # rotation angle (rad) and |dt| / |t| between two implementations: both stop at a step <= 1e-12 on the same
                       # inlier set, so they sit within ~1e-10 of the same minimum; three orders are left for conditioning
ERR_TOL = 1e-6         # pixels, of the per-correspondence errors


def boundary_inputs():
    """The batch of boundary_batch() without its reference (tools/geometry_fingerprint.py)."""
    counts = np.repeat(BOUNDARY_COUNTS, 5)
    np.random.default_rng(11).shuffle(counts)
    assert len(counts) == 75 and len(counts) % 4 != 0
    return make_queries(counts, (1, 2, 8), seed=12, p_outlier=0.3)


@functools.lru_cache(maxsize=None)
def boundary_batch():
    """(batch, reference): correspondence counts around the wavefront, the workgroup and the LDS capacity S, five queries each,
    shuffled -- 75 queries, not a multiple of 4 -- with 30 % outliers, a pinhole, a radial and a fisheye camera."""
    batch = boundary_inputs()
    return batch, reference(batch)


def compare(got, ref, report=None):
    """got / ref: dicts of host arrays (qvec, tvec, status, n_inliers, n_trials, inlier, err).  Everything discrete is equal, no
    query excused; poses within POSE_TOL, errors within ERR_TOL, NaN patterns equal.  Returns (max angle, max |dt|/|t|, max err diff)."""
    assert np.array_equal(got["status"], ref["status"])
    assert np.array_equal(got["n_inliers"], ref["n_inliers"])
    assert np.array_equal(got["n_trials"], ref["n_trials"])
    assert np.array_equal(got["inlier"], ref["inlier"])
    ok = ref["status"] == 0
    assert np.isnan(got["qvec"][~ok]).all() and np.isnan(got["tvec"][~ok]).all()
    d = np.array([pose_distance(ref["qvec"][i], ref["tvec"][i], got["qvec"][i], got["tvec"][i]) for i in np.flatnonzero(ok)]).reshape(-1, 2)
    assert np.array_equal(np.isnan(got["err"]), np.isnan(ref["err"]))
    have = ~np.isnan(ref["err"])
    worst = (d[:, 0].max() if len(d) else 0.0, d[:, 1].max() if len(d) else 0.0,
             np.abs(got["err"][have] - ref["err"][have]).max() if have.any() else 0.0)
    print("%smax rotation difference %.3e rad, max |dt|/|t| %.3e, max pixel-error difference %.3e px" % (report or "", *worst))
    assert (got["qvec"][ok][:, 0] >= 0).all() and np.abs(np.linalg.norm(got["qvec"][ok], axis=1) - 1.0).max() <= 1e-12
    assert worst[0] <= POSE_TOL and worst[1] <= POSE_TOL and worst[2] <= ERR_TOL
    return worst
