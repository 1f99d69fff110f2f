"""Helper of the fundamental-matrix tests (not collected): a numpy reference of the per-pair estimator, written from its
specification (include/pixsfm_hip.h) and not from the kernel, and generators of image pairs whose stated
focal lengths are off.

    samples   twoview_cases.sample with k = 7: the hash of section 19, seven distinct indices in ascending order
    solver    the 7 x 9 system, two null vectors by Gauss-Jordan with full pivoting, orthonormalised, mixed into A and B; the cubic
              det(x A + B) by expansion along row 0; Sturm chain + bisection + Newton with + - x / only; F = x A + B, unit norm
    score     squared Sampson error in the normalised planes, inlier iff err <= thr^2; key (count, -sum min(err, thr^2), -h, -root)
    stop      after every round: samples done >= clamp(log(1 - confidence) / log(1 - w^7), min_num_trials, max_num_trials)
    LO        Levenberg-Marquardt on the inliers' signed Sampson residuals over two columns of F (one entry fixed) and the two
              coefficients of the third, re-normalise, classify, repeat

The solver runs on all samples of a round at once (arrays with a leading sample axis): every element sees the operations the
specification states, in its order, so a sample's numbers do not depend on the round it is in.
"""
import functools

import numpy as np

import abspose_cases as ac
import homography_cases as hc
import triangulation_cases as tc
import twoview_cases as tv
from pixsfm_amd import synthetic

DEFAULTS = dict(tv.DEFAULTS)
LDS_MATCHES = tv.LDS_MATCHES
IMAGE = tv.IMAGE
PIVOT_TOL, LEAD_TOL, TRIM_TOL = 1e-12, 1e-9, 1e-12
BISECT, NEWTON = 64, 4
RSQRT2 = 0.70710678118654752440

sample = functools.partial(tv.sample, k=7)
sampson = tv.sampson


def need_inliers(o, n):
    return max(o["min_num_inliers"], int(np.ceil(o["min_inlier_ratio"] * n)))


def trials_needed(o, max_trials, cnt, n):
    """tv.trials_needed's clamp for samples of seven: w = cnt / n, all-inlier probability (w2 w2) (w2 w) with w2 = w w."""
    need = float(max_trials)
    if cnt > 0:
        w = cnt / n
        w2 = w * w
        with np.errstate(all="ignore"):
            x = np.log(1.0 - o["confidence"]) / np.log(1.0 - (w2 * w2) * (w2 * w))
        if x < need:
            need = x
    return min(max(need, float(o["min_num_trials"])), float(max_trials))


# ---- the seven-point solver -------------------------------------------------------------------------------------------------------
def null_space(A):
    """The null space of A (B, 7, 9): Gauss-Jordan with full pivoting -> [I | C] in permuted columns, vector k = (-C[:, k], e_k),
    orthonormalised by modified Gram-Schmidt in the order k = 0, 1.  Returns (ok (B,), u (B, 2, 9))."""
    A = A.copy()
    B = len(A)
    ar = np.arange(B)
    S = np.abs(A).reshape(B, -1).max(1)
    ok = np.isfinite(S)
    perm = np.tile(np.arange(9), (B, 1))
    for c in range(7):
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
    u = np.zeros((B, 2, 9))
    for k in range(2):
        v = np.zeros((B, 9))
        for r in range(7):
            v[ar, perm[:, r]] = -A[:, r, 7 + k]
        v[ar, perm[:, 7 + k]] = 1.0
        for j in range(k):
            d = np.zeros(B)
            for m in range(9):
                d = d + v[:, m] * u[:, j, m]
            v = v - d[:, None] * u[:, j]
        d = np.zeros(B)
        for m in range(9):
            d = d + v[:, m] * v[:, m]
        nrm = np.sqrt(d)
        ok &= (nrm > 0.0) & np.isfinite(nrm)
        u[:, k] = v / nrm[:, None]
    return ok, u


def cubic(A, B):
    """det(x A + B) for A, B (.., 9): the four ascending coefficients (.., 4), by expansion along row 0 as the header states."""
    c = [np.zeros(A.shape[:-1]) for _ in range(4)]
    for a in range(3):
        b, cc = (a + 1) % 3, (a + 2) % 3
        a1b, a1c, a2b, a2c = A[..., 3 + b], A[..., 3 + cc], A[..., 6 + b], A[..., 6 + cc]
        b1b, b1c, b2b, b2c = B[..., 3 + b], B[..., 3 + cc], B[..., 6 + b], B[..., 6 + cc]
        q2 = a1b * a2c - a1c * a2b
        q1 = (a1b * b2c + b1b * a2c) - (a1c * b2b + b1c * a2b)
        q0 = b1b * b2c - b1c * b2b
        a0, b0 = A[..., a], B[..., a]
        c[3] = c[3] + a0 * q2
        c[2] = c[2] + (a0 * q1 + b0 * q2)
        c[1] = c[1] + (a0 * q0 + b0 * q1)
        c[0] = c[0] + b0 * q0
    return np.stack(c, -1)


def sturm_chain(c):
    """The Sturm chain of one cubic c (4 ascending coefficients, plain floats): p, p', then minus the remainder of the two before,
    each scaled to a largest coefficient of 1.  Returns (chain (4, 4) zero-padded, ok)."""
    chain = np.zeros((4, 4))
    polys = [list(c), [(k + 1) * c[k + 1] for k in range(3)]]
    while len(polys) <= 3 and len(polys[-1]) > 1:
        a, b = polys[-2], polys[-1]
        db = len(b) - 1
        r = list(a)
        for k in range(len(a) - 1, db - 1, -1):
            q = r[k] / b[db]
            for j in range(db):
                r[k - db + j] = r[k - db + j] - q * b[j]
            r[k] = 0.0
        r = r[:db]
        m = max(abs(v) for v in r)
        if not np.isfinite(m):
            return chain, False
        if not m > 0.0:
            break
        r = [-(v / m) for v in r]
        while len(r) > 1 and not abs(r[-1]) > TRIM_TOL:
            r.pop()
        polys.append(r)
    for i, p in enumerate(polys):
        chain[i, :len(p)] = p
    return chain, True


def sign_changes(chain, x):
    """chain (B, 4, 4), x (B, K): sign changes of every chain at every x (zeros skipped)."""
    changes = np.zeros(x.shape, np.int64)
    prev = np.zeros(x.shape, np.int64)
    for i in range(4):
        v = np.broadcast_to(chain[:, i, 3, None], x.shape).copy()
        for k in range(2, -1, -1):
            v = v * x + chain[:, i, k, None]
        sg = (v > 0.0).astype(np.int64) - (v < 0.0).astype(np.int64)
        changes += (sg != 0) & (prev != 0) & (sg != prev)
        prev = np.where(sg != 0, sg, prev)
    return changes


def cubic_roots(c, ok=None):
    """The real roots of the scaled cubics c (B, 4) by the routine of section 21 at degree 3.  Returns (z (B, 3) ascending, n_roots
    (B,), ok (B,))."""
    c = np.array(c, dtype=np.float64)
    B = len(c)
    ok = np.ones(B, bool) if ok is None else ok.copy()
    with np.errstate(all="ignore"):
        ok &= np.abs(c[:, 3]) > LEAD_TOL
        bound = 1.0 + np.abs(c[:, :3] / c[:, 3:]).max(1)
        chain = np.zeros((B, 4, 4))
        for s in np.flatnonzero(ok):
            chain[s], good = sturm_chain([float(v) for v in c[s]])
            ok[s] &= good
        bound = np.where(ok, bound, 1.0)
        c = np.where(ok[:, None], c, 0.0)
        v_low = sign_changes(chain, -bound[:, None])[:, 0]
        n_roots = np.clip(v_low - sign_changes(chain, bound[:, None])[:, 0], 0, 3)
        n_roots[~ok] = 0
        k = np.arange(3)[None, :]
        lo, hi = np.repeat(-bound[:, None], 3, 1), np.repeat(bound[:, None], 3, 1)
        for _ in range(BISECT):
            mid = 0.5 * (lo + hi)
            left = v_low[:, None] - sign_changes(chain, mid) >= k + 1
            hi, lo = np.where(left, mid, hi), np.where(left, lo, mid)
        z = 0.5 * (lo + hi)
        for _ in range(NEWTON):
            p, dp = np.repeat(c[:, 3:], 3, 1), np.zeros_like(z)
            for j in range(2, -1, -1):
                dp = dp * z + p
                p = p * z + c[:, j, None]
            zn = z - p / dp
            z = np.where((zn >= lo) & (zn <= hi), zn, z)
    return z, n_roots, ok


def seven_point(rec, details=False):
    """rec (B, 7, 4): the records (x1, y1, x2, y2) of B samples.  Returns (F (B, 3, 9), valid (B, 3)): the fundamental matrix of
    every real root, roots ascending.  details: also a dict with A, B (B, 9), c (B, 4), roots (B, 3), n_roots (B,), ok (B,)."""
    rec = np.asarray(rec, dtype=np.float64)
    Bn = len(rec)
    with np.errstate(all="ignore"):
        u1, v1, u2, v2 = (rec[:, :, m] for m in range(4))
        M = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones_like(u1)], 2)
        ok, u = null_space(M)
        A, B = (u[:, 0] + u[:, 1]) * RSQRT2, (u[:, 0] - u[:, 1]) * RSQRT2
        c = cubic(A, B)
        big = np.abs(c).max(1)
        ok &= (big > 0.0) & np.isfinite(big)
        c = c / big[:, None]
        z, n_roots, ok = cubic_roots(np.where(ok[:, None], c, 0.0), ok)
        valid = np.arange(3)[None, :] < n_roots[:, None]
        F = z[:, :, None] * A[:, None, :] + B[:, None, :]
        d = np.zeros((Bn, 3))
        for m in range(9):
            d = d + F[:, :, m] * F[:, :, m]
        nrm = np.sqrt(d)
        valid &= (nrm > 0.0) & np.isfinite(nrm)
        F = F / nrm[:, :, None]
    if details:
        return F, valid, dict(A=A, B=B, c=c, roots=z, n_roots=n_roots, ok=ok)
    return F, valid


# ---- refinement ----------------------------------------------------------------------------------------------------------------------
def parametrise(F):
    """The rank-2 parametrisation of F (9,): ((i, k, l), x (8,)) with x = (column i, column k, alpha, beta), column l = alpha c_i +
    beta c_k; None where every cross product vanishes or the 2 x 2 determinant is not positive."""
    G = np.asarray(F, dtype=np.float64).reshape(3, 3)
    best, cols = 0.0, None
    for i, k in ((0, 1), (0, 2), (1, 2)):
        cr = np.cross(G[:, i], G[:, k])
        d = (cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2]
        if d > best:
            best, cols = d, (i, k, 3 - i - k)
    if cols is None or not np.isfinite(best):
        return None
    a, b, l = G[:, cols[0]], G[:, cols[1]], G[:, cols[2]]
    dot = lambda p, q: (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]
    g11, g12, g22, r1, r2 = dot(a, a), dot(a, b), dot(b, b), dot(a, l), dot(b, l)
    det = g11 * g22 - g12 * g12
    if not det > 0.0 or not np.isfinite(det):
        return None
    return cols, np.concatenate([a, b, [(r1 * g22 - r2 * g12) / det, (g11 * r2 - g12 * r1) / det]])


def build(cols, x):
    """F (9,) of the state x under the columns (i, k, l)."""
    G = np.zeros((3, 3))
    G[:, cols[0]], G[:, cols[1]] = x[0:3], x[3:6]
    G[:, cols[2]] = x[6] * x[0:3] + x[7] * x[3:6]
    return G.reshape(9)


def f_residuals(F, rec):
    """Signed Sampson residuals x2^t F x1 / sqrt(D), or None where a denominator is not positive."""
    F = np.asarray(F).reshape(3, 3)
    x1 = np.concatenate([rec[:, :2], np.ones((len(rec), 1))], 1)
    x2 = np.concatenate([rec[:, 2:], np.ones((len(rec), 1))], 1)
    a, b = x1 @ F.T, x2 @ F
    D = a[:, 0] ** 2 + a[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2
    if not ((D > 0.0) & np.isfinite(D)).all():
        return None
    return (x2 * a).sum(1) / np.sqrt(D)


def f_jacobian(cols, x, rec):
    """d residuals / d x: (n, 8), analytic."""
    F = build(cols, x).reshape(3, 3)
    i, k, l = cols
    dF = np.zeros((8, 3, 3))
    for r in range(3):
        dF[r, r, i], dF[r, r, l] = 1.0, x[6]
        dF[3 + r, r, k], dF[3 + r, r, l] = 1.0, x[7]
        dF[6, r, l], dF[7, r, l] = x[r], x[3 + r]
    x1 = np.concatenate([rec[:, :2], np.ones((len(rec), 1))], 1)
    x2 = np.concatenate([rec[:, 2:], np.ones((len(rec), 1))], 1)
    a, b = x1 @ F.T, x2 @ F
    N = (x2 * a).sum(1)
    D = a[:, 0] ** 2 + a[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2
    sD = np.sqrt(D)
    J = np.zeros((len(rec), 8))
    for c, G in enumerate(dF):
        f, g = x1 @ G.T, x2 @ G
        dN = (x2 * f).sum(1)
        dD = 2.0 * (a[:, 0] * f[:, 0] + a[:, 1] * f[:, 1] + b[:, 0] * g[:, 0] + b[:, 1] * g[:, 1])
        J[:, c] = dN / sD - 0.5 * (N / sD) * dD / D
    return J


def refine_f(F, rec, o):
    """One refinement of a unit-norm F on the records given (the inliers); returns it re-normalised (F itself where it has no
    parametrisation)."""
    par = parametrise(F)
    if par is None:
        return None
    cols, x = par
    fixed = int(np.argmax(np.abs(x[:6])))                # the first of equals
    free = [m for m in range(8) if m != fixed]

    def sums(y):
        r = f_residuals(build(cols, y), rec)
        if r is None:
            return None, None, np.inf
        J = f_jacobian(cols, y, rec)[:, free]
        return J.T @ J, J.T @ r, float(r @ r)

    def plus(y, d):
        y1 = y.copy()
        y1[free] = y[free] + d
        return y1
    F1 = build(cols, hc.lm(x, sums, plus, o))
    with np.errstate(all="ignore"):
        return F1 / np.sqrt(np.cumsum(F1 * F1)[-1])


def signed(F):
    """F with its entry of largest magnitude positive (the first of equals)."""
    F = np.asarray(F, dtype=np.float64)
    return -F if F.reshape(-1)[int(np.argmax(np.abs(F)))] < 0.0 else F


# ---- the estimator -----------------------------------------------------------------------------------------------------------------
def estimate(xy1, xy2, cam1, cam2, **options):
    """The estimator on one pair; cam = (model, params).  Returns dict(status, F, n_inliers, n_trials, inlier (n,), err (n,),
    usable (n,))."""
    o = {**DEFAULTS, **options}
    xy1, xy2 = np.asarray(xy1, dtype=np.float64).reshape(-1, 2), np.asarray(xy2, dtype=np.float64).reshape(-1, 2)
    k1, k2 = tv._params(*cam1), tv._params(*cam2)
    N = len(xy1)
    uv1, ok1 = ac.image_to_world(cam1[0], k1, xy1)
    uv2, ok2 = ac.image_to_world(cam2[0], k2, xy2)
    usable = ok1 & ok2 & np.isfinite(xy1).all(1) & np.isfinite(xy2).all(1)
    out = dict(status=1, F=None, n_inliers=0, n_trials=0, inlier=np.zeros(N, np.uint8), err=np.full(N, np.nan), usable=usable)
    idx = np.flatnonzero(usable)
    n = len(idx)
    if n < 7:
        return out
    rec = np.concatenate([uv1[idx], uv2[idx]], 1)
    thr = 0.5 * (o["max_error"] / ac.mean_focal(cam1[0], k1) + o["max_error"] / ac.mean_focal(cam2[0], k2))
    thr2 = thr * thr
    max_trials = -(-o["max_num_trials"] // o["round_size"]) * o["round_size"]
    best, done = None, 0
    while True:
        hs = list(range(done, done + o["round_size"]))
        F, valid = seven_point(rec[[list(sample(o["seed"], h, n)) for h in hs]])
        err = sampson(F, rec)                                               # (B, 3, n)
        with np.errstate(invalid="ignore"):
            inl = err <= thr2
        cnt = inl.sum(2)
        tot = np.cumsum(np.where(inl, err, thr2), 2)[:, :, -1]              # (cumsum: the sum in index order)
        for b, root in zip(*np.nonzero(valid)):
            key = (int(cnt[b, root]), -float(tot[b, root]), -hs[b], -int(root))
            if best is None or key > best[0]:
                best = (key, F[b, root].copy())
        done += o["round_size"]
        if done >= max_trials or done >= trials_needed(o, max_trials, best[0][0] if best else -1, n):
            break
    out["n_trials"] = done
    if best is None:
        out["status"] = 2
        return out
    F = best[1]
    with np.errstate(invalid="ignore"):
        cur = sampson(F, rec) <= thr2
    cur_cnt = int(cur.sum())
    for _ in range(o["lo_rounds"]):
        F1 = refine_f(F, rec[cur], o)
        if F1 is None:
            break
        with np.errstate(invalid="ignore"):
            new = sampson(F1, rec) <= thr2
        if not new.sum() >= cur_cnt:
            break
        changed = bool((new != cur).any())
        F, cur, cur_cnt = F1, new, int(new.sum())
        if not changed:
            break
    out["status"] = 3
    if cur_cnt < need_inliers(o, n):
        return out
    e2 = sampson(F, rec)
    out.update(status=0, F=signed(F), n_inliers=cur_cnt)
    out["inlier"][idx] = cur
    with np.errstate(invalid="ignore"):
        out["err"][idx] = np.sqrt(e2) * (o["max_error"] / thr)
    return out


NAMES = ("F", "status", "n_inliers", "n_trials", "inlier", "err")


def reference(batch, **options):
    """The estimator on every pair of a batch (the dict engine.FundamentalProblem takes).  Arrays like the kernel's outputs; F is
    NaN where status is not 0."""
    off = np.asarray(batch["pair_offsets"])
    T = len(off) - 1
    res = dict(F=np.full((T, 9), np.nan), status=np.zeros(T, np.int32), n_inliers=np.zeros(T, np.int32), n_trials=np.zeros(T, np.int32),
               inlier=np.zeros(off[-1], np.uint8), err=np.full(off[-1], np.nan))
    for p in range(T):
        c1, c2 = batch["pair_camera"][p]
        r = estimate(batch["xy1"][off[p]:off[p + 1]], batch["xy2"][off[p]:off[p + 1]], (int(batch["cam_model"][c1]), batch["cam_params"][c1]),
                     (int(batch["cam_model"][c2]), batch["cam_params"][c2]), **options)
        for k in ("status", "n_inliers", "n_trials"):
            res[k][p] = r[k]
        if r["status"] == 0:
            res["F"][p] = r["F"]
        res["inlier"][off[p]:off[p + 1]] = r["inlier"]
        res["err"][off[p]:off[p + 1]] = r["err"]
    return res


# ---- pairs -------------------------------------------------------------------------------------------------------------------------
def scale_focal(model, params, s):
    """The parameters of a camera whose focal length(s) are stated s times too long."""
    k = np.array(params, dtype=np.float64)
    k[:1 if int(model) in tc.SINGLE_FOCAL else 2] *= s
    return k


def make_pairs(kinds, counts, models, seed, focal_scale=None, sigma=0.5, p_outlier=0.3, min_outlier=20.0):
    """hc.make_pairs (pair i of kinds[i] with counts[i] matches through cameras models[i % L] and models[(i + 1) % L]), generated
    with the true cameras, and a camera table of its own per pair for the cameras *handed to the estimator*: pair i names cameras
    2 i and 2 i + 1, the true ones with their focal lengths multiplied by focal_scale[i] (None: 1 everywhere).  Returns the batch
    dict + kind, true_inlier, focal_scale."""
    T, L = len(counts), len(models)
    fs = np.ones(T) if focal_scale is None else np.asarray(focal_scale, dtype=np.float64)
    g = hc.make_pairs(kinds, counts, models, seed, sigma=sigma, p_outlier=p_outlier, min_outlier=min_outlier)
    cam_model, cam_params = [], []
    for i in range(T):
        for m in (int(models[i % L]), int(models[(i + 1) % L])):
            cam_model.append(m)
            cam_params.append(scale_focal(m, tc.MODEL_PARAMS[m], fs[i]))
    return dict(pair_offsets=g["pair_offsets"], xy1=g["xy1"], xy2=g["xy2"], pair_camera=np.arange(2 * T, dtype=np.int32).reshape(T, 2),
                cam_model=np.array(cam_model, np.int32), cam_params=tc.pad_params(cam_params), kind=g["kind"],
                true_inlier=g["true_inlier"], focal_scale=fs)


single = tv.single


def true_fundamental(R, t):
    """F = [t]x R of a relative pose in the normalised planes, Frobenius norm 1, signed like the kernel's."""
    E = tv.essential_of_pose(R, t).reshape(9)
    return signed(E / np.linalg.norm(E))


def f_distance(F0, F1):
    """Frobenius norm of the difference of two unit-norm, sign-fixed fundamental matrices."""
    return float(np.linalg.norm(np.asarray(F0).reshape(-1) - np.asarray(F1).reshape(-1)))


def noise_free_samples(B, seed, focal_scale=(0.7, 1.0, 1.4)):
    """B samples of seven noise-free matches, seen through a focal length stated focal_scale[b % 3] times too long on both sides:
    (rec (B, 7, 4), F (B, 9) the true matrix of those planes, unit norm, sign-fixed)."""
    rng = np.random.default_rng(seed)
    rec, Fs = np.zeros((B, 7, 4)), np.zeros((B, 9))
    for b in range(B):
        q, t = tv.random_relative_pose(rng)
        R = synthetic.qvec_to_rotmat(q)
        x1 = rng.uniform(-0.4, 0.4, (7, 2))
        X2 = (np.concatenate([x1, np.ones((7, 1))], 1) * rng.uniform(2.0, 20.0, (7, 1))) @ R.T + t
        s = focal_scale[b % len(focal_scale)]
        rec[b] = np.concatenate([x1, X2[:, :2] / X2[:, 2:]], 1) / s          # x_stated = x_true / s
        K = np.diag([s, s, 1.0])                                             # x_true = K x_stated: F = K^t E K
        Fm = (K @ tv.essential_of_pose(R, t) @ K).reshape(9)
        Fs[b] = signed(Fm / np.linalg.norm(Fm))
    return rec, Fs


# ---- hard families of minimal samples (tests/test_minimal_solvers_*.py) ---------------------------------------------------------
def _sample(rng, n=7, focal=1.0, half_field=0.4, depth=(2.0, 20.0), parallax=None):
    """n noise-free matches of a random relative pose seen through a focal length stated `focal` times too long: (rec (n, 4), F (9,)).
    parallax: the baseline as a fraction of the median depth (None: random_relative_pose's 1-3 units)."""
    q, t = tv.random_relative_pose(rng)
    R = synthetic.qvec_to_rotmat(q)
    x1 = rng.uniform(-half_field, half_field, (n, 2))
    d = rng.uniform(*depth, (n, 1))
    if parallax is not None:
        t = t / np.linalg.norm(t) * parallax * np.median(d)
    X2 = (np.concatenate([x1, np.ones((n, 1))], 1) * d) @ R.T + t
    K = np.diag([focal, focal, 1.0])
    Fm = (K @ tv.essential_of_pose(R, t) @ K).reshape(9)
    return np.concatenate([x1, X2[:, :2] / X2[:, 2:]], 1) / focal, signed(Fm / np.linalg.norm(Fm))


def _slide(rng, crossing):
    """A generic sample whose first match is slid along x2 to a sign change of crossing(rec (B, 7, 4)) -> (B,): (lo, hi, at) with
    at(lo) and at(hi) the samples on either side, one rounding apart."""
    while True:
        rec, _ = _sample(rng)

        def at(lam):
            r = rec.copy()
            r[0, 2] += lam
            return r

        grid = np.linspace(-0.2, 0.2, 81)
        val = crossing(np.array([at(lam) for lam in grid]))
        k = np.flatnonzero(np.sign(val[:-1]) * np.sign(val[1:]) < 0)
        if not len(k):
            continue
        lo, hi = grid[k[0]], grid[k[0] + 1]
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if np.sign(crossing(at(mid)[None])[0]) == np.sign(val[k[0]]) else (lo, mid)
        return lo, hi, at


DOUBLE_ROOT_MARGIN = 1e-8


def _double_root(rng):
    """A sample DOUBLE_ROOT_MARGIN (in the slid coordinate) from where two of the cubic's three real roots merge, on the side that
    has three: the pair is about 1e-4 apart, real beyond doubt and ill-conditioned, the third root is an ordinary one."""
    count = lambda r: seven_point(r, details=True)[2]["n_roots"].astype(np.float64)
    lo, hi, at = _slide(rng, lambda r: count(r) - 2.0)
    lam = lo - DOUBLE_ROOT_MARGIN if count(at(lo)[None])[0] == 3 else hi + DOUBLE_ROOT_MARGIN
    return at(lam), np.full(9, np.nan)


def _small_leading_coefficient(rng, target):
    """A sample whose scaled cubic has the leading coefficient `target` to a few per cent (one root of det(x A + B) runs off to infinity)."""
    lead = lambda r: seven_point(r, details=True)[2]["c"][:, 3]
    while True:
        lo, _, at = _slide(rng, lambda r: lead(r) - target)
        if abs(lead(at(lo)[None])[0] / target - 1.0) < 0.1:
            return at(lo), np.full(9, np.nan)


HARD_FAMILIES = {
    "generic, focal x 0.7": lambda rng: _sample(rng, focal=0.7),
    "generic, focal x 1": lambda rng: _sample(rng, focal=1.0),
    "generic, focal x 1.4": lambda rng: _sample(rng, focal=1.4),
    "parallax 1e-1": lambda rng: _sample(rng, parallax=1e-1),
    "parallax 1e-2": lambda rng: _sample(rng, parallax=1e-2),
    "parallax 1e-3": lambda rng: _sample(rng, parallax=1e-3),
    "parallax 1e-4": lambda rng: _sample(rng, parallax=1e-4),
    # depth spread 1e-3: kappa of F grows with 1 / spread, and at 1e-4 13 % of the solutions lie beyond the 1e-7 cap on C kappa u
    "near-planar": lambda rng: _sample(rng, depth=(8.0 * (1.0 - 1e-3), 8.0 * (1.0 + 1e-3))),
    "narrow field": lambda rng: _sample(rng, half_field=0.008),
    "double root": _double_root,
    "leading coefficient above LEAD_TOL": lambda rng: _small_leading_coefficient(rng, rng.choice([-1.0, 1.0]) * rng.uniform(1.5, 10.0) * LEAD_TOL),
    "leading coefficient below LEAD_TOL": lambda rng: _small_leading_coefficient(rng, rng.choice([-1.0, 1.0]) * rng.uniform(0.1, 0.7) * LEAD_TOL),
}
# families that the solver's own rule declares degenerate: no hypothesis by specification, whatever the problem's conditioning
REFUSED_FAMILIES = ("leading coefficient below LEAD_TOL",)


def hard_family(name, seed, B=64):
    """B samples of a family of HARD_FAMILIES: (rec (B, 7, 4), F (B, 9) the generating matrix, NaN where the family has none)."""
    rng = np.random.default_rng(seed)
    parts = [HARD_FAMILIES[name](rng) for _ in range(B)]
    return np.array([p[0] for p in parts]), np.array([p[1] for p in parts])


def degenerate_samples(seed=0):
    """(rec (4, 7, 4)): a repeated match, seven copies of one match, a coordinate that is not a number, a pure rotation."""
    rng = np.random.default_rng(seed)
    rec = np.array([_sample(rng)[0] for _ in range(4)])
    rec[0, 1] = rec[0, 0]
    rec[1, :] = rec[1, 0]
    rec[2, 0, 2] = np.nan
    R = synthetic.qvec_to_rotmat(tv.random_relative_pose(rng)[0])
    X2 = np.concatenate([rec[3, :, :2], np.ones((7, 1))], 1) @ R.T
    rec[3, :, 2:] = X2[:, :2] / X2[:, 2:]
    return rec


def eleven_models_pairs():
    """tv.eleven_models_pairs: (batch, F (11, 9)) -- one noise-free pair of 40 matches per camera model, and its true F."""
    batch, gq, gt = tv.eleven_models_pairs()
    return batch, np.array([true_fundamental(synthetic.qvec_to_rotmat(q), t) for q, t in zip(gq, gt)])


# ---- the batch the lane emulation and the GPU are both held to ------------------------------------------------------------------
BOUNDARY_COUNTS = (0, 1, 6, 7, 8, 14, 15, 16, 63, 64, 65, 255, 256, 257, LDS_MATCHES - 1, LDS_MATCHES, LDS_MATCHES + 1, 2 * LDS_MATCHES + 7)
PLANAR_COUNT = 64                     # the one planar pair: a degenerate family for seven points
POSE_CAP, ERR_CAP = tv.POSE_CAP, tv.ERR_CAP
# 1000 x the largest differences measured between the kernel's source run lane by lane on the CPU and this reference on the
# boundary batch (tests/test_fundamental_lanes_cpu.py, where the measured values are written down): room for the device's sqrt /
# divide sequences
F_TOL = min(1000 * 2.9e-15, POSE_CAP)          # Frobenius norm of the difference of the unit-norm, sign-fixed matrices
ERR_TOL = min(1000 * 4.6e-13, ERR_CAP)         # pixels, of the per-match Sampson distances

BOUNDARY_SEED = 1      # one for which the reference ends at the generated inlier set on every general pair of >= 15


def boundary_inputs():
    """The batch of boundary_batch() without its reference."""
    kinds = ["general"] * (2 * len(BOUNDARY_COUNTS)) + ["planar"]
    counts = np.array(list(BOUNDARY_COUNTS) * 2 + [PLANAR_COUNT], np.int64)
    order = np.random.default_rng(11).permutation(len(counts))
    # Every third pair of the shuffled batch is handed focal lengths that are off, x 0.7 and x 1.4 in turn.  These are the pairs of
    # a PINHOLE and a SIMPLE_RADIAL camera (positions 0 mod 3 of the model cycle), and deliberately so: a fisheye camera read with
    # a wrong focal length maps tan(theta) to tan(theta / s), which no fundamental matrix relates to anything, so such a pair
    # could not promise its generated inlier set; the radial term (k = 0.05) read at the wrong radius leaves a residual of a
    # pixel or two that the 4 px threshold covers for the seed chosen below.
    scale = np.ones(len(counts))
    scale[0::6], scale[3::6] = 0.7, 1.4
    assert len(counts) == 37 and len(counts) % 4 != 0
    return make_pairs([kinds[i] for i in order], counts[order], (1, 2, 8), seed=BOUNDARY_SEED, focal_scale=scale, p_outlier=0.3)


@functools.lru_cache(maxsize=None)
def boundary_batch():
    """(batch, reference): two general pairs of every match count around the minimal sample, min_num_inliers, the wavefront, the
    workgroup and the LDS capacity S, and one planar pair, shuffled -- 37 pairs, not a multiple of 4 -- with 30 % outliers, a
    pinhole, a radial and a fisheye camera, every third pair handed focal lengths off by x 0.7 or x 1.4."""
    batch = boundary_inputs()
    return batch, reference(batch)


def check_reference(batch, ref):
    """What the boundary batch promises of the reference alone: every status, and the generated inlier set on every general pair
    of >= 15 matches (no pair excused), whatever focal length it was handed.  The planar pair is held to nothing here."""
    counts = np.diff(batch["pair_offsets"])
    general = np.array(batch["kind"]) == "general"
    assert {0, 1, 3}.issubset(set(ref["status"]))
    assert (ref["status"][general & (counts >= 15)] == 0).all() and (ref["status"][general & (counts < 7)] == 1).all()
    assert (ref["status"][general & (counts >= 7) & (counts < 15)] == 3).all()
    assert set(batch["focal_scale"][general & (counts >= 15)]) == {0.7, 1.0, 1.4}
    m = np.repeat(general, counts)
    want = batch["true_inlier"] & np.repeat(counts >= 15, counts)
    assert np.array_equal(ref["inlier"].astype(bool)[m], want[m])


def compare(got, ref, report=None):
    """got / ref: dicts of host arrays (NAMES).  Everything discrete is equal, no pair excused; F within F_TOL, errors within
    ERR_TOL, NaN patterns equal.  Returns (max F difference, max err diff)."""
    for k in ("status", "n_inliers", "n_trials", "inlier"):
        assert np.array_equal(got[k], ref[k]), k
    ok = ref["status"] == 0
    assert np.isnan(got["F"][~ok]).all()
    dF = [f_distance(ref["F"][i], got["F"][i]) for i in np.flatnonzero(ok)]
    assert np.array_equal(np.isnan(got["err"]), np.isnan(ref["err"]))
    have = ~np.isnan(ref["err"])
    worst = (max(dF, default=0.0), np.abs(got["err"][have] - ref["err"][have]).max() if have.any() else 0.0)
    print("%smax F difference %.3e, max error difference %.3e px" % (report or "", *worst))
    assert np.abs(np.linalg.norm(got["F"][ok], axis=1) - 1.0).max() <= 1e-12
    big = np.argmax(np.abs(got["F"][ok]), 1)
    assert (got["F"][ok][np.arange(ok.sum()), big] > 0).all()
    assert worst[0] <= F_TOL and worst[1] <= ERR_TOL
    return worst


# ---- the pairs api.TwoViewClassifier is held to with "fundamental" set ---------------------------------------------------------------
WRONG_FOCAL = 0.7
CLASSIFIER_SEED = 1


@functools.lru_cache(maxsize=None)
def uncalibrated_batch():
    """(batch, F reference, E reference, H reference): SIMPLE_PINHOLE pairs of 200 matches with 30 % outliers -- two general
    pairs with their true focal length, the same two handed the focal length x WRONG_FOCAL, a planar and a rotation-only pair.
    CLASSIFIER_SEED is one for which the essential-matrix reference loses more than 5 % of the fundamental matrix's inliers on
    both pairs with the wrong focal length (most general pairs do, not all: some geometries do not constrain the focal length)."""
    kinds = ["general"] * 4 + ["planar", "rotation"]
    g = hc.make_pairs(["general"] * 2 + ["planar", "rotation"], [200] * 4, (0,), seed=CLASSIFIER_SEED, p_outlier=0.3)
    off = g["pair_offsets"]
    take = [0, 1, 0, 1, 2, 3]
    scale = np.array([1.0, 1, WRONG_FOCAL, WRONG_FOCAL, 1, 1])
    sl = [slice(off[p], off[p + 1]) for p in take]
    T = len(take)
    batch = dict(pair_offsets=np.arange(T + 1, dtype=np.int64) * 200, xy1=np.concatenate([g["xy1"][s] for s in sl]),
                 xy2=np.concatenate([g["xy2"][s] for s in sl]), pair_camera=np.stack([np.arange(T), np.arange(T)], 1).astype(np.int32),
                 cam_model=np.zeros(T, np.int32), cam_params=tc.pad_params([scale_focal(0, tc.MODEL_PARAMS[0], s) for s in scale]),
                 kind=kinds, true_inlier=np.concatenate([g["true_inlier"][s] for s in sl]), focal_scale=scale)
    return batch, reference(batch), tv.reference(batch), hc.reference(batch)
