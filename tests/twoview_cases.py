"""Helper of the two-view geometry tests (not collected): a numpy reference of the per-pair estimator, written from its
specification (include/pixsfm_hip.h) and not from the kernel, and a generator of image pairs.

    samples   draw d of sample h = mix(mix(seed + G (h + 1)) + G (d + 1)) mod n (the hash of section 19), repeated indices drawn
              again, the five used in ascending order
    solver    Nister's five-point: null space by Gauss-Jordan (orthonormalised, mixed), the ten cubics as polynomial products, Gauss-Jordan, det B(z) of
              degree 10, Sturm chain + bisection + Newton with + - x / only, E by back-substitution, then Gauss-Newton
              steps to convergence (at most eight) over (x, y, z) on the ten cubic constraints of the 3 x 3 matrix itself
    score     squared Sampson error in the normalised plane, inlier iff err <= thr^2; key (count, -sum min(err, thr^2), -h, -root)
    stop      after every round: samples done >= clamp(log(1 - confidence) / log(1 - w^5), min_num_trials, max_num_trials)
    pose      Horn's closed form, the pose of four with the most inliers in front of both cameras
    LO        Levenberg-Marquardt on the signed Sampson residuals of the inliers over (rotation, direction of t), classify, repeat

The solver runs on all samples of a round at once (arrays with a leading sample axis): every element sees the operations the
specification states, in its order, so a sample's numbers do not depend on the round it is in.
"""
import functools

import numpy as np

import abspose_cases as ac
import pxo
import triangulation_cases as tc
from pixsfm_amd import synthetic

DEFAULTS = dict(max_error=4.0, min_inlier_ratio=0.25, min_num_inliers=15, confidence=0.999, min_num_trials=64, max_num_trials=10000,
                round_size=64, seed=0, refine_max_iterations=100, lo_rounds=4)
LDS_MATCHES = 1024     # PXR_TWOVIEW_LDS_MATCHES: the staged-in-LDS capacity S of the kernel (include/pixsfm_hip.h)
IMAGE = ac.IMAGE
PIVOT_TOL, LEAD_TOL, TRIM_TOL = 1e-12, 1e-9, 1e-12
BISECT, NEWTON = 64, 4
POLISH = 8             # at most this many Gauss-Newton steps on the ten cubic constraints over (x, y, z), per hypothesis (TV_POLISH)
POLISH_TOL = 1e-10     # the last step: one of at most this size, relative to max(1, |x|, |y|, |z|) (quadratic convergence: what is left is rounding)

# ---- samples and the stop rule: ac's, for samples of five --------------------------------------------------------------------------
sample = functools.partial(ac.sample, k=5)
trials_needed = functools.partial(ac.trials_needed, k=5)


# ---- polynomials in (x, y, z, 1) = variables 0 .. 3 -------------------------------------------------------------------------------
PAIRS = [(i, j) for i in range(4) for j in range(i, 4)]
TRIPLES = [(i, j, k) for i in range(4) for j in range(i, 4) for k in range(j, 4)]
PAIR_INDEX = {p: x for x, p in enumerate(PAIRS)}
# Nister's column order: x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x | yz^2 yz y | z^3 z^2 z 1
NISTER = [(0, 0, 0), (1, 1, 1), (0, 0, 1), (0, 1, 1), (0, 0, 2), (0, 0, 3), (1, 1, 2), (1, 1, 3), (0, 1, 2), (0, 1, 3),
          (0, 2, 2), (0, 2, 3), (0, 3, 3), (1, 2, 2), (1, 2, 3), (1, 3, 3), (2, 2, 2), (2, 2, 3), (2, 3, 3), (3, 3, 3)]
COLUMN = {t: x for x, t in enumerate(NISTER)}


def mul11(a, b, out):
    """out (.., 10) += a (.., 4) b (.., 4)"""
    for i in range(4):
        for j in range(4):
            out[..., PAIR_INDEX[(min(i, j), max(i, j))]] += a[..., i] * b[..., j]


def mul21(p, a, row):
    """row (.., 20, Nister's order) += p (.., 10) a (.., 4)"""
    for i in range(4):
        for j in range(i, 4):
            for k in range(4):
                row[..., COLUMN[tuple(sorted((i, j, k)))]] += p[..., PAIR_INDEX[(i, j)]] * a[..., k]


def gauss_jordan(M):
    """Gauss-Jordan with partial pivoting on the first `rows` columns of M (B, rows, cols), in place.  Returns ok (B,)."""
    B, rows, cols = M.shape
    ar = np.arange(B)
    S = np.abs(M).reshape(B, -1).max(1)
    ok = np.isfinite(S)
    for c in range(rows):
        col = np.abs(M[:, c:, c])
        pr = c + np.argmax(col, 1)                   # the first of equals, like a scan with >
        ok &= col[ar, pr - c] > PIVOT_TOL * S
        tmp = M[ar, c, :].copy()
        M[ar, c, :] = M[ar, pr, :]
        M[ar, pr, :] = tmp
        p = M[:, c, c].copy()
        M[:, c, c:] = M[:, c, c:] / p[:, None]
        f = M[:, :, c].copy()
        f[:, c] = 0.0
        M[:, :, c + 1:] = M[:, :, c + 1:] - f[:, :, None] * M[:, None, c, c + 1:]
        M[:, :, c] = 0.0
        M[:, c, c] = 1.0
    return ok


def null_space(A):
    """The null space of A (B, 5, 9): Gauss-Jordan with full pivoting -> [I | C] in permuted columns, vector k = (-C[:, k], e_k),
    orthonormalised by modified Gram-Schmidt in the order k = 0 .. 3.  Returns (ok (B,), u (B, 4, 9))."""
    A = A.copy()
    B = len(A)
    ar = np.arange(B)
    S = np.abs(A).reshape(B, -1).max(1)
    ok = np.isfinite(S)
    perm = np.tile(np.arange(9), (B, 1))
    for c in range(5):
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
    u = np.zeros((B, 4, 9))
    for k in range(4):
        v = np.zeros((B, 9))
        for r in range(5):
            v[ar, perm[:, r]] = -A[:, r, 5 + k]
        v[ar, perm[:, 5 + k]] = 1.0
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


def sturm_chain(c):
    """The Sturm chain of one polynomial c (11 ascending coefficients, plain floats): p, p', then minus the remainder of the two
    before, each scaled to a largest coefficient of 1.  Returns (chain (11, 11) zero-padded, ok)."""
    chain = np.zeros((11, 11))
    polys = [list(c), [(k + 1) * c[k + 1] for k in range(10)]]
    while len(polys) <= 10 and len(polys[-1]) > 1:
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
    """chain (B, 11, 11), x (B, K): sign changes of every chain at every x (zeros skipped)."""
    changes = np.zeros(x.shape, np.int64)
    prev = np.zeros(x.shape, np.int64)
    for i in range(11):
        v = np.broadcast_to(chain[:, i, 10, None], x.shape).copy()
        for k in range(9, -1, -1):
            v = v * x + chain[:, i, k, None]
        sg = (v > 0.0).astype(np.int64) - (v < 0.0).astype(np.int64)
        changes += (sg != 0) & (prev != 0) & (sg != prev)
        prev = np.where(sg != 0, sg, prev)
    return changes


def _cofactors(E):
    """The cofactor matrix of E (.., 3, 3): d det(E) / dE."""
    c = np.zeros_like(E)
    for i in range(3):
        for j in range(3):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            c[..., i, j] = E[..., i1, j1] * E[..., i2, j2] - E[..., i1, j2] * E[..., i2, j1]
    return c


def polish_essential(x, y, z, basis):
    """Up to POLISH Gauss-Newton steps (until one is no larger than POLISH_TOL) on the ten cubic constraints 2 E E^t E - tr(E E^t) E = 0, det E = 0 of E = x N0 + y N1 + z N2 + N3
    over (x, y, z) (.., each), basis (.., 9, 4): the constraints are evaluated on the 3 x 3 matrix itself, which is well
    conditioned where the elimination to the polynomial in z is not.  The 3 x 3 normal equations of a step by the adjugate; a
    step is skipped where their determinant vanishes or the step is not finite."""
    b = basis.reshape(basis.shape[:-2] + (3, 3, 4))
    T = lambda A: np.swapaxes(A, -1, -2)
    live = np.ones(np.broadcast(x, y, z).shape, bool)
    for _ in range(POLISH):
        E = ((x[..., None, None] * b[..., 0] + y[..., None, None] * b[..., 1]) + z[..., None, None] * b[..., 2]) + b[..., 3]
        M, G = E @ T(E), T(E) @ E
        tr = (M[..., 0, 0] + M[..., 1, 1] + M[..., 2, 2])[..., None, None]
        cof = _cofactors(E)
        det = (E[..., 0, :] * cof[..., 0, :]).sum(-1)
        r = np.concatenate([(2.0 * (M @ E) - tr * E).reshape(E.shape[:-2] + (9,)), det[..., None]], -1)
        cols = []
        for k in range(3):
            D = np.broadcast_to(b[..., k], E.shape)
            dC = 2.0 * ((D @ G + E @ T(D) @ E) + M @ D) - 2.0 * (E * D).sum((-1, -2))[..., None, None] * E - tr * D
            cols.append(np.concatenate([dC.reshape(E.shape[:-2] + (9,)), (cof * D).sum((-1, -2))[..., None]], -1))
        J = np.stack(cols, -1)
        A, g = T(J) @ J, (T(J) @ r[..., None])[..., 0]
        adj = T(_cofactors(A))
        dA = (A[..., 0, :] * T(adj)[..., 0, :]).sum(-1)
        d = (adj @ g[..., None])[..., 0] / dA[..., None]
        ok = live & (dA != 0.0) & np.isfinite(d).all(-1)
        x, y, z = np.where(ok, x - d[..., 0], x), np.where(ok, y - d[..., 1], y), np.where(ok, z - d[..., 2], z)
        size = np.maximum(np.maximum(np.abs(d[..., 0]), np.abs(d[..., 1])), np.abs(d[..., 2]))
        scale = np.maximum(np.maximum(1.0, np.abs(x)), np.maximum(np.abs(y), np.abs(z)))
        live = ok & ~(size <= POLISH_TOL * scale)                 # (a skipped step would only repeat itself)
    return x, y, z


def five_point(rec, details=False, exact=None):
    """rec (B, 5, 4): the records (u1, v1, u2, v2) of B samples.  Returns (E (B, 10, 9), valid (B, 10)): the essential matrix of
    every real root, roots ascending.  details: also a dict with c (B, 11) (zero where a sample is refused; c_scaled: not), roots (B, 10), n_roots (B,), ok (B,).  exact: a dict
    that replaces a stage's result by one computed elsewhere (tools/five_point_stages.py locates a loss of accuracy with
    it): basis (B, 9, 4), rows (B, 10, 20) the constraints before elimination, c (B, 11) the polynomial before scaling."""
    rec = np.asarray(rec, dtype=np.float64)
    B = len(rec)
    with np.errstate(all="ignore"):
        u1, v1, u2, v2 = (rec[:, :, m] for m in range(4))
        A = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones_like(u1)], 2)
        ok, u = null_space(A)
        if not ok.any() and not details:             # (a round of degenerate samples: nothing to solve)
            return np.zeros((B, 10, 9)), np.zeros((B, 10), bool)
        basis = np.zeros((B, 9, 4))
        basis[:, :, 0] = 0.5 * (((u[:, 0] + u[:, 1]) + u[:, 2]) + u[:, 3])
        basis[:, :, 1] = 0.5 * (((u[:, 0] - u[:, 1]) + u[:, 2]) - u[:, 3])
        basis[:, :, 2] = 0.5 * (((u[:, 0] + u[:, 1]) - u[:, 2]) - u[:, 3])
        basis[:, :, 3] = 0.5 * (((u[:, 0] - u[:, 1]) - u[:, 2]) + u[:, 3])
        if exact and "basis" in exact:
            basis = np.array(exact["basis"], dtype=np.float64)
        # the ten cubic constraints
        M = np.zeros((B, 10, 20))
        EEt = {}
        for a in range(3):
            for b in range(a, 3):
                EEt[(a, b)] = np.zeros((B, 10))
                for c in range(3):
                    mul11(basis[:, 3 * a + c], basis[:, 3 * b + c], EEt[(a, b)])
        half_tr = 0.5 * ((EEt[(0, 0)] + EEt[(1, 1)]) + EEt[(2, 2)])
        for a in range(3):
            EEt[(a, a)] = EEt[(a, a)] - half_tr
        for a in range(3):
            for b in range(3):
                for c in range(3):
                    mul21(EEt[(min(a, c), max(a, c))], basis[:, 3 * c + b], M[:, 3 * a + b])
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            pos, neg = np.zeros((B, 10)), np.zeros((B, 10))
            mul11(basis[:, 3 + b], basis[:, 6 + c], pos)
            mul11(basis[:, 3 + c], basis[:, 6 + b], neg)
            mul21(pos - neg, basis[:, a], M[:, 9])
        if exact and "rows" in exact:
            M = np.array(exact["rows"], dtype=np.float64)
        ok &= gauss_jordan(M)
        bx, by, bw = np.zeros((B, 3, 4)), np.zeros((B, 3, 4)), np.zeros((B, 3, 5))
        for r in range(3):
            e, f = M[:, 4 + 2 * r], M[:, 5 + 2 * r]
            bx[:, r] = np.stack([e[:, 12], e[:, 11] - f[:, 12], e[:, 10] - f[:, 11], -f[:, 10]], 1)
            by[:, r] = np.stack([e[:, 15], e[:, 14] - f[:, 15], e[:, 13] - f[:, 14], -f[:, 13]], 1)
            bw[:, r] = np.stack([e[:, 19], e[:, 18] - f[:, 19], e[:, 17] - f[:, 18], e[:, 16] - f[:, 17], -f[:, 16]], 1)
        m0, m1, m2, c = np.zeros((B, 8)), np.zeros((B, 8)), np.zeros((B, 7)), np.zeros((B, 11))
        for i in range(4):
            for j in range(5):
                m0[:, i + j] += by[:, 1, i] * bw[:, 2, j] - by[:, 2, i] * bw[:, 1, j]
                m1[:, i + j] += bx[:, 1, i] * bw[:, 2, j] - bx[:, 2, i] * bw[:, 1, j]
        for i in range(4):
            for j in range(4):
                m2[:, i + j] += bx[:, 1, i] * by[:, 2, j] - by[:, 1, i] * bx[:, 2, j]
        for i in range(4):
            for j in range(8):
                c[:, i + j] += bx[:, 0, i] * m0[:, j] - by[:, 0, i] * m1[:, j]
        for i in range(5):
            for j in range(7):
                c[:, i + j] += bw[:, 0, i] * m2[:, j]
        if exact and "c" in exact:
            c = np.array(exact["c"], dtype=np.float64)
        big = np.abs(c).max(1)
        ok &= (big > 0.0) & np.isfinite(big)
        c = c / big[:, None]
        ok &= np.abs(c[:, 10]) > LEAD_TOL
        bound = 1.0 + np.abs(c[:, :10] / c[:, 10:]).max(1)
        chain = np.zeros((B, 11, 11))
        for s in np.flatnonzero(ok):
            chain[s], good = sturm_chain([float(v) for v in c[s]])
            ok[s] &= good
        bound = np.where(ok, bound, 1.0)
        c_scaled = c
        c = np.where(ok[:, None], c, 0.0)
        v_low = sign_changes(chain, -bound[:, None])[:, 0]
        n_roots = np.clip(v_low - sign_changes(chain, bound[:, None])[:, 0], 0, 10)
        n_roots[~ok] = 0
        k = np.arange(10)[None, :]
        lo, hi = np.repeat(-bound[:, None], 10, 1), np.repeat(bound[:, None], 10, 1)
        for _ in range(BISECT):
            mid = 0.5 * (lo + hi)
            left = v_low[:, None] - sign_changes(chain, mid) >= k + 1
            hi, lo = np.where(left, mid, hi), np.where(left, lo, mid)
        z = 0.5 * (lo + hi)
        for _ in range(NEWTON):
            p, dp = np.repeat(c[:, 10:], 10, 1), np.zeros_like(z)
            for j in range(9, -1, -1):
                dp = dp * z + p
                p = p * z + c[:, j, None]
            zn = z - p / dp
            z = np.where((zn >= lo) & (zn <= hi), zn, z)
        valid = k < n_roots[:, None]
        # back-substitution
        Bz = np.zeros((B, 10, 3, 3))
        for r in range(3):
            Bz[:, :, r, 0] = ((bx[:, None, r, 3] * z + bx[:, None, r, 2]) * z + bx[:, None, r, 1]) * z + bx[:, None, r, 0]
            Bz[:, :, r, 1] = ((by[:, None, r, 3] * z + by[:, None, r, 2]) * z + by[:, None, r, 1]) * z + by[:, None, r, 0]
            Bz[:, :, r, 2] = (((bw[:, None, r, 4] * z + bw[:, None, r, 3]) * z + bw[:, None, r, 2]) * z + bw[:, None, r, 1]) * z + bw[:, None, r, 0]
        best = np.zeros((B, 10, 3))
        for a, b in ((0, 1), (0, 2), (1, 2)):
            w = Bz[:, :, a, 0] * Bz[:, :, b, 1] - Bz[:, :, a, 1] * Bz[:, :, b, 0]
            cr = np.stack([Bz[:, :, a, 1] * Bz[:, :, b, 2] - Bz[:, :, a, 2] * Bz[:, :, b, 1],
                           Bz[:, :, a, 2] * Bz[:, :, b, 0] - Bz[:, :, a, 0] * Bz[:, :, b, 2], w], 2)
            best = np.where((np.abs(w) > np.abs(best[:, :, 2]))[:, :, None], cr, best)
        valid &= np.abs(best[:, :, 2]) > 0.0
        x, y = best[:, :, 0] / best[:, :, 2], best[:, :, 1] / best[:, :, 2]
        start = valid & np.isfinite(x) & np.isfinite(y)
        x, y, zp = polish_essential(np.where(start, x, 0.0), np.where(start, y, 0.0), np.where(start, z, 0.0), basis[:, None])
        z_poly = z
        x, y, z = np.where(start, x, np.nan), np.where(start, y, np.nan), np.where(start, zp, z)
        E = ((x[:, :, None] * basis[:, None, :, 0] + y[:, :, None] * basis[:, None, :, 1]) + z[:, :, None] * basis[:, None, :, 2]) + basis[:, None, :, 3]
        valid &= np.isfinite(x) & np.isfinite(y) & np.isfinite(E).all(2)
    if details:
        return E, valid, dict(c=c, c_scaled=c_scaled, roots=z_poly, n_roots=n_roots, ok=ok)           # (the polynomial's roots, before the polish)
    return E, valid


def sampson(E, rec):
    """Squared Sampson error of records rec (n, 4) under E (.., 9): (.., n)."""
    E = np.asarray(E)[..., None, :]
    u1, v1, u2, v2 = (rec[:, m] for m in range(4))
    with np.errstate(all="ignore"):
        a0 = (E[..., 0] * u1 + E[..., 1] * v1) + E[..., 2]
        a1 = (E[..., 3] * u1 + E[..., 4] * v1) + E[..., 5]
        a2 = (E[..., 6] * u1 + E[..., 7] * v1) + E[..., 8]
        b0 = (E[..., 0] * u2 + E[..., 3] * v2) + E[..., 6]
        b1 = (E[..., 1] * u2 + E[..., 4] * v2) + E[..., 7]
        N = (u2 * a0 + v2 * a1) + a2
        D = ((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1
        return (N * N) / D


# ---- pose ------------------------------------------------------------------------------------------------------------------------
def skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def essential_of_pose(R, t):
    return skew(t) @ R


def horn(E):
    """Horn 1990: (t (unit), Ra, Rb) of an essential matrix E (3, 3), or None.  t t^t = tr(E E^t) / 2 I - E E^t; with E scaled to
    tr(E E^t) = 2: Ra = Cof(E) - [t]x E, Rb = Cof(E) + [t]x E, Cof(E) the matrix of cofactors."""
    EEt = E @ E.T
    half_tr = 0.5 * np.trace(EEt)
    T = half_tr * np.eye(3) - EEt
    m = 0
    for j in (1, 2):
        if T[j, j] > T[m, m]:
            m = j
    if not T[m, m] > 0.0 or not np.isfinite(half_tr):
        return None
    nt = np.sqrt(T[m] @ T[m])
    if not nt > 0.0:
        return None
    t = T[m] / nt
    En = E / np.sqrt(half_tr)
    C = np.stack([np.cross(En[1], En[2]), np.cross(En[2], En[0]), np.cross(En[0], En[1])])
    tE = skew(t) @ En
    Ra, Rb = C - tE, C + tE
    if not (np.isfinite(Ra).all() and np.isfinite(Rb).all()):
        return None
    return t, Ra, Rb


def in_front(R, t, rec):
    """Which records lie in front of both cameras under (R, t): lambda2 x2 = lambda1 R x1 + t, both lambdas positive."""
    x1 = np.concatenate([rec[:, :2], np.ones((len(rec), 1))], 1)
    x2 = np.concatenate([rec[:, 2:], np.ones((len(rec), 1))], 1)
    a = x1 @ R.T
    c, d = np.cross(x2, a), np.cross(x2, np.broadcast_to(t, x2.shape))
    s1, cc = -(c * d).sum(1), (c * c).sum(1)
    p = s1[:, None] * a + cc[:, None] * t
    return (s1 > 0.0) & ((p * x2).sum(1) > 0.0)


def tangent_basis(t):
    m = 0
    for j in (1, 2):
        if abs(t[j]) < abs(t[m]):
            m = j
    b1 = np.cross(t, np.eye(3)[m])
    b1 = b1 / np.sqrt(b1 @ b1)
    return b1, np.cross(t, b1)


def pose_plus(q, t, d):
    """q as section 19 moves it (QuaternionManifold::Plus, re-normalised); t + d3 b1 + d4 b2 back onto the sphere."""
    q1, _ = ac.pose_plus(q, np.zeros(3), np.concatenate([d[:3], np.zeros(3)]))
    b1, b2 = tangent_basis(t)
    t1 = (t + d[3] * b1) + d[4] * b2
    return q1, t1 / np.sqrt(t1 @ t1)


def residuals(q, t, rec):
    """Signed Sampson residuals x2^t E x1 / sqrt(D) of E = [t]x R(q)."""
    E = essential_of_pose(synthetic.qvec_to_rotmat(q), t)
    x1 = np.concatenate([rec[:, :2], np.ones((len(rec), 1))], 1)
    x2 = np.concatenate([rec[:, 2:], np.ones((len(rec), 1))], 1)
    a, b = x1 @ E.T, x2 @ E
    D = a[:, 0] ** 2 + a[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2
    with np.errstate(all="ignore"):
        return (x2 * a).sum(1) / np.sqrt(D)


def jacobian(q, t, rec):
    """d residuals / d (rotation tangent (3), a, b) at zero: (n, 5), analytic."""
    R = synthetic.qvec_to_rotmat(q)
    E = essential_of_pose(R, t)
    b1, b2 = tangent_basis(t)
    dE = [skew(t) @ (2.0 * skew(np.eye(3)[c]) @ R) for c in range(3)] + [skew(b1) @ R, skew(b2) @ R]
    x1 = np.concatenate([rec[:, :2], np.ones((len(rec), 1))], 1)
    x2 = np.concatenate([rec[:, 2:], np.ones((len(rec), 1))], 1)
    a, b = x1 @ E.T, x2 @ E
    N = (x2 * a).sum(1)
    D = a[:, 0] ** 2 + a[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2
    sD = np.sqrt(D)
    J = np.zeros((len(rec), 5))
    for c, F in enumerate(dE):
        f, g = x1 @ F.T, x2 @ F
        dN = (x2 * f).sum(1)
        dD = 2.0 * (a[:, 0] * f[:, 0] + a[:, 1] * f[:, 1] + b[:, 0] * g[:, 0] + b[:, 1] * g[:, 1])
        J[:, c] = dN / sD - 0.5 * (N / sD) * dD / D
    return J


def normal_equations(q, t, rec):
    r = residuals(q, t, rec)
    if not np.isfinite(r).all():
        return None, None, np.inf
    J = jacobian(q, t, rec)
    return J.T @ J, J.T @ r, float(r @ r)


def refine(q, t, rec, o):
    """Levenberg-Marquardt on the matches given (the inliers), lambda and the keep / refuse rule of section 19."""
    H, g, cost = normal_equations(q, t, rec)
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
        H1, g1, cost1 = normal_equations(q1, t1, rec)
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
def _params(model, params):
    return np.asarray(params, dtype=np.float64)[:pxo.lib().pxo_camera_num_params(int(model))]


def estimate(xy1, xy2, cam1, cam2, prior=None, **options):
    """The estimator on one pair; cam = (model, params), prior = (qvec, tvec) or None.  Returns dict(status, qvec, tvec, E,
    n_inliers, n_trials, inlier (n,), err (n,), usable (n,))."""
    o = {**DEFAULTS, **options}
    xy1, xy2 = np.asarray(xy1, dtype=np.float64).reshape(-1, 2), np.asarray(xy2, dtype=np.float64).reshape(-1, 2)
    k1, k2 = _params(*cam1), _params(*cam2)
    N = len(xy1)
    uv1, ok1 = ac.image_to_world(cam1[0], k1, xy1)
    uv2, ok2 = ac.image_to_world(cam2[0], k2, xy2)
    usable = ok1 & ok2 & np.isfinite(xy1).all(1) & np.isfinite(xy2).all(1)
    out = dict(status=1, qvec=None, tvec=None, E=None, n_inliers=0, n_trials=0, inlier=np.zeros(N, np.uint8), err=np.full(N, np.nan),
               usable=usable)
    idx = np.flatnonzero(usable)
    n = len(idx)
    if n < 5:
        return out
    rec = np.concatenate([uv1[idx], uv2[idx]], 1)
    thr = 0.5 * (o["max_error"] / ac.mean_focal(cam1[0], k1) + o["max_error"] / ac.mean_focal(cam2[0], k2))
    thr2 = thr * thr
    max_trials = -(-o["max_num_trials"] // o["round_size"]) * o["round_size"]

    if prior is not None:
        q, t = np.asarray(prior[0], dtype=np.float64), np.asarray(prior[1], dtype=np.float64)
        out["status"] = 2
        if not (np.isfinite(q).all() and np.isfinite(t).all() and q @ q > 0 and t @ t > 0):
            return out
        q_out, t_out = q.copy(), t.copy()
        t = t * (1.0 / np.sqrt(t @ t))
    else:
        best, done = None, 0
        while True:
            hs = list(range(done, done + o["round_size"]))
            E, valid = five_point(rec[[list(sample(o["seed"], h, n)) for h in hs]])
            err = sampson(E, rec)                                           # (B, 10, n)
            with np.errstate(invalid="ignore"):
                inl = err <= thr2
            cnt = inl.sum(2)
            tot = np.cumsum(np.where(inl, err, thr2), 2)[:, :, -1]          # (cumsum: the sum in index order)
            for b, root in zip(*np.nonzero(valid)):
                key = (int(cnt[b, root]), -float(tot[b, root]), -hs[b], -int(root))
                if best is None or key > best[0]:
                    best = (key, E[b, root].copy())
            done += o["round_size"]
            if done >= max_trials or done >= trials_needed(o, max_trials, best[0][0] if best else -1, n):
                break
        out["n_trials"] = done
        if best is None:
            out["status"] = 2
            return out
        E0 = best[1]
        with np.errstate(invalid="ignore"):
            cur = sampson(E0, rec) <= thr2
        out["status"] = 3
        dec = horn(E0.reshape(3, 3))
        if dec is None:
            return out
        t, Ra, Rb = dec
        poses = [(Ra, t), (Ra, -t), (Rb, t), (Rb, -t)]
        front = [int(in_front(R, tt, rec[cur]).sum()) for R, tt in poses]
        R, t = poses[int(np.argmax(front))]                                 # (argmax: the first of equals)
        q = synthetic.rotmat_to_qvec(R)
        q = q / np.linalg.norm(q)
        cur_cnt = int(cur.sum())
        for _ in range(o["lo_rounds"]):
            q1, t1 = refine(q.copy(), t.copy(), rec[cur], o)
            with np.errstate(invalid="ignore"):
                new = sampson(essential_of_pose(synthetic.qvec_to_rotmat(q1), t1).reshape(9), rec) <= thr2
            if new.sum() < cur_cnt:
                break
            changed = bool((new != cur).any())
            q, t, cur, cur_cnt = q1, t1, new, int(new.sum())
            if not changed:
                break
        q_out, t_out = (-q if q[0] < 0 else q), t
    Ef = essential_of_pose(synthetic.qvec_to_rotmat(q), t).reshape(9)
    e2 = sampson(Ef, rec)
    with np.errstate(invalid="ignore"):
        fin = e2 <= thr2
    out["status"] = 3
    if fin.sum() < max(o["min_num_inliers"], int(np.ceil(o["min_inlier_ratio"] * n))):
        return out
    out.update(status=0, qvec=q_out, tvec=t_out, E=Ef, n_inliers=int(fin.sum()))
    out["inlier"][idx] = fin
    out["err"][idx] = np.sqrt(e2) * (o["max_error"] / thr)
    return out


NAMES = ("qvec", "tvec", "E", "status", "n_inliers", "n_trials", "inlier", "err")


def reference(batch, **options):
    """The estimator on every pair of a batch (the dict engine.TwoViewProblem takes).  Arrays like the kernel's outputs; qvec /
    tvec / E are NaN where status is not 0."""
    off = np.asarray(batch["pair_offsets"])
    T = len(off) - 1
    res = dict(qvec=np.full((T, 4), np.nan), tvec=np.full((T, 3), np.nan), E=np.full((T, 9), np.nan), status=np.zeros(T, np.int32),
               n_inliers=np.zeros(T, np.int32), n_trials=np.zeros(T, np.int32), inlier=np.zeros(off[-1], np.uint8),
               err=np.full(off[-1], np.nan))
    for p in range(T):
        c1, c2 = batch["pair_camera"][p]
        prior = (batch["prior_qvec"][p], batch["prior_tvec"][p]) if batch.get("prior_qvec") is not None else None
        r = estimate(batch["xy1"][off[p]:off[p + 1]], batch["xy2"][off[p]:off[p + 1]], (int(batch["cam_model"][c1]), batch["cam_params"][c1]),
                     (int(batch["cam_model"][c2]), batch["cam_params"][c2]), prior=prior, **options)
        res["status"][p], res["n_inliers"][p], res["n_trials"][p] = r["status"], r["n_inliers"], r["n_trials"]
        if r["status"] == 0:
            res["qvec"][p], res["tvec"][p], res["E"][p] = r["qvec"], r["tvec"], r["E"]
        res["inlier"][off[p]:off[p + 1]] = r["inlier"]
        res["err"][off[p]:off[p + 1]] = r["err"]
    return res


def pose_distance(q0, t0, q1, t1):
    """(rotation angle in radians, angle between the translation directions in radians) between two relative poses."""
    ang, _ = ac.pose_distance(q0, t0, q1, t1)
    a, b = np.asarray(t0) / np.linalg.norm(t0), np.asarray(t1) / np.linalg.norm(t1)
    return ang, float(np.arctan2(np.linalg.norm(np.cross(a, b)), a @ b))


# ---- pairs -------------------------------------------------------------------------------------------------------------------------
def random_relative_pose(rng):
    """A second camera that still sees what the first sees: a rotation of up to 0.25 rad, a baseline of 1-3 units."""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    half = 0.5 * rng.uniform(0.02, 0.25)
    q = np.concatenate([[np.cos(half)], np.sin(half) * axis])
    t = rng.normal(size=3)
    t *= rng.uniform(1.0, 3.0) / np.linalg.norm(t)
    return q, t


def sampson_px(q, t, cam1, cam2, xy1, xy2, max_error=4.0):
    """Sampson distance in pixels (the kernel's d_err) of matches under the pose (q, t)."""
    k1, k2 = _params(*cam1), _params(*cam2)
    uv1, _ = ac.image_to_world(cam1[0], k1, xy1)
    uv2, _ = ac.image_to_world(cam2[0], k2, xy2)
    thr = 0.5 * (max_error / ac.mean_focal(cam1[0], k1) + max_error / ac.mean_focal(cam2[0], k2))
    E = essential_of_pose(synthetic.qvec_to_rotmat(q), np.asarray(t) / np.linalg.norm(t)).reshape(9)
    return np.sqrt(sampson(E, np.concatenate([uv1, uv2], 1))) * (max_error / thr)


def make_pairs(counts, models, seed, sigma=0.5, p_outlier=0.3, min_outlier_sampson=20.0):
    """A batch of pairs: pair i has counts[i] matches, its first camera is models[i % L], its second models[(i + 1) % L]
    (tc.MODEL_PARAMS).  Camera 1 sits at the origin; the points are pixels spread over image 1 at depths 2-12; camera 2 is a
    random_relative_pose; only points in front of it and inside its image are kept.  An inlier is the true projection plus
    Gaussian noise of sigma clipped at 3 sigma, on both sides; floor(p_outlier n) matches (p_outlier: a number or one per pair;
    none in pairs of fewer than 20, and never so many that fewer than 15 inliers remain) are outliers: their second pixel is
    uniform in the image, at a Sampson distance of at least min_outlier_sampson px under the true geometry (None: no condition).
    Returns the batch dict + gt_qvec, gt_tvec, true_inlier."""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, dtype=np.int64)
    p_out = np.broadcast_to(np.asarray(p_outlier, dtype=np.float64), counts.shape)
    L = len(models)
    cam_model = np.array(models, np.int32)
    cam_params = tc.pad_params([tc.MODEL_PARAMS[m] for m in models])
    xy1, xy2, inl, gq, gt = [], [], [], [], []
    W, H = IMAGE
    for i, n in enumerate(counts):
        cam1 = (int(models[i % L]), np.array(tc.MODEL_PARAMS[models[i % L]], dtype=np.float64))
        cam2 = (int(models[(i + 1) % L]), np.array(tc.MODEL_PARAMS[models[(i + 1) % L]], dtype=np.float64))
        while True:                                        # a pose under which at least a fifth of the candidates is seen by both
            q, t = random_relative_pose(rng)
            R = synthetic.qvec_to_rotmat(q)
            pix1, pix2 = np.zeros((0, 2)), np.zeros((0, 2))
            for _ in range(8):
                if len(pix1) >= n:
                    break
                m = 2 * int(n) + 16
                cand = np.stack([rng.uniform(0.05 * W, 0.95 * W, m), rng.uniform(0.05 * H, 0.95 * H, m)], 1)
                uv, ok = ac.image_to_world(cam1[0], cam1[1], cand)
                assert ok.all()
                X2 = (np.concatenate([uv, np.ones((m, 1))], 1) * rng.uniform(2.0, 12.0, (m, 1))) @ R.T + t
                with np.errstate(all="ignore"):
                    x, y = ac.world_to_image(cam2[0], cam2[1], X2[:, 0] / X2[:, 2], X2[:, 1] / X2[:, 2])
                seen = (X2[:, 2] > 0.5) & (x >= 0) & (x <= W) & (y >= 0) & (y <= H)
                pix1, pix2 = np.concatenate([pix1, cand[seen]]), np.concatenate([pix2, np.stack([x, y], 1)[seen]])
            if len(pix1) >= n:
                pix1, pix2 = pix1[:n], pix2[:n]
                break
        noise = lambda: np.clip(rng.normal(0, sigma, (n, 2)), -3 * sigma, 3 * sigma) if sigma > 0 else np.zeros((n, 2))
        obs1, obs2 = pix1 + noise(), pix2 + noise()
        bad = np.zeros(n, bool)
        if n >= 20:
            bad[rng.permutation(n)[:min(int(p_out[i] * n), n - 15)]] = True
        for j in np.flatnonzero(bad):
            while True:
                c = np.array([rng.uniform(0, W), rng.uniform(0, H)])
                if min_outlier_sampson is None or sampson_px(q, t, cam1, cam2, obs1[j:j + 1], c[None])[0] >= min_outlier_sampson:
                    break
            obs2[j] = c
        xy1.append(obs1); xy2.append(obs2); inl.append(~bad); gq.append(q); gt.append(t / np.linalg.norm(t))
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    cat = lambda parts: np.concatenate(parts).reshape(-1, 2) if len(parts) else np.zeros((0, 2))
    pair_camera = np.stack([np.arange(len(counts)) % L, (np.arange(len(counts)) + 1) % L], 1).astype(np.int32)
    return dict(pair_offsets=off, xy1=cat(xy1), xy2=cat(xy2), pair_camera=pair_camera, cam_model=cam_model, cam_params=cam_params,
                gt_qvec=np.array(gq).reshape(-1, 4), gt_tvec=np.array(gt).reshape(-1, 3),
                true_inlier=np.concatenate(inl) if len(inl) else np.zeros(0, bool))


def single(batch, p):
    """Pair p of a batch as a batch of its own."""
    off = batch["pair_offsets"]
    s = slice(off[p], off[p + 1])
    return dict(batch, pair_offsets=np.array([0, off[p + 1] - off[p]], np.int64), xy1=batch["xy1"][s], xy2=batch["xy2"][s],
                pair_camera=batch["pair_camera"][p:p + 1])


def noise_free_samples(B, seed):
    """B samples of five noise-free matches in the normalised plane: (rec (B, 5, 4), R (B, 3, 3), t (B, 3))."""
    rng = np.random.default_rng(seed)
    rec, Rs, ts = np.zeros((B, 5, 4)), np.zeros((B, 3, 3)), np.zeros((B, 3))
    for b in range(B):
        q, t = random_relative_pose(rng)
        R = synthetic.qvec_to_rotmat(q)
        x1 = rng.uniform(-0.4, 0.4, (5, 2))
        X2 = (np.concatenate([x1, np.ones((5, 1))], 1) * rng.uniform(2.0, 20.0, (5, 1))) @ R.T + t
        rec[b] = np.concatenate([x1, X2[:, :2] / X2[:, 2:]], 1)
        Rs[b], ts[b] = R, t / np.linalg.norm(t)
    return rec, Rs, ts


# ---- hard families of minimal samples (tests/test_minimal_solvers_*.py) ---------------------------------------------------------
def unit_essential(R, t):
    """[t]x R as 9 numbers of unit norm, its entry of largest magnitude positive (fundamental_cases.signed)."""
    E = essential_of_pose(R, t).reshape(9)
    E = E / np.linalg.norm(E)
    return -E if E[int(np.argmax(np.abs(E)))] < 0.0 else E


def _sample(rng, n=5, half_field=0.4, depth=(2.0, 20.0), parallax=None, planar=False, motion=None, angle=None):
    """n noise-free matches of a relative pose in the normalised planes: (rec (n, 4), E (9,)).  parallax: the baseline as a
    fraction of the median depth (None: random_relative_pose's 1-3 units); planar: the points on one random plane; motion:
    "forward" (the baseline along the optical axis) or "sideways" (along x, no rotation); angle: the rotation angle in radians."""
    q, t = random_relative_pose(rng)
    if angle is not None:
        axis = q[1:] / np.linalg.norm(q[1:])
        q = np.concatenate([[np.cos(0.5 * angle)], np.sin(0.5 * angle) * axis])
    if motion == "forward":
        t = np.array([0.0, 0.0, np.linalg.norm(t)])
    if motion == "sideways":
        q, t = np.array([1.0, 0.0, 0.0, 0.0]), np.array([np.linalg.norm(t), 0.0, 0.0])
    R = synthetic.qvec_to_rotmat(q)
    x1 = np.concatenate([rng.uniform(-half_field, half_field, (n, 2)), np.ones((n, 1))], 1)
    d = rng.uniform(*depth, (n, 1))
    if planar:
        nrm = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), 1.0])
        d = rng.uniform(*depth) / (x1 @ nrm)[:, None]
    if parallax is not None:
        t = t / np.linalg.norm(t) * parallax * np.median(d)
    X2 = (x1 * d) @ R.T + t
    return np.concatenate([x1[:, :2], X2[:, :2] / X2[:, 2:]], 1), unit_essential(R, t)


def _slide(rng, value, level):
    """A generic sample whose first match is slid along x2 to where value(rec (B, 5, 4)) -> (B,) crosses `level` (a number, or a
    function of the values on the grid that first brackets the crossing): (lo, hi, at) with at(lo) and at(hi) the samples on
    either side, one rounding apart."""
    while True:
        rec, _ = _sample(rng)

        def at(lam):
            r = rec.copy()
            r[0, 2] += lam
            return r

        grid = np.linspace(-0.2, 0.2, 81)
        val = value(np.array([at(lam) for lam in grid]))
        lev = level(val) if callable(level) else level
        k = np.flatnonzero(np.sign(val[:-1] - lev) * np.sign(val[1:] - lev) < 0)
        if not len(k):
            continue
        lo, hi = grid[k[0]], grid[k[0] + 1]
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if np.sign(value(at(mid)[None])[0] - lev) == np.sign(val[k[0]] - lev) else (lo, mid)
        return lo, hi, at


DOUBLE_ROOT_MARGIN = 1e-8


def _double_root(rng):
    """A sample DOUBLE_ROOT_MARGIN (in the slid coordinate) from where two real roots of the polynomial merge, on the side that
    has them: the pair is about 1e-4 apart, real beyond doubt and ill-conditioned, the other roots are ordinary ones."""
    count = lambda r: five_point(r, details=True)[2]["n_roots"].astype(np.float64)
    lo, hi, at = _slide(rng, count, lambda val: val.min() + 1.0)        # (a sample has 0, 2, .. 10 real roots)
    lam = lo - DOUBLE_ROOT_MARGIN if count(at(lo)[None])[0] > count(at(hi)[None])[0] else hi + DOUBLE_ROOT_MARGIN
    return at(lam), np.full(9, np.nan)


def _small_leading_coefficient(rng, target):
    """A sample whose scaled polynomial has the leading coefficient `target` to a few per cent (one root in z runs off to infinity)."""
    lead = lambda r: five_point(r, details=True)[2]["c_scaled"][:, 10]
    while True:
        lo, _, at = _slide(rng, lead, target)
        if abs(lead(at(lo)[None])[0] / target - 1.0) < 0.1:
            return at(lo), np.full(9, np.nan)


HARD_FAMILIES = {
    "generic": _sample,
    "parallax 1e-1": lambda rng: _sample(rng, parallax=1e-1),
    "parallax 1e-2": lambda rng: _sample(rng, parallax=1e-2),
    "parallax 1e-3": lambda rng: _sample(rng, parallax=1e-3),
    "parallax 1e-4": lambda rng: _sample(rng, parallax=1e-4),
    "planar scene": lambda rng: _sample(rng, planar=True),
    "forward motion": lambda rng: _sample(rng, motion="forward"),
    "sideways, no rotation": lambda rng: _sample(rng, motion="sideways"),
    "rotation 1e-4": lambda rng: _sample(rng, angle=1e-4),
    "wide field": lambda rng: _sample(rng, half_field=2.0),
    "narrow field": lambda rng: _sample(rng, half_field=0.01),
    "double root": _double_root,
    "leading coefficient above LEAD_TOL": lambda rng: _small_leading_coefficient(rng, rng.choice([-1.0, 1.0]) * rng.uniform(1.5, 10.0) * LEAD_TOL),
    "leading coefficient below LEAD_TOL": lambda rng: _small_leading_coefficient(rng, rng.choice([-1.0, 1.0]) * rng.uniform(0.1, 0.7) * LEAD_TOL),
}
PARALLAX_FAMILIES = {"parallax 1e-1": 1e-1, "parallax 1e-2": 1e-2, "parallax 1e-3": 1e-3, "parallax 1e-4": 1e-4}
# The smallest tested parallax (baseline / median depth) at and above which every well-conditioned solution of every sample is
# returned within the bound of tests/test_minimal_solvers_cpu.py.  Measured there (64 samples per decade, after the Gauss-Newton
# polish): at 1e-1 all 322 solutions are met; at 1e-2 the elimination to det B(z) loses 4 of 328, at 1e-3 64 of 328, at 1e-4
# 174 of 318 -- whole roots, which no polish of the roots that are found returns.
FIVE_POINT_MIN_PARALLAX = 1e-1
# families that the solver's own rule declares degenerate: no hypothesis by specification, whatever the problem's conditioning
REFUSED_FAMILIES = ("leading coefficient below LEAD_TOL",)


def hard_family(name, seed, B=64):
    """B samples of a family of HARD_FAMILIES: (rec (B, 5, 4), E (B, 9) the generating matrix, NaN where the family has none)."""
    rng = np.random.default_rng(seed)
    parts = [HARD_FAMILIES[name](rng) for _ in range(B)]
    return np.array([p[0] for p in parts]), np.array([p[1] for p in parts])


def degenerate_samples(seed=0):
    """(rec (4, 5, 4)): a repeated match, five copies of one match, a coordinate that is not a number, a pure rotation."""
    rng = np.random.default_rng(seed)
    rec = np.array([_sample(rng)[0] for _ in range(4)])
    rec[0, 1] = rec[0, 0]
    rec[1, :] = rec[1, 0]
    rec[2, 0, 2] = np.nan
    R = synthetic.qvec_to_rotmat(random_relative_pose(rng)[0])
    X2 = np.concatenate([rec[3, :, :2], np.ones((5, 1))], 1) @ R.T
    rec[3, :, 2:] = X2[:, :2] / X2[:, 2:]
    return rec


def eleven_models_pairs():
    """(batch, gt_qvec, gt_tvec): one noise-free pair of 40 matches per camera model, its second camera the next model."""
    models = sorted(tc.MODEL_PARAMS)
    rng = np.random.default_rng(31)
    xy1, xy2, gq, gt = [], [], [], []
    ident = np.array([1.0, 0, 0, 0])
    for i, m in enumerate(models):
        m2 = models[(i + 1) % len(models)]
        q, t = random_relative_pose(rng)
        X1 = np.concatenate([rng.uniform(-0.3, 0.3, (40, 2)), np.ones((40, 1))], 1) * rng.uniform(2, 20, (40, 1))
        k1, k2 = (np.array(tc.MODEL_PARAMS[x], dtype=np.float64) for x in (m, m2))
        xy1.append(np.array([pxo.world_to_pixel(m, k1, ident, np.zeros(3), x, jac=False)[0] for x in X1]))
        xy2.append(np.array([pxo.world_to_pixel(m2, k2, q, t, x, jac=False)[0] for x in X1]))
        gq.append(q); gt.append(t / np.linalg.norm(t))
    L = len(models)
    batch = dict(pair_offsets=np.arange(L + 1, dtype=np.int64) * 40, xy1=np.concatenate(xy1), xy2=np.concatenate(xy2),
                 pair_camera=np.stack([np.arange(L), (np.arange(L) + 1) % L], 1).astype(np.int32), cam_model=np.array(models, np.int32),
                 cam_params=tc.pad_params([tc.MODEL_PARAMS[m] for m in models]))
    return batch, gq, gt


# ---- the batch the lane emulation and the GPU are both held to ------------------------------------------------------------------
BOUNDARY_COUNTS = (0, 1, 4, 5, 6, 14, 15, 16, 63, 64, 65, 255, 256, 257, LDS_MATCHES - 1, LDS_MATCHES, LDS_MATCHES + 1, 2 * LDS_MATCHES + 7)
POSE_CAP, ERR_CAP = 1e-7, 1e-6      # section 19's bounds: no bound of this estimator may exceed them
# 1000 x the largest differences measured between the kernel's source run lane by lane on the CPU and this reference on the
# boundary batch (tests/test_twoview_lanes_cpu.py, where the measured values are written down): room for the device's sqrt /
# divide sequences
POSE_TOL = min(1000 * 1.1e-15, POSE_CAP)       # rotation angle and angle between the translation directions, radians
ERR_TOL = min(1000 * 3.5e-13, ERR_CAP)         # pixels, of the per-match Sampson distances


BOUNDARY_SEED = 12     # one for which the reference ends at the generated inlier set on every pair (asserted by the tests)


def boundary_inputs():
    """The batch of boundary_batch() without its reference (tools/geometry_fingerprint.py)."""
    counts = np.repeat(BOUNDARY_COUNTS, 3)
    np.random.default_rng(11).shuffle(counts)
    assert len(counts) == 54 and len(counts) % 4 != 0
    return make_pairs(counts, (1, 2, 8), seed=BOUNDARY_SEED, p_outlier=0.3)


@functools.lru_cache(maxsize=None)
def boundary_batch():
    """(batch, reference): match counts around the minimal sample, min_num_inliers, the wavefront, the workgroup and the LDS
    capacity S, three pairs each, shuffled -- 54 pairs, not a multiple of 4 -- with 30 % outliers, a pinhole, a radial and a
    fisheye camera."""
    batch = boundary_inputs()
    return batch, reference(batch)


def compare(got, ref, report=None):
    """got / ref: dicts of host arrays (NAMES).  Everything discrete is equal, no pair excused; poses within POSE_TOL, errors
    within ERR_TOL, NaN patterns equal.  Returns (max rotation angle, max translation angle, max err diff)."""
    assert np.array_equal(got["status"], ref["status"])
    assert np.array_equal(got["n_inliers"], ref["n_inliers"])
    assert np.array_equal(got["n_trials"], ref["n_trials"])
    assert np.array_equal(got["inlier"], ref["inlier"])
    ok = ref["status"] == 0
    assert np.isnan(got["qvec"][~ok]).all() and np.isnan(got["tvec"][~ok]).all() and np.isnan(got["E"][~ok]).all()
    d = np.array([pose_distance(ref["qvec"][i], ref["tvec"][i], got["qvec"][i], got["tvec"][i]) for i in np.flatnonzero(ok)]).reshape(-1, 2)
    assert np.array_equal(np.isnan(got["err"]), np.isnan(ref["err"]))
    have = ~np.isnan(ref["err"])
    worst = (d[:, 0].max() if len(d) else 0.0, d[:, 1].max() if len(d) else 0.0,
             np.abs(got["err"][have] - ref["err"][have]).max() if have.any() else 0.0)
    print("%smax rotation difference %.3e rad, max translation-direction difference %.3e rad, max error difference %.3e px"
          % (report or "", *worst))
    assert (got["qvec"][ok][:, 0] >= 0).all() and np.abs(np.linalg.norm(got["qvec"][ok], axis=1) - 1.0).max() <= 1e-12
    assert np.abs(np.linalg.norm(got["tvec"][ok], axis=1) - 1.0).max() <= 1e-12
    assert np.abs(np.linalg.norm(got["E"][ok], axis=1) - np.sqrt(2.0)).max() <= 1e-12
    assert worst[0] <= POSE_TOL and worst[1] <= POSE_TOL and worst[2] <= ERR_TOL
    return worst
