"""Helper of the minimal-solver tests (not collected): references of the minimal problems in mpmath at DIGITS digits, written from
the mathematical definition of each problem and sharing no elimination order, tolerance or constant with the kernels or with
the numpy restatements of tests/*_cases.py.

    P3P          the three cosine-law equations in the distances (s1, s2, s3).  With x = s2 / s1, y = s3 / s1 two conics remain;
                 their resultant in x is a quartic in y (polyroots).  Every real y with either x of the second conic starts a
                 Newton iteration on the three equations themselves; what converges with positive distances is a solution
                 (equal ones counted once).  Pose: R maps the triad (e1, e2, e1 x e2) of the world points to that of s_i f_i.
    seven-point  null space of the 7 x 9 system from a QR factorisation of its transpose, the cubic det(x A + (1 - x) B)
                 interpolated through four values, polyroots, F = x A + (1 - x) B at every real root.
    four-point   the null vector of the 8 x 9 system from a QR factorisation of its transpose.
    five-point   null space from QR, turned by a fixed orthogonal matrix; the ten cubic constraints read as a 10 x 10 matrix C(z) over
                 the monomials of (x, y) (hidden variable z); det C(z) interpolated through 11 values, polyroots, the null vector
                 of C(z) at every real root.

A root counts as real where |imaginary part| < 1e-30 |root|; nothing else decides what a solution is.

Per solution also kappa, the 2-norm of d(model) / d(sample coordinates): central differences with step 1e-20 of the solution
followed through the perturbed problem by one Newton step on the defining equations from the unperturbed solution (quadratic
convergence: what is left after the step is of order 1e-40, far below the difference itself).

attainable_*: the error level that double precision can reach on a sample -- three Newton steps in double on the defining
equations, started from the mp solution rounded to double.  The tests' constants C are set from it.
"""
import functools

import mpmath as mp
import numpy as np

DIGITS = 60
U = 2.0 ** -53                     # unit roundoff of double
STEP = mp.mpf(10) ** -20
REAL_TOL = mp.mpf(10) ** -30


# ---- arithmetic that works on mpf and on float alike -------------------------------------------------------------------------------
def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _mp(a):
    return [mp.mpf(float(v)) for v in np.asarray(a, dtype=np.float64).reshape(-1)]


def _np(a):
    return np.array([float(v) for v in a])


def _is_real(z):
    return z == 0 or abs(mp.im(z)) < REAL_TOL * abs(z)


def _solve(A, b):
    """A (list of rows) x = b; None where A is singular."""
    try:
        return list(mp.lu_solve(mp.matrix(A), mp.matrix(b)))
    except ZeroDivisionError:
        return None


def _solve3(A, b):
    """The 3 x 3 system A x = b by the adjugate (any arithmetic); None where the determinant vanishes."""
    c0, c1, c2 = _cross(A[1], A[2]), _cross(A[2], A[0]), _cross(A[0], A[1])
    det = _dot(A[0], c0)
    if det == 0:
        return None
    return [(c0[i] * b[0] + c1[i] * b[1] + c2[i] * b[2]) / det for i in range(3)]


def _two_norm(J):
    J = np.array([[float(v) for v in row] for row in J])
    return float(np.linalg.norm(J, 2)) if np.isfinite(J).all() else np.inf


def _central(fun, x):
    """d fun / d x (rows: outputs) by central differences with STEP."""
    cols = []
    for j in range(len(x)):
        hi, lo = list(x), list(x)
        hi[j], lo[j] = x[j] + STEP, x[j] - STEP
        a, b = fun(hi), fun(lo)
        cols.append([(p - q) / (2 * STEP) for p, q in zip(a, b)])
    return [[cols[j][i] for j in range(len(x))] for i in range(len(cols[0]))]


def _implicit(G, m, x):
    """(kappa, G_m as a float array) of the solution m of G(m, x) = 0: d m / d x = -G_m^-1 G_x, which is the central difference of
    m followed by one Newton step."""
    Gm = _central(lambda mm: G(mm, x), m)
    Gx = _central(lambda xx: G(m, xx), x)
    try:
        J = mp.inverse(mp.matrix(Gm)) * mp.matrix(Gx)
    except ZeroDivisionError:
        return np.inf, None
    return _two_norm([[J[i, j] for j in range(J.cols)] for i in range(J.rows)]), np.array([[float(v) for v in r] for r in Gm])


def _newton_double(G, Gm, m, x, steps=3):
    m, x = np.array(m, dtype=np.float64), [float(v) for v in x]
    for _ in range(steps):
        r = np.array([float(v) for v in G([float(v) for v in m], x)])
        m = m - np.linalg.solve(Gm, r)
    return m


# ---- P3P ---------------------------------------------------------------------------------------------------------------------------
def _p3p_geometry(x, sqrt):
    """x: 15 sample coordinates (u1 v1 u2 v2 u3 v3, X1 X2 X3).  Unit bearings, the world points, 1 - cos of the angles (alpha,
    beta, gamma) opposite points 1, 2, 3 and the squared sides (a2, b2, c2) they face."""
    f = []
    for i in range(3):
        u, v = x[2 * i], x[2 * i + 1]
        n = sqrt(u * u + v * v + 1)
        f.append([u / n, v / n, 1 / n])
    X = [list(x[6 + 3 * i:9 + 3 * i]) for i in range(3)]
    h = tuple(_dot(e, e) / 2 for e in (_sub(f[1], f[2]), _sub(f[0], f[2]), _sub(f[0], f[1])))      # 1 - cos, without the cancellation
    d = (_sub(X[1], X[2]), _sub(X[0], X[2]), _sub(X[0], X[1]))
    return f, X, h, tuple(_dot(e, e) for e in d)


def _p3p_equations(s, h, side2):
    """The law of cosines as (s_i - s_j)^2 + 2 s_i s_j (1 - cos) = side^2."""
    return [(s[1] - s[2]) * (s[1] - s[2]) + 2 * s[1] * s[2] * h[0] - side2[0],
            (s[0] - s[2]) * (s[0] - s[2]) + 2 * s[0] * s[2] * h[1] - side2[1],
            (s[0] - s[1]) * (s[0] - s[1]) + 2 * s[0] * s[1] * h[2] - side2[2]]


def _p3p_jacobian(s, h):
    return [[0, 2 * (s[1] - s[2]) + 2 * s[2] * h[0], 2 * (s[2] - s[1]) + 2 * s[1] * h[0]],
            [2 * (s[0] - s[2]) + 2 * s[2] * h[1], 0, 2 * (s[2] - s[0]) + 2 * s[0] * h[1]],
            [2 * (s[0] - s[1]) + 2 * s[1] * h[2], 2 * (s[1] - s[0]) + 2 * s[0] * h[2], 0]]


def _pose_of_distances(s, f, X):
    """(R rows, t): camera = R world + t with R mapping the world triad (e1, e2, e1 x e2) to the camera's."""
    Q = [[s[i] * f[i][k] for k in range(3)] for i in range(3)]
    a, b = _sub(X[1], X[0]), _sub(X[2], X[0])
    c = _cross(a, b)
    det = _dot(c, c)                                           # det [a b c] = (a x b) . c
    inv = [[v / det for v in _cross(b, c)], [v / det for v in _cross(c, a)], [v / det for v in c]]       # rows of [a b c]^-1
    A, B = _sub(Q[1], Q[0]), _sub(Q[2], Q[0])
    Cc = _cross(A, B)
    R = [[A[i] * inv[0][j] + B[i] * inv[1][j] + Cc[i] * inv[2][j] for j in range(3)] for i in range(3)]
    t = [Q[0][i] - _dot(R[i], X[0]) for i in range(3)]
    return R, t


def _poly_mul(a, b):
    out = [mp.mpf(0)] * (len(a) + len(b) - 1)
    for i, p in enumerate(a):
        for j, q in enumerate(b):
            out[i + j] = out[i + j] + p * q
    return out


def _poly_sub(a, b):
    n = max(len(a), len(b))
    a, b = list(a) + [mp.mpf(0)] * (n - len(a)), list(b) + [mp.mpf(0)] * (n - len(b))
    return [p - q for p, q in zip(a, b)]


def _roots(c_ascending):
    c = list(c_ascending)
    while len(c) > 1 and c[-1] == 0:
        c.pop()
    if len(c) < 2:
        return []
    return mp.polyroots(c[::-1], maxsteps=2000, extraprec=8 * mp.mp.prec, error=False)


def p3p(uv, X, kappa=True):
    """All poses of three correspondences (uv (3, 2) normalised image points, X (3, 3)): a list of dict(R (3, 3), t (3,), s (3,)
    as float arrays, kappa, mp=(s, R, t) in mp) in ascending order of s1."""
    with mp.workdps(DIGITS):
        x = _mp(uv) + _mp(X)
        f, Xw, cos, side2 = _p3p_geometry(x, mp.sqrt)
        ca, cb, cg = (1 - v for v in cos)
        a2, b2, c2 = side2
        if a2 == 0 or b2 == 0 or c2 == 0:
            return []
        # the conics in x = s2 / s1 and y = s3 / s1, as polynomials in x whose coefficients are ascending polynomials in y
        p = ([-a2, 2 * a2 * cb, b2 - a2], [mp.mpf(0), -2 * b2 * ca], [b2])
        q = ([c2 - b2, -2 * c2 * cb, c2], [2 * b2 * cg], [-b2])
        r20 = _poly_sub(_poly_mul(p[2], q[0]), _poly_mul(p[0], q[2]))
        r21 = _poly_sub(_poly_mul(p[2], q[1]), _poly_mul(p[1], q[2]))
        r10 = _poly_sub(_poly_mul(p[1], q[0]), _poly_mul(p[0], q[1]))
        res = _poly_sub(_poly_mul(r20, r20), _poly_mul(r21, r10))
        found = []
        for y in _roots(res):
            if not _is_real(y) or mp.re(y) <= 0:
                continue
            y = mp.re(y)
            g = 1 + y * y - 2 * y * cb
            if g <= 0:
                continue
            disc = mp.sqrt(mp.mpc(cg * cg - (1 - c2 * g / b2)))
            for xs in (cg + mp.re(disc), cg - mp.re(disc)):
                s1 = mp.sqrt(b2 / g)
                s = [s1, xs * s1, y * s1]
                good = False
                for _ in range(200):
                    d = _solve3(_p3p_jacobian(s, cos), _p3p_equations(s, cos, side2))
                    if d is None:
                        break
                    s = [a - b for a, b in zip(s, d)]
                    size = max(abs(v) for v in s)
                    if max(abs(v) for v in d) <= mp.mpf(10) ** (8 - DIGITS) * size:
                        good = True
                        break
                if not good or min(s) <= 0:
                    continue
                if any(max(abs(a - b) for a, b in zip(s, o)) <= REAL_TOL * max(o) for o in found):
                    continue
                found.append(s)
        out = []
        for s in sorted(found, key=lambda v: v[0]):
            R, t = _pose_of_distances(s, f, Xw)
            sol = dict(R=np.array([[float(v) for v in r] for r in R]), t=_np(t), s=_np(s), kappa=None, mp=(s, R, t))
            if kappa:
                tn = 1 + mp.sqrt(_dot(t, t))

                def model(xx, s=s, tn=tn):
                    ff, XX, cc, ss = _p3p_geometry(xx, mp.sqrt)
                    d = _solve3(_p3p_jacobian(s, cc), _p3p_equations(s, cc, ss))
                    if d is None:
                        return [mp.inf] * 12
                    Rr, tt = _pose_of_distances([a - b for a, b in zip(s, d)], ff, XX)
                    return [v for r in Rr for v in r] + [v / tn for v in tt]

                sol["kappa"] = _two_norm(_central(model, x))
            out.append(sol)
        return out


def pose_error(R, t, R0, t0):
    """|dR|_F + |dt| / (1 + |t0|)."""
    return float(np.linalg.norm(np.asarray(R) - R0) + np.linalg.norm(np.asarray(t) - t0) / (1.0 + np.linalg.norm(t0)))


def attainable_p3p(uv, X, sol):
    """The pose of three Newton steps in double on the cosine-law equations from sol's distances rounded to double."""
    x = [float(v) for v in np.concatenate([np.asarray(uv, dtype=np.float64).reshape(-1), np.asarray(X, dtype=np.float64).reshape(-1)])]
    f, Xw, cos, side2 = _p3p_geometry(x, np.sqrt)
    s = np.array(sol["s"], dtype=np.float64)
    for _ in range(3):
        J = np.array(_p3p_jacobian(list(s), cos), dtype=np.float64)
        s = s - np.linalg.solve(J, np.array(_p3p_equations(list(s), cos, side2)))
    R, t = _pose_of_distances(list(s), f, Xw)
    return np.array(R), np.array(t)


# ---- seven-point -------------------------------------------------------------------------------------------------------------------
def _null_space(rows, k):
    """The last k columns of Q in the QR factorisation of the transposed system: an orthonormal basis of its null space."""
    Q, _ = mp.qr(mp.matrix(rows).T)
    n = Q.rows
    return [[Q[i, n - k + j] for i in range(n)] for j in range(k)]


def _det3(F):
    return (F[0] * (F[4] * F[8] - F[5] * F[7]) - F[1] * (F[3] * F[8] - F[5] * F[6]) + F[2] * (F[3] * F[7] - F[4] * F[6]))


def _epipolar_rows(x, n):
    rows = []
    for i in range(n):
        u1, v1, u2, v2 = x[4 * i:4 * i + 4]
        rows.append([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1])
    return rows


def _seven_equations(F, x):
    return [sum(a * b for a, b in zip(row, F)) for row in _epipolar_rows(x, 7)] + [_det3(F), sum(v * v for v in F) - 1]


def _sign_fixed(F):
    k = max(range(9), key=lambda i: (abs(F[i]), -i))
    return [-v for v in F] if F[k] < 0 else list(F)


def seven_point(rec, kappa=True):
    """All fundamental matrices of seven matches rec (7, 4) = (x1, y1, x2, y2): a list of dict(F (9,) unit norm, sign-fixed like
    fundamental_cases.signed, kappa, Gm) in ascending order of the root."""
    with mp.workdps(DIGITS):
        x = _mp(rec)
        A, B = _null_space(_epipolar_rows(x, 7), 2)
        nodes = [mp.mpf(-1), mp.mpf(0), mp.mpf(1), mp.mpf(2)]
        vals = [_det3([t * a + (1 - t) * b for a, b in zip(A, B)]) for t in nodes]
        c = _solve([[t ** k for k in range(4)] for t in nodes], vals)
        out = []
        for r in sorted((mp.re(z) for z in _roots(c) if _is_real(z))):
            F = [r * a + (1 - r) * b for a, b in zip(A, B)]
            n = mp.sqrt(sum(v * v for v in F))
            F = _sign_fixed([v / n for v in F])
            sol = dict(F=_np(F), kappa=None, Gm=None, mp=F)
            if kappa:
                sol["kappa"], sol["Gm"] = _implicit(_seven_equations, F, x)
            out.append(sol)
        return out


def attainable_seven_point(rec, sol):
    F = _newton_double(_seven_equations, sol["Gm"], sol["F"], np.asarray(rec, dtype=np.float64).reshape(-1))
    return F / np.linalg.norm(F)


# ---- four-point --------------------------------------------------------------------------------------------------------------------
def _four_equations(H, x):
    out = []
    for i in range(4):
        x1, y1, x2, y2 = x[4 * i:4 * i + 4]
        w = H[6] * x1 + H[7] * y1 + H[8]
        out += [H[0] * x1 + H[1] * y1 + H[2] - x2 * w, H[3] * x1 + H[4] * y1 + H[5] - y2 * w]
    return out + [sum(v * v for v in H) - 1]


def four_point(rec, kappa=True):
    """The homography of four matches rec (4, 4): a list of at most one dict(H (9,) unit norm with a positive third component on
    the four points, kappa, Gm); none where the third components have mixed signs or the system has no single null vector."""
    with mp.workdps(DIGITS):
        x = _mp(rec)
        rows = []
        for i in range(4):
            x1, y1, x2, y2 = x[4 * i:4 * i + 4]
            rows += [[x1, y1, 1, 0, 0, 0, -x2 * x1, -x2 * y1, -x2], [0, 0, 0, x1, y1, 1, -y2 * x1, -y2 * y1, -y2]]
        try:
            H = _null_space(rows, 1)[0]
        except ZeroDivisionError:
            return []
        w = [H[6] * x[4 * i] + H[7] * x[4 * i + 1] + H[8] for i in range(4)]
        if all(v < 0 for v in w):
            H = [-v for v in H]
        elif not all(v > 0 for v in w):
            return []
        sol = dict(H=_np(H), kappa=None, Gm=None, mp=H)
        if kappa:
            sol["kappa"], sol["Gm"] = _implicit(_four_equations, H, x)
        return [sol]


def attainable_four_point(rec, sol):
    H = _newton_double(_four_equations, sol["Gm"], sol["H"], np.asarray(rec, dtype=np.float64).reshape(-1))
    return H / np.linalg.norm(H)



# ---- five-point --------------------------------------------------------------------------------------------------------------------
# Polynomials in (x, y, z) are dicts {(i, j, k): coefficient}.  E = x N0 + y N1 + z N2 + N3 over an orthonormal null-space basis; the
# ten cubic constraints (det E = 0 and 2 E E^t E - tr(E E^t) E = 0) are read as ten linear equations in the ten monomials of (x, y)
# of degree <= 3 with coefficients that are polynomials in z (the hidden variable, as in Li and Hartley, "Five-point motion
# estimation made easy", ICPR 2006): det C(z) has degree 10, interpolated here through 11 values; at a root the null vector of
# C(z) holds x and y.  No Gauss-Jordan elimination of the 10 x 20 system, no expansion by products.
XY_MONOMIALS = [(3, 0), (0, 3), (2, 1), (1, 2), (2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)]


def _pmul(a, b):
    out = {}
    for ka, va in a.items():
        for kb, vb in b.items():
            k = (ka[0] + kb[0], ka[1] + kb[1], ka[2] + kb[2])
            out[k] = out.get(k, 0) + va * vb
    return out


def _padd(a, b, scale=1):
    out = dict(a)
    for k, v in b.items():
        out[k] = out.get(k, 0) + scale * v
    return out


def _five_constraints(basis):
    """The ten cubics of E = x basis[0] + y basis[1] + z basis[2] + basis[3]: the nine entries of 2 E E^t E - tr(E E^t) E by rows, then det E."""
    E = [[{(1, 0, 0): basis[0][3 * r + c], (0, 1, 0): basis[1][3 * r + c], (0, 0, 1): basis[2][3 * r + c], (0, 0, 0): basis[3][3 * r + c]}
          for c in range(3)] for r in range(3)]
    EEt = [[functools.reduce(_padd, [_pmul(E[a][c], E[b][c]) for c in range(3)]) for b in range(3)] for a in range(3)]
    tr = functools.reduce(_padd, [EEt[a][a] for a in range(3)])
    out = []
    for a in range(3):
        for b in range(3):
            acc = _pmul(tr, E[a][b])
            acc = {k: -v for k, v in acc.items()}
            for c in range(3):
                acc = _padd(acc, _pmul(EEt[a][c], E[c][b]), 2)
            out.append(acc)
    det = {}
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        minor = _padd(_pmul(E[1][b], E[2][c]), _pmul(E[1][c], E[2][b]), -1)
        det = _padd(det, _pmul(E[0][a], minor))
    return out + [det]


def _hidden_matrix(cons, z):
    return [[sum(con.get((i, j, k), 0) * z ** k for k in range(4 - i - j)) for (i, j) in XY_MONOMIALS] for con in cons]


def _skew_times(t, R):
    return [[t[(i + 1) % 3] * R[(i + 2) % 3][j] - t[(i + 2) % 3] * R[(i + 1) % 3][j] for j in range(3)] for i in range(3)]


def _pose_essential(p, frame):
    """[t]x R (rows) at the local pose parameters p = (a, b, c, d, e): R = R(q = (1, a, b, c)) R0 without the division by |q|^2,
    t = t0 + d e1 + e e2.  Any arithmetic."""
    R0, t0, e1, e2 = frame
    a, b, c, d, e = p
    Rq = [[1 + a * a - b * b - c * c, 2 * (a * b - c), 2 * (a * c + b)], [2 * (a * b + c), 1 - a * a + b * b - c * c, 2 * (b * c - a)],
          [2 * (a * c - b), 2 * (b * c + a), 1 - a * a - b * b + c * c]]
    R = [[Rq[i][0] * R0[0][j] + Rq[i][1] * R0[1][j] + Rq[i][2] * R0[2][j] for j in range(3)] for i in range(3)]
    t = [t0[i] + d * e1[i] + e * e2[i] for i in range(3)]
    return _skew_times(t, R)


def _five_equations(p, x, frame):
    E = _pose_essential(p, frame)
    out = []
    for i in range(5):
        u1, v1, u2, v2 = x[4 * i:4 * i + 4]
        l = [E[r][0] * u1 + E[r][1] * v1 + E[r][2] for r in range(3)]
        out.append(u2 * l[0] + v2 * l[1] + l[2])
    return out


def _unit_essential(p, frame, sign, sqrt):
    E = [v for row in _pose_essential(p, frame) for v in row]
    n = sqrt(sum(v * v for v in E))
    return [sign * v / n for v in E]


def _five_frame(E):
    """A pose (R0, t0) with [t0]x R0 proportional to E (rows, mp), two unit vectors spanning the plane across t0, and the sign that
    makes the unit-norm [t0]x R0 equal the unit-norm E."""
    U_, S_, V_ = mp.svd_r(mp.matrix(E))
    if mp.det(U_) < 0:
        U_ = -U_
    if mp.det(V_) < 0:
        V_ = -V_
    W = mp.matrix([[0, -1, 0], [1, 0, 0], [0, 0, 1]])
    R0 = U_ * W * V_
    R0 = [[R0[i, j] for j in range(3)] for i in range(3)]
    t0 = [U_[i, 2] for i in range(3)]
    k = min(range(3), key=lambda i: abs(t0[i]))
    e1 = _cross(t0, [1 if i == k else 0 for i in range(3)])
    n = mp.sqrt(_dot(e1, e1))
    e1 = [v / n for v in e1]
    e2 = _cross(t0, e1)
    frame = (R0, t0, e1, e2)
    flat = [v for row in E for v in row]
    got = _unit_essential([0] * 5, frame, 1, mp.sqrt)
    n = mp.sqrt(sum(v * v for v in flat))
    sign = 1 if sum(a * b for a, b in zip(got, flat)) > 0 else -1
    if not max(abs(sign * a - b / n) for a, b in zip(got, flat)) < mp.mpf(10) ** -20:
        return None, sign           # a multiple root: its null vector is not determined, and what comes out is no essential matrix
    return frame, sign


def _mixed(basis):
    """The basis turned by a fixed orthogonal 4 x 4 matrix without structure (Q of a matrix of small integers).  A motion aligned
    with the axes can leave a solution at infinity in one coordinate of the basis that QR happens to return -- det C(z) then
    drops a degree, and its computed leading coefficient of 1e-60 would come back as a root of 1e59 -- which no aligned motion
    does in a basis turned like this."""
    Q, _ = mp.qr(mp.matrix([[2, -1, 3, 5], [7, 4, -2, 1], [-3, 6, 1, 2], [1, 3, 5, -4]]))
    return [[sum(Q[k, j] * basis[k][m] for k in range(4)) for m in range(9)] for j in range(4)]


def five_point(rec, kappa=True, nister=None):
    """All essential matrices of five matches rec (5, 4) = (x1, y1, x2, y2): (solutions, stages).  solutions: a list of dict(E (9,)
    unit norm, sign-fixed like fundamental_cases.signed, kappa, frame, Gp) in ascending order of z.  stages: the intermediates as
    float arrays -- basis (9, 4) with E = basis . (x, y, z, 1), rows (10, 20) the constraints in the column order `nister` (triples
    of variable indices, 3 for the constant: twoview_cases.NISTER) where given, c (11,) the polynomial in z, ascending, largest
    coefficient 1, z (n,) its real roots."""
    with mp.workdps(DIGITS):
        x = _mp(rec)
        basis = _mixed(_null_space(_epipolar_rows(x, 5), 4))
        cons = _five_constraints(basis)
        nodes = [mp.mpf(k) / 2 for k in range(-5, 6)]
        vals = [mp.det(mp.matrix(_hidden_matrix(cons, t))) for t in nodes]
        c = _solve([[t ** k for k in range(11)] for t in nodes], vals)
        big = max(abs(v) for v in c)
        c = [v / big for v in c]
        stages = dict(basis=np.array([_np(b) for b in basis]).T, c=_np(c))
        if nister is not None:
            rows = np.zeros((10, 20))
            for r, con in enumerate(cons):
                for col, tri in enumerate(nister):
                    rows[r, col] = float(con.get(tuple(sum(1 for v in tri if v == m) for m in range(3)), 0))
            stages["rows"] = rows
        out, zs = [], []
        for z in sorted(mp.re(r) for r in _roots(c) if _is_real(r)):
            Q, _ = mp.qr(mp.matrix(_hidden_matrix(cons, z)).T)
            v = [Q[i, 9] for i in range(10)]
            E = [v[7] * basis[0][m] + v[8] * basis[1][m] + v[9] * (z * basis[2][m] + basis[3][m]) for m in range(9)]      # (x, y, 1) = v[7:] / v[9]
            n = mp.sqrt(sum(e * e for e in E))
            E = _sign_fixed([e / n for e in E])
            sol = dict(E=_np(E), kappa=None, mp=E)
            zs.append(float(z))
            if kappa:
                frame, sign = _five_frame([E[0:3], E[3:6], E[6:9]])
                if frame is None:
                    sol["kappa"] = np.inf
                    out.append(sol)
                    continue
                zero = [mp.mpf(0)] * 5
                Gp = _central(lambda pp: _five_equations(pp, x, frame), zero)
                Gx = _central(lambda xx: _five_equations(zero, xx, frame), x)
                Mp = _central(lambda pp: _unit_essential(pp, frame, sign, mp.sqrt), zero)
                try:
                    J = mp.matrix(Mp) * (mp.inverse(mp.matrix(Gp)) * mp.matrix(Gx))
                    sol["kappa"] = _two_norm([[J[i, j] for j in range(J.cols)] for i in range(J.rows)])
                except ZeroDivisionError:
                    sol["kappa"] = np.inf
                sol["frame"] = tuple([[float(v) for v in r] for r in frame[0]] if i == 0 else [float(v) for v in frame[i]] for i in range(4))
                sol["sign"], sol["Gp"] = sign, np.array([[float(v) for v in r] for r in Gp])
            out.append(sol)
        stages["z"] = np.array(zs)
        return out, stages


def attainable_five_point(rec, sol):
    """Three Newton steps in double on the five epipolar equations over rotation x direction of translation."""
    x = [float(v) for v in np.asarray(rec, dtype=np.float64).reshape(-1)]
    p = np.zeros(5)
    for _ in range(3):
        p = p - np.linalg.solve(sol["Gp"], np.array(_five_equations(list(p), x, sol["frame"])))
    return np.array(_unit_essential(list(p), sol["frame"], sol["sign"], np.sqrt))


# ---- what the CPU and the GPU tests share: the bound and its bookkeeping -----------------------------------------------------------
CAP = 1e-7             # the estimators' cap on any bound (POSE_CAP of twoview_cases): a solution whose bound C kappa u exceeds it is
                       # ill-conditioned by construction, counted and left out


def polynomial_roots(c):
    """The real roots of a polynomial given by its double coefficients c (ascending), in mp, ascending, with the bound that a root
    finder working on Horner's scheme in double can be held to: Horner's value of a polynomial of degree n carries an error of at
    most 2 n u sum |c_k z^k| (Higham, Accuracy and Stability of Numerical Algorithms, section 5.1), so the sign of the computed
    value -- all that bisection and a guarded Newton step see -- is right outside |dz| <= 2 n u sum |c_k z^k| / |p'(z)|, and z
    itself is rounded to u |z|.  Returns [(z, bound)]; the bound is inf at a multiple root."""
    with mp.workdps(DIGITS):
        cm = _mp(c)
        n = len(cm) - 1
        out = []
        for z in sorted(mp.re(r) for r in _roots(cm) if _is_real(r)):
            dp = sum(k * cm[k] * z ** (k - 1) for k in range(1, n + 1))
            mag = sum(abs(cm[k] * z ** k) for k in range(n + 1))
            out.append((float(z), float(2 * n * U * mag / abs(dp) + U * abs(z)) if dp != 0 else np.inf))
        return out


def projective_distance(a, b):
    """Frobenius distance of two matrices known up to scale and sign: both scaled to unit norm, the nearer of the two signs.  Where
    a sign convention is well defined (an entry of largest magnitude without a rival) this is the distance of the sign-fixed
    matrices; [t]x of a motion along an axis has two entries of equal magnitude, and there a convention flips with rounding."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
    return float(min(np.linalg.norm(a - b), np.linalg.norm(a + b)))


def judge(solutions, hypotheses, distance, C):
    """One sample: its mp solutions against the hypotheses a solver returned for it (arrays), with distance(hypothesis, solution).
    Returns (ratios, excluded): err / (kappa u) of the nearest hypothesis for every solution whose bound C kappa u is within CAP
    (inf where there is no hypothesis), and the number of solutions left out."""
    ratios, excluded = [], 0
    for s in solutions:
        if not C * s["kappa"] * U <= CAP:
            excluded += 1
            continue
        err = min([distance(h, s) for h in hypotheses] or [np.inf])
        ratios.append(err / (s["kappa"] * U))
    return ratios, excluded
