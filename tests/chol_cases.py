"""Test systems and error measures for the dense Cholesky (csrc/pxr_chol.hip), pure numpy.

Generators: seeded, return (A, b) with A symmetric float64 and b = rng.normal(n).
Checkers:   componentwise backward-error ratios in units of u = 2^-53, with bounds that come from the rounding-error analysis of
            Cholesky (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Theorems 10.3 / 10.4), never from the
            code under test:
  factor_excess(A, L)          = max_ij |A - L L^T|_ij / (|L| |L^T|)_ij / u     <= n + 8
      gamma_{n+1} for any summation order (inner products of at most n terms plus the square root), plus a handful of further
      roundings per entry that pxr_chol_core.h's factor_panel adds: the correction of v_rsq_f64, d00 * inv0, the 2 x 2
      determinant, multiplication by a reciprocal where the textbook divides.  Evaluated in double (n > 300, sweeps over many
      sizes) the product L L^T itself carries gamma_n |L| |L^T|: bound 2 n + 10.
  solve_excess(A, Lref, x, b)  = max_i |b - A x|_i / (|Lref| |Lref^T| |x|)_i / u <= 3 n + 1
      Theorem 10.4 ((A + dA) x = b with |dA| <= gamma_{3n+1} |L| |L^T|), with the factor LAPACK computes on the right-hand
      side so that the bound does not depend on the factor under test.
"""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble


def _sym(a):
    return 0.5 * (a + a.T)


def random_spd(n, seed):
    """the family of tests/test_chol_gpu.py's first test: M M^T + 1e-3 n I, cond <= ~1e5"""
    rng = np.random.default_rng(seed)
    M = rng.normal(size=(n, n + 5))
    A = M @ M.T + np.eye(n) * 1e-3 * n
    return _sym(A), rng.normal(size=n)


def graded(n, seed):
    """D B D, B well conditioned, D = diag(10^U(-6, 6)): entries over 24 decades -- an absolute tolerance sees only the largest"""
    rng = np.random.default_rng(seed)
    M = rng.normal(size=(n, n))
    B = M @ M.T / n + 1e-3 * np.eye(n)
    d = 10.0 ** rng.uniform(-6.0, 6.0, n)
    return _sym(d[:, None] * B * d[None, :]), rng.normal(size=n)


def illcond(n, seed, k):
    """Q diag(10^(-k i / (n - 1))) Q^T: condition number 10^k, no structure"""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    ev = 10.0 ** (-k * np.arange(n) / max(n - 1, 1))
    return _sym((Q * ev[None, :]) @ Q.T), rng.normal(size=n)


def correlated_pairs(n, seed, eps):
    """T B T^T with T = I except T[2j+1, 2j] = 1, T[2j+1, 2j+1] = eps: columns 2j, 2j+1 -- the two pivots factor_panel takes
    together -- are dependent up to eps (conditional correlation 1 - O(eps^2)), as focal length / distortion columns are"""
    rng = np.random.default_rng(seed)
    M = rng.normal(size=(n, n))
    B = M @ M.T / n + 0.1 * np.eye(n)
    T = np.eye(n)
    for j in range(n // 2):
        T[2 * j + 1, 2 * j] = 1.0
        T[2 * j + 1, 2 * j + 1] = eps
    return _sym(T @ B @ T.T), rng.normal(size=n)


def indefinite_at(n, p, seed):
    """L0 D L0^T, L0 unit lower triangular (strict part U(-1, 1) / sqrt(n)), D ~ U(1, 2) except D[p] = -1: the leading p x p block
    is positive definite with pivots >= 1, pivot p is -1 (0-based; a Cholesky reports p + 1)"""
    rng = np.random.default_rng(seed)
    L0 = np.tril(rng.uniform(-1.0, 1.0, (n, n)) / np.sqrt(n), -1) + np.eye(n)
    d = rng.uniform(1.0, 2.0, n)
    d[p] = -1.0
    return _sym((L0 * d[None, :]) @ L0.T), rng.normal(size=n)


def factor_bound(n, dtype=LD):
    return n + 8 if dtype is LD else 2 * n + 10


def solve_bound(n):
    return 3 * n + 1


def _ratio_max(num, den):
    """max num / den over the entries; an entry with den == 0 must have num == 0 (every product that forms it is zero)"""
    if np.any((den == 0) & (num != 0)) or not np.all(np.isfinite(num)):
        return np.inf
    ok = den > 0
    return float((num[ok] / den[ok]).max()) if ok.any() else 0.0


def factor_excess(A, L, dtype=LD, where=False):
    """max_ij |A - L L^T|_ij / (|L| |L^T|)_ij / u; with where=True also the (i, j) of the maximum"""
    Lx, Ax = np.tril(L).astype(dtype), np.asarray(A).astype(dtype)
    num = np.abs(Ax - Lx @ Lx.T)
    den = np.abs(Lx) @ np.abs(Lx).T
    ex = _ratio_max(num, den) / U
    if not where:
        return ex
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(den > 0, num / den, np.where(num != 0, np.inf, 0.0))
    return ex, tuple(int(v) for v in np.unravel_index(np.argmax(q), q.shape))


def solve_excess(A, Lref, x, b, dtype=LD):
    """max_i |b - A x|_i / (|Lref| |Lref^T| |x|)_i / u"""
    Ax, xx, bx, Lx = np.asarray(A).astype(dtype), np.asarray(x).astype(dtype), np.asarray(b).astype(dtype), np.abs(Lref).astype(dtype)
    num = np.abs(bx - Ax @ xx)
    den = Lx @ (Lx.T @ np.abs(xx))
    return _ratio_max(num, den) / U


def diag_block_cond1(Lref, nb=64):
    """max over the nb x nb diagonal blocks of Lref of cond_1(block): what a back-substitution through explicit inverses of
    those blocks (k_chol_backsolve) pays over a substitution"""
    n = Lref.shape[0]
    return max(float(np.linalg.cond(Lref[k:k + nb, k:k + nb], 1)) for k in range(0, n, nb))


def cholesky_ld(A):
    """unblocked Cholesky in long double: (L, info, pivots) with info = 0 or 1 + the first non-positive pivot (L, pivots up to there)"""
    Ax = np.asarray(A).astype(LD)
    n = Ax.shape[0]
    L = np.zeros((n, n), LD)
    piv = np.zeros(n, LD)
    for j in range(n):
        piv[j] = Ax[j, j] - L[j, :j] @ L[j, :j]
        if not piv[j] > 0:
            return L, j + 1, piv[:j + 1]
        L[j, j] = np.sqrt(piv[j])
        L[j + 1:, j] = (Ax[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L, 0, piv


def _fma(a, b, c):
    """fma in double out of a long double product: the product of two doubles is not exact in 64 bits, but its error (2^-64 relative)
    is 2^-11 u -- invisible at the scale the tests look at"""
    return np.asarray(LD(a) * LD(b) + LD(c)).astype(np.float64)


def _rsqrt(x):
    return np.float64(1.0) / np.sqrt(np.float64(x))


def pairwise_cholesky_emulation(A, diagonal):
    """Unblocked float64 right-looking Cholesky that takes its pivots in pairs with factor_panel's formulas (pxr_chol_core.h):
        inv0 = rsqrt(d00),  inv1 = rsqrt(d00 d11 - d10^2) (d00 inv0),  l0 = a0 inv0,  l1 = (a1 - l0 l10) inv1.
    diagonal = "product":    L[j+1][j+1] = (d11 - l10^2) inv1, what falls out of scaling the column (the kernel before the fix)
    diagonal = "reciprocal": L[j][j] = 1 / inv0, L[j+1][j+1] = 1 / inv1, consistent with the inv that scaled the column"""
    W = np.array(A, dtype=np.float64)
    n = W.shape[0]
    L = np.zeros((n, n))
    for j in range(0, n, 2):
        d00 = W[j, j]
        inv0 = _rsqrt(d00)
        l0 = W[j:, j] * inv0
        L[j:, j] = l0
        if j + 1 < n:
            d10, d11 = W[j + 1, j], W[j + 1, j + 1]
            det = _fma(d00, d11, -(d10 * d10))
            inv1 = _rsqrt(det) * (d00 * inv0)
            l10 = d10 * inv0
            l1 = _fma(-l0[1:], l10, W[j + 1:, j + 1]) * inv1
            L[j + 1:, j + 1] = l1
            W[j + 2:, j + 2:] = _fma(-l1[1:, None], l1[None, 1:], _fma(-l0[2:, None], l0[None, 2:], W[j + 2:, j + 2:]))
            if diagonal == "reciprocal":
                L[j + 1, j + 1] = 1.0 / inv1
        if diagonal == "reciprocal":
            L[j, j] = 1.0 / inv0
    return L
