"""The checkers of tests/chol_cases.py have teeth: LAPACK passes them on every family, a factor with ONE entry off by a relative 1e-13
fails, and so does an emulation of factor_panel's pivot pair that stores (d11 - l10^2) inv1 on the diagonal (no GPU needed)."""
import numpy as np
import pytest
import scipy.linalg

import chol_cases as cc

SIZES = [7, 65, 130, 200]
FAMILIES = {
    "random_spd": lambda n: cc.random_spd(n, n),
    "graded": lambda n: cc.graded(n, n),
    "illcond6": lambda n: cc.illcond(n, n, 6),
    "illcond10": lambda n: cc.illcond(n, n, 10),
    "illcond13": lambda n: cc.illcond(n, n, 13),
    "correlated1e-3": lambda n: cc.correlated_pairs(n, n, 1e-3),
    "correlated1e-5": lambda n: cc.correlated_pairs(n, n, 1e-5),
}
# the (n, p) of tests/test_chol_gpu.py::test_first_failing_pivot
INDEFINITE = [(272, p) for p in (0, 1, 7, 8, 9, 62, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 271)] + \
             [(65, 64), (100, 99), (129, 128), (200, 199)]


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("n", SIZES)
def test_lapack_passes_both_checkers(family, n):
    A, b = FAMILIES[family](n)
    assert np.array_equal(A, A.T) and A.dtype == np.float64 and b.shape == (n,)
    L = np.linalg.cholesky(A)
    x = scipy.linalg.cho_solve((L, True), b)
    fe, fed, se = cc.factor_excess(A, L), cc.factor_excess(A, L, np.float64), cc.solve_excess(A, L, x, b)
    print("%s n = %d: factor_excess %.2f (double %.2f), solve_excess %.2f" % (family, n, fe, fed, se))
    assert fe <= cc.factor_bound(n)
    assert fed <= cc.factor_bound(n, np.float64)
    assert se <= cc.solve_bound(n)
    # measured with LAPACK: <= 16 and <= 1.4; far below the bounds, so neither bound is near what a correct fp64 solver delivers
    assert fe <= 32 and se <= 4


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_one_entry_off_by_1e_13_fails(family):
    n = 130
    A, _ = FAMILIES[family](n)
    L = np.linalg.cholesky(A)
    rng = np.random.default_rng(3)
    # L_ij (1 + d) moves entry (i, j) of L L^T by d |L_ij| L_jj, against (|L||L^T|)_ij = sum_{k <= j} |L_ik| |L_jk|: the measure moves
    # by share_ij d / u with share_ij = |L_ij| L_jj / (|L||L^T|)_ij, and 1e-13 / u = 900.  In column 0 the share is 1 (one product);
    # elsewhere a share above 2 bound / 900 = 0.31 is enough, and 10 to 40 % of the entries of every family have one.  An entry
    # that carries a smaller share of every product it enters is, by the definition of a componentwise backward error, allowed
    # to be that wrong.
    share = np.tril(np.abs(L) * np.diag(L)[None, :] / (np.abs(L) @ np.abs(L).T), -1)
    assert np.all(share[1:, 0] > 1.0 - 1e-12)
    heavy = np.argwhere(share[:, 1:] >= 2 * cc.factor_bound(n) * cc.U / 1e-13) + [0, 1]
    assert len(heavy) >= 0.05 * n * (n - 1) / 2
    picks = [(int(i), 0) for i in rng.integers(1, n, 4)] + [tuple(int(v) for v in heavy[k]) for k in rng.integers(0, len(heavy), 8)]
    for i, j in picks:
        Lp = L.copy()
        Lp[i, j] *= 1.0 + 1e-13
        assert cc.factor_excess(A, Lp) > cc.factor_bound(n), (family, i, j)
        if j == 0:                                                     # the double-precision variant (bound 2 n + 10 = 270 here)
            assert cc.factor_excess(A, Lp, np.float64) > cc.factor_bound(n, np.float64), (family, i, j)
    # a diagonal entry: (i, i) moves by 2e-13 L_ii^2 of sum_k L_ik^2 -- the first one, and the one past it with the largest share
    dshare = np.diag(L) ** 2 / (L ** 2).sum(axis=1)
    for i in (0, 1 + int(np.argmax(dshare[1:]))):
        Lp = L.copy()
        Lp[i, i] *= 1.0 + 1e-13
        assert 1800 * dshare[i] > 2 * cc.factor_bound(n) and cc.factor_excess(A, Lp) > cc.factor_bound(n), (family, i)


@pytest.mark.parametrize("eps", [1e-3, 1e-5])
@pytest.mark.parametrize("n", SIZES)
def test_pair_pivot_diagonal_must_match_the_reciprocal_that_scaled_its_column(n, eps):
    """(d11 - l10^2) inv1 and 1 / inv1 are the same number in exact arithmetic; in floating point they differ relatively by about
    u / (1 - rho^2), rho the conditional correlation of the pair, and the column below was scaled with inv1."""
    A, _ = cc.correlated_pairs(n, n, eps)
    bad = cc.factor_excess(A, cc.pairwise_cholesky_emulation(A, "product"))
    good, where = cc.factor_excess(A, cc.pairwise_cholesky_emulation(A, "reciprocal"), where=True)
    print("n = %d eps = %g: product diagonal %.3g, reciprocal diagonal %.3g at %s (bound %d)" % (n, eps, bad, good, where, cc.factor_bound(n)))
    assert good <= cc.factor_bound(n)
    assert bad > 10 * cc.factor_bound(n)                               # measured: 1e3 to 2e7 against bounds of 15 to 208


def test_pair_pivot_emulation_is_a_cholesky_on_benign_input():
    A, _ = cc.random_spd(65, 65)
    for diagonal in ("product", "reciprocal"):
        assert cc.factor_excess(A, cc.pairwise_cholesky_emulation(A, diagonal)) <= cc.factor_bound(65)


@pytest.mark.parametrize("n,p", INDEFINITE)
def test_indefinite_at_fails_exactly_at_p(n, p):
    A, _ = cc.indefinite_at(n, p, 1000 * n + p)
    _, info, piv = cc.cholesky_ld(A)
    assert info == p + 1
    # the margins: A is L0 D L0^T rounded to double (relative 1e-16 of entries <= ~4), so every pivot is its D within ~1e-14
    assert piv[:p].min() >= 1.0 - 1e-13 if p else True
    assert abs(float(piv[p]) + 1.0) <= 1e-13


def test_checkers_reject_nan_and_structural_zeros():
    A = np.eye(3)
    L = np.eye(3)
    assert cc.factor_excess(A, L) == 0.0
    L[1, 1] = np.nan
    assert cc.factor_excess(A, L) == np.inf
    A[2, 0] = A[0, 2] = 1e-300                                        # |L||L^T| is exactly 0 there: any residual is infinitely too large
    assert cc.factor_excess(A, np.eye(3)) == np.inf
    assert cc.solve_excess(np.eye(3), np.eye(3), np.array([1.0, np.nan, 0.0]), np.ones(3)) == np.inf
