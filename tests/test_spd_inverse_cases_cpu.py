"""CPU: the bound of tests/spd_inverse_cases.py against a float64 numpy emulation of the kernels' algorithm, and against LAPACK."""
import numpy as np
import pytest

import chol_cases as cc
import spd_inverse_cases as sic


@pytest.mark.parametrize("family,arg", [("random_spd", None), ("graded", None), ("illcond", 8), ("correlated_pairs", 1e-3)])
@pytest.mark.parametrize("n", [2, 65, 130])
def test_emulation_meets_bound(family, arg, n):
    gen = getattr(cc, family)
    A, _ = gen(n, n) if arg is None else gen(n, n, arg)
    L, T, X = sic.reference(A)
    bound = sic.inverse_bound(L, T, X)
    left, right = sic.inverse_excess(A, L, sic.blocked_inverse_emulation(A))
    print("%s(%s) n = %d: emulation %.3g / %.3g, bound %.4g" % (family, arg, n, left, right, bound))
    assert max(left, right) <= bound
    assert bound >= 2 * n + 8


def test_reference_inverse_is_an_inverse():
    A, _ = cc.graded(70, 3)
    L, T, X = sic.reference(A)
    assert np.abs(T @ L - np.eye(70)).max() < 1e-16
    assert max(sic.inverse_excess(A, L, X)) < 1.0          # long double: far below one unit of u = 2^-53


def test_a_wrong_inverse_misses_the_bound():
    """the measure sees a transposed tile, a dropped term and a one-ulp-per-entry-times-1e4 perturbation"""
    A, _ = cc.random_spd(130, 130)
    L, T, X = sic.reference(A)
    bound = sic.inverse_bound(L, T, X)
    X64 = np.asarray(X, dtype=np.float64)
    bad = X64.copy()
    bad[64:128, 0:64] = bad[64:128, 0:64].T.copy()
    assert max(sic.inverse_excess(A, L, bad)) > 1e6 * bound
    rng = np.random.default_rng(0)
    noisy = X64 * (1.0 + 1e7 * cc.U * rng.standard_normal(X64.shape))
    assert max(sic.inverse_excess(A, L, noisy)) > bound
