"""GPU: the dense SPD inverse (pxr_dense_spd_inverse) against the error bound derived in tests/spd_inverse_cases.py."""
import functools

import numpy as np
import pytest

import chol_cases as cc
import spd_inverse_cases as sic

pytestmark = pytest.mark.gpu

FAMILIES = [("random_spd", None), ("graded", None), ("illcond", 8), ("correlated_pairs", 1e-3), ("correlated_pairs", 1e-5)]
SIZES = [1, 2, 63, 64, 65, 130, 257]      # one tile, a partial tile, a tile and one row, three and five block columns


def gpu_inverse(ctx, A, fill_lower=np.nan):
    """pxr_dense_spd_inverse on the upper triangle of A (the strictly lower part filled with `fill_lower`): (info, X)"""
    from pixsfm_amd.engine import dense_spd_inverse
    n = A.shape[0]
    return dense_spd_inverse(ctx, np.triu(A) + np.tril(np.full((n, n), fill_lower), -1))


@functools.lru_cache(maxsize=None)
def reference(family, n, arg=None):
    """(A, L, bound) of a system of tests/chol_cases.py: computed once, never written to"""
    gen = getattr(cc, family)
    A, _ = gen(n, n) if arg is None else gen(n, n, arg)
    L, T, X = sic.reference(A)
    A.setflags(write=False)
    L.setflags(write=False)
    return A, L, sic.inverse_bound(L, T, X)


@pytest.mark.parametrize("family,arg", FAMILIES)
@pytest.mark.parametrize("n", SIZES)
def test_inverse_meets_derived_bound(ctx, family, arg, n):
    A, L, bound = reference(family, n, arg)
    info, X = gpu_inverse(ctx, A)
    left, right = sic.inverse_excess(A, L, X)
    print("%s(%s) n = %d: info %d, |XA - I| excess %.3g, |AX - I| excess %.3g (bound %.4g)" % (family, arg, n, info, left, right, bound))
    assert info == 0
    assert np.all(np.isfinite(X))
    assert X.tobytes() == X.T.copy().tobytes(), "not symmetric bit for bit"
    assert left <= bound, (left, bound)
    assert right <= bound, (right, bound)


@pytest.mark.parametrize("n", [65, 257])
def test_two_runs_give_the_same_bits(ctx, n):
    A, _, _ = reference("graded", n)
    first, second = gpu_inverse(ctx, A), gpu_inverse(ctx, A)
    assert first[0] == second[0] == 0
    assert first[1].tobytes() == second[1].tobytes()


def test_first_non_positive_pivot_is_reported(ctx):
    """-1 on the diagonal at index 70 of n = 130 (the leading 70 x 70 block stays positive definite): info == 71, the call returns"""
    A = np.array(reference("random_spd", 130)[0])
    A[70, 70] = -1.0
    info, _ = gpu_inverse(ctx, A)
    assert info == 71
    # ... and leaves nothing behind
    A, L, bound = reference("random_spd", 130)
    info, X = gpu_inverse(ctx, A)
    assert info == 0 and max(sic.inverse_excess(A, L, X)) <= bound


def test_device_array_is_inverted_in_place(ctx):
    from pixsfm_amd.engine import dense_spd_inverse
    A, L, bound = reference("random_spd", 65)
    d = ctx.to_device(np.triu(A))
    info, out = dense_spd_inverse(ctx, d)
    assert info == 0 and out is d
    assert max(sic.inverse_excess(A, L, d.download())) <= bound


def test_size_limit(ctx):
    import ctypes as C

    from pixsfm_amd._lib import PixsfmHipError, check
    info = C.c_int(0)
    d = ctx.empty((1,), np.float64)
    with pytest.raises(PixsfmHipError, match="exceeds"):
        check(ctx.lib.pxr_dense_spd_inverse(ctx.handle, d.ptr, 18001, C.byref(info)), "pxr_dense_spd_inverse")
