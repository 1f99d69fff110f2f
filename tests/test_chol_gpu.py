"""GPU: hand-written blocked Cholesky (pxr_dense_spd_solve) vs numpy.linalg on SPD systems."""
import ctypes as C
import functools

import numpy as np
import pytest

import chol_cases as cc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", [1, 7, 64, 65, 130, 500, 1593])
def test_spd_solve_matches_numpy(ctx, n):
    rng = np.random.default_rng(n)
    M = rng.normal(size=(n, n + 5))
    A = M @ M.T + np.eye(n) * 1e-3 * n
    b = rng.normal(size=n)
    x_ref = np.linalg.solve(A, b)
    dA = ctx.to_device(np.triu(A) + np.tril(np.full((n, n), np.nan), -1))   # lower part must be ignored
    db = ctx.to_device(b)
    info = C.c_int(-1)
    from pixsfm_amd._lib import check
    check(ctx.lib.pxr_dense_spd_solve(ctx.handle, dA.ptr, n, db.ptr, C.byref(info)), "pxr_dense_spd_solve")
    assert info.value == 0
    x = db.download()
    assert np.abs(x - x_ref).max() <= 1e-9 * max(1.0, np.abs(x_ref).max()) * np.linalg.cond(A) ** 0.5
    L = np.tril(dA.download().T)        # row-major upper == column-major lower
    assert np.abs(L @ L.T - A).max() < 1e-10 * np.abs(A).max()


@pytest.mark.parametrize("pivot", [70, 71, 0, 63, 64, 99])      # the panel sweeps column PAIRS: first and second of a pair
def test_not_positive_definite_is_reported(ctx, pivot):
    n = 100
    A = np.eye(n); A[pivot, pivot] = -1.0
    dA, db = ctx.to_device(A), ctx.to_device(np.ones(n))
    info = C.c_int(0)
    ctx.lib.pxr_dense_spd_solve(ctx.handle, dA.ptr, n, db.ptr, C.byref(info))
    assert info.value == pivot + 1


def test_pivot_that_turns_negative_only_after_elimination(ctx):
    """positive diagonal, indefinite matrix: the failing pivot is the SECOND column of a pair (d11 - l10^2 <= 0)"""
    n = 40
    A = np.eye(n); A[6, 7] = A[7, 6] = 2.0
    dA, db = ctx.to_device(np.triu(A)), ctx.to_device(np.ones(n))
    info = C.c_int(0)
    ctx.lib.pxr_dense_spd_solve(ctx.handle, dA.ptr, n, db.ptr, C.byref(info))
    assert info.value == 8


def test_more_panel_workgroups_than_compute_units(ctx):
    """n > 48 * 256: the first block steps have more panel workgroups than the GPU has CUs, so some of them start after
    workgroup 0 has finished its tile -- they must still find the tile's INPUT values (the factor of a diagonal tile goes
    to the workspace, not over the tile).  Checked through the residual of the solve."""
    n = 12352
    rng = np.random.default_rng(5)
    M = rng.normal(size=(n, 64))
    A = M @ M.T + np.diag(rng.uniform(50.0, 100.0, n))
    b = rng.normal(size=n)
    info = C.c_int(-1)
    dA, db = ctx.to_device(np.triu(A)), ctx.to_device(b)
    assert ctx.lib.pxr_dense_spd_solve(ctx.handle, dA.ptr, n, db.ptr, C.byref(info)) == 0 and info.value == 0
    x = db.download()
    assert np.linalg.norm(A @ x - b) <= 1e-10 * np.linalg.norm(b)
    L = np.triu(dA.download()).T                      # the returned factor, diagonal tiles included
    rows = rng.integers(0, n, 40)
    assert np.allclose((L[rows] @ L.T), A[rows], rtol=0, atol=1e-9 * np.abs(A).max())


# ---- factor and solve against derived error bounds (tests/chol_cases.py) ----------------------------------------------------------
def gpu_solve(ctx, A, b, fill_lower=np.nan):
    """pxr_dense_spd_solve on the upper triangle of A (the strictly lower part filled with `fill_lower`): (info, L, x)"""
    n = A.shape[0]
    dA = ctx.to_device(np.triu(A) + np.tril(np.full((n, n), fill_lower), -1))
    db = ctx.to_device(b)
    info = C.c_int(-1)
    try:
        rc = ctx.lib.pxr_dense_spd_solve(ctx.handle, dA.ptr, n, db.ptr, C.byref(info))
        assert rc == 0, "pxr_dense_spd_solve returned %d" % rc
        return info.value, np.tril(dA.download().T), db.download()          # row-major upper == column-major lower
    finally:
        dA.free(); db.free()


@functools.lru_cache(maxsize=None)
def reference(family, n, arg=None):
    """(A, b, Lref) of a system of tests/chol_cases.py, computed once and never written to"""
    gen = getattr(cc, family)
    A, b = gen(n, n) if arg is None else gen(n, n, arg)
    out = (A, b, np.linalg.cholesky(A))
    for v in out:
        v.setflags(write=False)
    return out


def check_bounds(tag, A, b, Lref, info, L, x, dtype=cc.LD, inverse_limited=False):
    """info == 0, factor_excess <= its bound, solve_excess <= 3 n + 1 (twice that when evaluated in double); prints the figures.
    inverse_limited: see test_scaling_and_conditioning"""
    n = A.shape[0]
    fe, where = cc.factor_excess(A, L, dtype, where=True)
    se = cc.solve_excess(A, Lref, x, b, dtype)
    sb = cc.solve_bound(n) * (1 if dtype is cc.LD else 2) * (cc.diag_block_cond1(Lref) if inverse_limited else 1)
    print("%s n = %d: info %d, factor_excess %.3g at %s (bound %d), solve_excess %.3g (bound %.4g)" % (tag, n, info, fe, where, cc.factor_bound(n, dtype), se, sb))
    assert info == 0, (tag, info)
    assert fe <= cc.factor_bound(n, dtype), (tag, fe, where)
    assert se <= sb, (tag, se)


def test_every_size_class(ctx):
    """n = 1 .. 272: every residue of n + 1 modulo 16, 48 and 64 in block steps 0 to 4 -- every rows_valid, one to three live row
    wavefronts in the last panel workgroup, the workgroup that mixes identity rows with real rows, a last block of every width, the
    first update tiles (n >= 128) and a tile row of three tiles (n >= 256)"""
    worst_f = worst_s = 0.0
    for n in range(1, 273):
        A, b = cc.random_spd(n, n)
        info, L, x = gpu_solve(ctx, A, b)
        assert info == 0, n
        fe = cc.factor_excess(A, L, np.float64)
        se = cc.solve_excess(A, np.linalg.cholesky(A), x, b, np.float64)
        worst_f, worst_s = max(worst_f, fe / cc.factor_bound(n, np.float64)), max(worst_s, se / (2 * cc.solve_bound(n)))
        assert fe <= cc.factor_bound(n, np.float64), (n, fe)
        assert se <= 2 * cc.solve_bound(n), (n, se)
    print("largest fraction of the bound over n = 1 .. 272: factor %.3f, solve %.3f" % (worst_f, worst_s))


@pytest.mark.parametrize("n", [1599, 1600, 1601])
def test_twenty_five_tile_rows(ctx, n):
    """25 tile rows, steps with more than 256 workgroups (a second round of update tiles), a last tile one row high (n + 1 = 1601)"""
    A, b, Lref = reference("random_spd", n)
    check_bounds("random_spd", A, b, Lref, *gpu_solve(ctx, A, b), dtype=np.float64)


FAMILIES = [("random_spd", None), ("graded", None), ("illcond", 6), ("illcond", 10), ("illcond", 13), ("correlated_pairs", 1e-3), ("correlated_pairs", 1e-5)]


@pytest.mark.parametrize("family,arg", FAMILIES)
@pytest.mark.parametrize("n", [7, 65, 130, 200])
def test_scaling_and_conditioning(ctx, family, arg, n):
    """The factor meets (n + 8) u |L||L^T| on every family.  The solution meets (3 n + 1) u |L||L^T||x| on random_spd, graded and illcond; on
    correlated_pairs it does NOT, and is held to (3 n + 1) max_k cond_1(Lref_kk) instead: k_chol_backsolve forms
    x_k = inv(L_kk)^T z_k with the explicit inverse of the 64 x 64 diagonal factor, which is stable only conditionally (residual
    <= c n u cond(L_kk); Higham, section 14.1), and T's eps makes cond_1(L_kk) 1e4 .. 8e4 (eps = 1e-3), 1e6 .. 8e6 (1e-5).
    solve_excess measured on an MI355X, next to LAPACK (potrf + potrs) and to a numpy back-substitution through inv(L_kk) of
    LAPACK's factor on the same systems, n = 7 / 65 / 130 / 200:
        eps = 1e-3:  kernel 64 / 591 / 372 / 169          LAPACK 0.76 / 0.24 / 0.27 / 0.16   numpy, inverses 90 / 835 / 390 / 294
        eps = 1e-5:  kernel 3.8e3 / 5.2e4 / 5.2e4 / 4.7e4  LAPACK 0.38 / 0.43 / 0.37 / 0.28   numpy, inverses 6e3 / 7e4 / 4e4 / 2e4
    (3 n + 1 = 22 / 196 / 391 / 601; with a substitution inside the block the numpy figures are <= 0.9.)  graded has
    cond_1(L_kk) ~ 1e12 and illcond up to 1e7, yet both stay below 3 (LAPACK: below 1.4): there the inverse's rows are as badly
    scaled as the factor's and the product loses nothing componentwise."""
    A, b, Lref = reference(family, n, arg)
    check_bounds("%s(%s)" % (family, arg), A, b, Lref, *gpu_solve(ctx, A, b), inverse_limited=family == "correlated_pairs")


INDEFINITE = [(272, p) for p in (0, 1, 7, 8, 9, 62, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 271)] + \
             [(65, 64), (100, 99), (129, 128), (200, 199)]      # the last four: the failure lies in a partial last block


@pytest.mark.parametrize("n,p", INDEFINITE)
def test_first_failing_pivot(ctx, n, p):
    """the first non-positive pivot, produced by the elimination (not present in the input's diagonal for p > 0): inside the first
    tile, by the rank-64 update of the previous step in a panel workgroup, and in tiles that update workgroups wrote before
    (tests/test_chol_cases_cpu.py: a long double Cholesky of the same matrices stops at p with pivot -1, every earlier one >= 1)"""
    A, b = cc.indefinite_at(n, p, 1000 * n + p)
    info, _, _ = gpu_solve(ctx, A, b)
    assert info == p + 1


@pytest.mark.parametrize("i,j,v", [(0, 1, np.nan), (3, 70, np.nan), (70, 130, np.nan), (0, 199, np.nan), (100, 199, np.nan),
                                   (64, 64, np.nan), (3, 70, np.inf), (70, 130, np.inf)])
def test_nan_or_inf_in_the_matrix_is_reported(ctx, i, j, v):
    """entry (i, j), i <= j, of the upper triangle is L's row j: it reaches row j's diagonal first, so pivot j is the first that is
    not a positive number (inf: the diagonal becomes -inf or NaN)"""
    A, b, _ = reference("random_spd", 200)
    A = A.copy()
    A[i, j] = A[j, i] = v
    info, _, _ = gpu_solve(ctx, A, b)
    assert info == j + 1


def test_nan_in_the_right_hand_side_is_not_a_factorisation_failure(ctx):
    A, b, _ = reference("random_spd", 200)
    b = b.copy()
    b[17] = np.nan
    info, L, x = gpu_solve(ctx, A, b)
    assert info == 0
    assert cc.factor_excess(A, L) <= cc.factor_bound(200)
    assert np.isnan(x).any()


def test_no_state_between_calls(ctx):
    A, b, Lref = reference("random_spd", 200)
    Ai, bi = cc.indefinite_at(200, 70, 1)
    assert gpu_solve(ctx, Ai, bi)[0] == 71                              # a failing call ...
    check_bounds("after a failure", A, b, Lref, *gpu_solve(ctx, A, b))  # ... leaves nothing behind (info, flags, workspace)
    A16, b16, L16 = reference("random_spd", 1600)
    check_bounds("n = 1600", A16, b16, L16, *gpu_solve(ctx, A16, b16), dtype=np.float64)
    A5, b5, L5 = reference("random_spd", 5)
    check_bounds("n = 5 after n = 1600", A5, b5, L5, *gpu_solve(ctx, A5, b5))
    first, second = gpu_solve(ctx, A, b), gpu_solve(ctx, A, b)
    assert first[0] == second[0] == 0
    assert first[1].tobytes() == second[1].tobytes() and first[2].tobytes() == second[2].tobytes()      # bit-identical
