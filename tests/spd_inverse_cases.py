"""Error measure and bound for the dense SPD inverse (csrc/pxr_spd_inverse.hip), pure numpy, in the style of chol_cases.py.

Measure: inverse_excess(A, X) = max_ij |X A - I|_ij / (|X| |L| |L^T|)_ij / u  and its mirror |A X - I| / (|L| |L^T| |X|),
         L the long double Cholesky factor of A, the products evaluated in long double.

Bound, from the rounding analysis of the algorithm the kernels run (first order in u; gamma_k = k u):
  1. A + dA = L L^T,  |dA| <= (n + 8) u |L| |L^T|                                   (chol_cases.factor_bound)
  2. M_j, the inverse of the 64 x 64 diagonal tile L_jj, comes out of the factorisation's sweep as identity rows carried through
     a substitution (pxr_chol_core.h): every row of M_j^T is the exact solution of a system perturbed by gamma_65 |L_jj|, so
     |L_jj M_j - I| <= 65 u |L_jj| |M_j|   and, on the other side,   |M_j L_jj - I| <= 65 u |M_j| K_j |L_jj|,  K_j = |L_jj| |M_j|.
  3. T = inv(L) by block columns: T_jj = M_j,  T_ij = -G M_j with G = sum_{j < k <= i} T_ik L_kj (inner products of at most n
     terms, any order: |dG| <= n u (|T| |L|)_ij), the product with M_j another 64 terms (|d2| <= 64 u |G| |M_j|), and
     |G| = |T_ij L_jj| <= |T_ij| |L_jj|.  Block (i, j) of R = T L - I is  -dG - G (M_j L_jj - I) + d2 L_jj, hence
         |R| <= u |T| C |L|,   C = n I + blockdiag(64 K_j + 65 K_j^2).
     The explicit inverses of the diagonal tiles make this stable only conditionally (Higham, Accuracy and Stability, 14.1 --
     and the back-substitution of the solve, tests/test_chol_gpu.py): K_j is where the tiles' condition enters.
  4. X = fl(T^T T) = T^T T + E,  |E| <= n u |T^T| |T|  (inner products of at most n terms).
  With these,  X A - I = (L T - I)^T + T^T R L^T + E A - X dA,  and the residual on the other side is L T - I = L R T to first
  order (L (T L - I) T = (L T)^2 - L T), so
      |X A - I| <= u B,   B = (n + 8) |X| |L| |L^T| + n |T^T| |T| |L| |L^T| + (|L| |T| C |L| |T|)^T + |T^T| |T| C |L| |L^T| .
  Every term scales with a diagonal scaling of A as the denominator does (K_j -> D K_j D^-1): the bound is as blind to the grading
  of the `graded` family as the measure is.
  inverse_bound(A) = max_ij B_ij / (|X| |L| |L^T|)_ij with L, T, X, M_j of the REFERENCE (long double): nothing in it comes from
  the code under test.  (X is symmetric bit for bit and so is A: the mirror measure is the transpose of the first.)
"""
import numpy as np

import chol_cases as cc

NB = 64
LD = cc.LD


def reference(A):
    """(L, T, X) of A in long double: Cholesky factor, its inverse by substitution, T^T T"""
    L, info, _ = cc.cholesky_ld(A)
    assert info == 0
    n = L.shape[0]
    T = np.zeros((n, n), LD)
    for j in range(n):                      # column j of inv(L) by forward substitution
        T[j, j] = LD(1) / L[j, j]
        for i in range(j + 1, n):
            T[i, j] = -(L[i, j:i] @ T[j:i, j]) / L[i, i]
    return L, T, T.T @ T


def inverse_bound(L, T, X):
    n = L.shape[0]
    aL, aT, aX = np.abs(L), np.abs(T), np.abs(X)
    C = np.eye(n, dtype=LD) * n
    for k in range(0, n, NB):
        K = aL[k:k + NB, k:k + NB] @ aT[k:k + NB, k:k + NB]          # (the diagonal blocks of inv(L) are the blocks' inverses)
        C[k:k + NB, k:k + NB] += 64 * K + 65 * (K @ K)
    LLt = aL @ aL.T
    TtT = aT.T @ aT
    den = aX @ LLt
    B = (n + 8) * den + n * (TtT @ LLt) + (aL @ aT @ C @ aL @ aT).T + TtT @ C @ LLt
    return float((B / den).max())


def inverse_excess(A, L, X):
    """(max |X A - I| / (|X| |L| |L^T|), max |A X - I| / (|L| |L^T| |X|)) in units of u"""
    Ax, Xx = np.asarray(A).astype(LD), np.asarray(X).astype(LD)
    n = Ax.shape[0]
    LLt = np.abs(L) @ np.abs(L).T
    I = np.eye(n, dtype=LD)
    left = cc._ratio_max(np.abs(Xx @ Ax - I), np.abs(Xx) @ LLt) / cc.U
    right = cc._ratio_max(np.abs(Ax @ Xx - I), LLt @ np.abs(Xx)) / cc.U
    return left, right


def blocked_inverse_emulation(A):
    """The kernels' algorithm in float64 numpy (LAPACK's factor in place of the device's): tile inverses by substitution,
    T by block columns through the explicit tile inverses, X = T^T T"""
    n = A.shape[0]
    L = np.linalg.cholesky(A)
    N = (n + NB - 1) // NB
    sl = [slice(k * NB, min(n, (k + 1) * NB)) for k in range(N)]
    T = np.zeros((n, n))
    M = []
    for k in range(N):
        Lk = L[sl[k], sl[k]]
        m = Lk.shape[0]
        Mk = np.zeros((m, m))
        for c in range(m):
            Mk[c, c] = 1.0 / Lk[c, c]
            for r in range(c + 1, m):
                Mk[r, c] = -(Lk[r, c:r] @ Mk[c:r, c]) / Lk[r, r]
        M.append(Mk)
        T[sl[k], sl[k]] = Mk
    for j in range(N - 2, -1, -1):
        for i in range(j + 1, N):
            G = np.zeros((sl[i].stop - sl[i].start, NB))
            for k in range(j + 1, i + 1):
                G += T[sl[i], sl[k]] @ L[sl[k], sl[j]]
            T[sl[i], sl[j]] = (-G) @ M[j]
    X = np.tril(T.T @ T)
    return X + np.tril(X, -1).T
