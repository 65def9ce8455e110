"""The numpy restatement of orbm_llt_solve_dev (include/orbslam_hip.h) in the contract's order, the inputs of its tests
and the backward-error bound (test infrastructure: never part of the product).

The contract is per ENTRY: L[i][j] = (a[i][j] - dot) / L[j][j] with dot = L[i][0] L[j][0] and then dot = dot + L[i][k] L[j][k] in
ascending k.  A right-looking sweep over k that updates every trailing entry at once keeps exactly that order per entry, and is
fast enough in numpy up to n of about 800: the products and the sums are separate numpy operations (no fused multiply-add), the
first product INITIALISES the dot (no 0.0 + product, which would lose the sign of a zero)."""
import functools

import numpy as np

U = 2.0 ** -53


def llt_solve(A, b):
    """(L, x, ok) of the lower triangle of A (the upper one is never read).  ok = 0 at a pivot that is not > 0: x = 0."""
    A = np.asarray(A, np.float64); b = np.asarray(b, np.float64)
    n = len(b)
    L = np.zeros((n, n))
    dot = np.zeros((n, n))
    for j in range(n):
        s = A[j:, j] if j == 0 else A[j:, j] - dot[j:, j]
        if not s[0] > 0.0:
            return L, np.zeros(n), 0
        piv = np.sqrt(s[0])
        L[j, j] = piv
        L[j + 1:, j] = s[1:] / piv
        c = L[j + 1:, j]
        outer = c[:, None] * c[None, :]
        if j == 0:
            dot[1:, 1:] = outer
        else:
            dot[j + 1:, j + 1:] = dot[j + 1:, j + 1:] + outer
    y = b.copy()
    for j in range(n):
        y[j] = y[j] / L[j, j]
        y[j + 1:] = y[j + 1:] - L[j + 1:, j] * y[j]
    for j in range(n - 1, -1, -1):
        y[j] = y[j] / L[j, j]
        y[:j] = y[:j] - L[j, :j] * y[j]
    return L, y, 1


def llt_solve_scalar(A, b):
    """The contract as a literal triple loop over Python floats (IEEE doubles): small n only."""
    n = len(b)
    a = [[float(A[i][j]) for j in range(n)] for i in range(n)]
    L = [[0.0] * n for _ in range(n)]
    for j in range(n):
        for i in range(j, n):
            s = a[i][j]
            if j > 0:
                dot = L[i][0] * L[j][0]
                for k in range(1, j):
                    dot = dot + L[i][k] * L[j][k]
                s = s - dot
            if i == j:
                if not s > 0.0:
                    return np.array(L), np.zeros(n), 0
                L[j][j] = float(np.sqrt(s))
            else:
                L[i][j] = s / L[j][j]
    y = [float(v) for v in b]
    for i in range(n):
        for j in range(i):
            y[i] -= L[i][j] * y[j]
        y[i] = y[i] / L[i][i]
    for i in range(n - 1, -1, -1):
        for j in range(n - 1, i, -1):
            y[i] -= L[j][i] * y[j]
        y[i] = y[i] / L[i][i]
    return np.array(L), np.array(y), 1


def sizes(T):
    """the tile-relative sizes every exact test runs"""
    return sorted({1, 5, 6, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T + 5, 390, 780})


def spd(n, seed=0):
    """B B^T + n I from a seeded B, and a right-hand side"""
    rng = np.random.default_rng(1000 + 7 * n + seed)
    B = rng.standard_normal((n, n))
    return B @ B.T + n * np.eye(n), rng.standard_normal(n)


def block_sparse(n, seed=0, band=3):
    """A reduced camera system's pattern: 6 x 6 blocks, a sum of J^T J over 'points' that each see up to band + 1 neighbouring
    keyframes, plus I -- blocks further than `band` apart are EXACT zeros, and so is L there (no fill outside the band).  The
    leading n x n part of it (n need not be a multiple of 6)."""
    rng = np.random.default_rng(5000 + 11 * n + seed)
    nb = (n + 5) // 6
    S = np.eye(6 * nb)
    for _ in range(4 * nb):
        k0 = int(rng.integers(0, nb))
        ks = np.arange(k0, min(k0 + int(rng.integers(1, band + 2)), nb))
        idx = (6 * ks[:, None] + np.arange(6)[None, :]).reshape(-1)
        J = rng.standard_normal((3, len(idx)))
        S[np.ix_(idx, idx)] += J.T @ J
    S = 0.5 * (S + S.T)
    return S[:n, :n].copy(), rng.standard_normal(n)


@functools.lru_cache(maxsize=None)
def case(kind, n):
    """(A, b, L, x, ok), computed once per process; the arrays are shared: do not write to them"""
    A, b = spd(n) if kind == "spd" else block_sparse(n)
    L, x, ok = llt_solve(A, b)
    for a in (A, b, L, x):
        a.setflags(write=False)
    return A, b, L, x, ok


def gamma(k):
    return k * U / (1 - k * U)


def backward_errors(A, b, L, x):
    """normwise relative backward errors of the factorisation and of the solve, and their bound n gamma_(3n+1) (Higham, Accuracy and
    Stability, Thm 10.4 with || |L^T| |L| || <= n ||A||).  Matrices in the Frobenius norm, vectors in the 2-norm: a consistent pair,
    and the theorem's componentwise bound gives || |L| |L^T| ||_F <= ||L||_F^2 = trace(A) <= sqrt(n) ||A||_F, inside the same bound."""
    A = np.tril(A) + np.tril(A, -1).T
    L = np.tril(L)
    n = len(b)
    fact = np.linalg.norm(L @ L.T - A) / np.linalg.norm(A)
    solve = np.linalg.norm(A @ x - b) / (np.linalg.norm(A) * np.linalg.norm(x) + np.linalg.norm(b))
    return float(fact), float(solve), n * gamma(3 * n + 1)
