"""Input families and references for the window solver on given systems (tsba_debug_solve_given; tests/test_gpu_solve_given.py).  numpy only.

The systems are S dp = -g with S symmetric of 6 nb rows (nb pose blocks); only S's lower triangle is meaningful to the solver.

exact(nb, seed)           S = L D L^T, L unit lower with integer entries in [-2, 2] no further than BAND = 12 columns from the diagonal, D from
                          {0.5, 1, 2, 4}, g = -S x for an integer x.  An unpivoted LDL^T of S meets only small dyadic numbers: the pivots are D's entries
                          (their reciprocals powers of two), the multipliers L's integers, every Schur-complement entry a partial sum of at most 13 products
                          l d l' (multiples of 1/2 below 2^8), both substitutions and the 6x6 inverse factors integers or halves far below 2^53.  No operation
                          rounds, so the result does not depend on the order of the sums or on fused multiply-adds: dp == x in every bit.  One thing does
                          depend on the order: the sign of a zero.  The solver computes y = -x out of cancelling sums and stores dp = -y; a component x = 0
                          would come out as +0 or -0 depending on which partial sums cancel.  x is therefore drawn from the NON-ZERO integers of [-8, 8].
exact(..., bad=(b, r, v)) the same with D[6 b + r] = v for v = -1, 0.0 or NaN.  The pivots before it are D's positive entries whatever the order of the
                          operations, so the first pivot that is not positive is exactly v, at row r of block b.  (S is summed over L's structural
                          non-zeros only: 0 x NaN must not reach the rows before the bad pivot.)
conditioned(nb, kappa)    S = Q diag(logspace(0, -log10 kappa, n)) Q^T, symmetrised, Q the QR factor of a seeded normal matrix, g seeded normal.

reference(S, g)           unpivoted LDL^T in np.longdouble with two steps of iterative refinement on residuals taken in np.longdouble.
yardstick(S, g)           the same LDL^T in float64, no refinement: the error a plain double-precision solver of this kind makes."""
import numpy as np

BAND = 12
D_VALUES = np.array([0.5, 1.0, 2.0, 4.0])
KAPPAS = (1e2, 1e6, 1e10)


def exact(nb, seed=0, bad=None):
    """-> S [n, n] (symmetric, both triangles), g [n], x [n]: S x = -g exactly; bad = (block, row, value) plants one pivot (x is then not a solution)."""
    n = 6*nb
    rng = np.random.default_rng([nb, seed, 20240607])
    L = np.tril(rng.integers(-2, 3, (n, n)).astype(np.float64), -1)
    i, j = np.indices((n, n))
    L[i - j > BAND] = 0.0
    L[np.arange(n), np.arange(n)] = 1.0
    D = D_VALUES[rng.integers(0, 4, n)]
    x = rng.integers(1, 9, n)*rng.choice([-1, 1], n).astype(np.float64)
    D0 = D.copy()
    if bad is not None:
        D0[6*bad[0] + bad[1]] = 0.0
    S = (L*D0) @ L.T
    g = -(S @ x)
    if bad is not None:                                  # the planted pivot's term, on the support of its column of L only
        k = 6*bad[0] + bad[1]
        sup = np.nonzero(L[:, k])[0]
        col = L[sup, k]
        S[np.ix_(sup, sup)] += bad[2]*np.outer(col, col)
        g[sup] -= bad[2]*col*float(col @ x[sup])
    return S, g, x


def conditioned(nb, kappa, seed=0):
    n = 6*nb
    rng = np.random.default_rng([nb, seed, int(round(np.log10(kappa))), 977])
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    S = (Q*np.logspace(0.0, -np.log10(kappa), n)) @ Q.T
    return 0.5*(S + S.T), rng.standard_normal(n)


def ldlt(S, dtype=np.float64):
    """Unpivoted right-looking LDL^T of S's lower triangle in `dtype` -> (L unit lower, d, index of the first pivot that is not > 0 or -1).
    The factorisation stops at such a pivot (L, d are then partial)."""
    A = np.tril(np.asarray(S)).astype(dtype)
    n = A.shape[0]
    d = np.zeros(n, dtype)
    for k in range(n):
        dk = A[k, k]
        if not dk > 0:
            return A, d, k
        d[k] = dk
        c = A[k + 1:, k].copy()
        l = c/dk
        A[k + 1:, k + 1:] -= np.tril(np.outer(l, c))
        A[k + 1:, k] = l
        A[k, k] = 1
    return A, d, -1


def _substitute(L, d, b):
    x = np.array(b, dtype=L.dtype)
    n = x.shape[0]
    for k in range(n):                                    # L z = b
        x[k + 1:] -= L[k + 1:, k]*x[k]
    x /= d
    for k in range(n - 1, -1, -1):                        # L^T x = z
        x[:k] -= L[k, :k]*x[k]
    return x


def _full(S, dtype):
    T = np.tril(np.asarray(S)).astype(dtype)
    return T + np.tril(T, -1).T


def yardstick(S, g):
    """float64 LDL^T, no refinement -> dp with S dp = -g (None where a pivot is not positive)."""
    L, d, badk = ldlt(S, np.float64)
    return None if badk >= 0 else _substitute(L, d, -np.asarray(g, np.float64))


def reference(S, g, steps=2):
    """np.longdouble LDL^T + `steps` of refinement -> (dp as np.longdouble, residual S dp + g in np.longdouble)."""
    ld = np.longdouble
    L, d, badk = ldlt(S, ld)
    assert badk < 0, badk
    A, b = _full(S, ld), -np.asarray(g).astype(ld)
    x = _substitute(L, d, b)
    for _ in range(steps):
        x = x + _substitute(L, d, b - A @ x)
    return x, A @ x - b


def backward_error(S, dp, g):
    """|| S dp + g ||_inf / (|| S ||_inf || dp ||_inf + || g ||_inf), the residual in np.longdouble."""
    ld = np.longdouble
    A, x, b = _full(S, ld), np.asarray(dp).astype(ld), np.asarray(g).astype(ld)
    r = np.abs(A @ x + b).max()
    return float(r/(np.abs(A).sum(axis=1).max()*np.abs(x).max() + np.abs(b).max()))


def forward_error(dp, ref):
    """|| dp - ref ||_inf / || ref ||_inf in np.longdouble."""
    ld = np.longdouble
    return float(np.abs(np.asarray(dp).astype(ld) - ref).max()/np.abs(ref).max())
