"""The input families and references of tests/solve_given_ref.py hold what tests/test_gpu_solve_given.py relies on (no GPU)."""
import numpy as np
import pytest

import solve_given_ref as sg


@pytest.mark.parametrize("nb", [1, 3, 31])
def test_exact_family_is_exact_in_float64(nb):
    for seed in range(3):
        S, g, x = sg.exact(nb, seed)
        n = 6*nb
        assert np.array_equal(S, S.T) and np.all(x != 0) and np.all(x == np.rint(x)) and np.abs(x).max() <= 8
        assert np.all(S*2 == np.rint(S*2)) and np.abs(S).max() <= 13*16 and np.all(g*2 == np.rint(g*2)) and np.abs(g).max() < 2**16      # small dyadic numbers
        L, d, badk = sg.ldlt(S)
        assert badk == -1 and np.all(np.isin(d, sg.D_VALUES))
        Lo = np.tril(L, -1)
        assert np.all(Lo == np.rint(Lo)) and np.abs(Lo).max() <= 2                       # the factor IS the construction: integers in [-2, 2] ...
        i, j = np.indices((n, n))
        assert np.all(Lo[i - j > sg.BAND] == 0)                                          # ... no further than 12 columns from the diagonal
        dp = sg.yardstick(S, g)
        assert np.array_equal(dp.view(np.uint64), x.view(np.uint64))                     # every bit
        ref, res = sg.reference(S, g)
        assert np.all(ref == x) and np.all(res == 0)


@pytest.mark.parametrize("nb", [1, 2, 5, 31])
def test_bad_pivot_members_fail_exactly_where_planted(nb):
    for b in sorted({0, min(1, nb - 1), nb//2, max(nb - 2, 0), nb - 1}):
        for r in range(6):
            for v in (-1.0, 0.0, np.nan):
                S, g, x = sg.exact(nb, 1, bad=(b, r, v))
                k = 6*b + r
                assert np.all(np.isfinite(S[:k])) and np.all(np.isfinite(S[:, :k])) and np.all(np.isfinite(g[:k]))      # nothing non-finite before the pivot
                L, d, badk = sg.ldlt(S)
                assert badk == k, (nb, b, r, v, badk)
                assert np.all(np.isin(d[:k], sg.D_VALUES))                               # the pivots before it are the construction's
                A = np.tril(S).copy()                                                    # ... and the pivot met is the planted value itself
                for q in range(k):
                    c = A[q + 1:, q].copy()
                    A[q + 1:, q + 1:] -= np.tril(np.outer(c/A[q, q], c))
                assert (np.isnan(A[k, k]) if v != v else A[k, k] == v), (A[k, k], v)
                assert sg.yardstick(S, g) is None


def test_conditioned_family_has_the_condition_number_it_names():
    for nb in (1, 5, 17):
        for kappa in sg.KAPPAS:
            S, g = sg.conditioned(nb, kappa)
            w = np.linalg.eigvalsh(S)
            assert np.array_equal(S, S.T) and w.min() > 0
            assert abs(np.log10(w.max()/w.min()) - np.log10(kappa)) < 0.01, (nb, kappa, w.max()/w.min())
            S2, g2 = sg.conditioned(nb, kappa)
            assert np.array_equal(S, S2) and np.array_equal(g, g2)                       # seeded


def test_yardstick_backward_error_is_a_tenth_of_the_bound():
    """The bound of test_gpu_solve_given.py, n 2^-53, is the first-order Cholesky bound without its constant; a correct float64 LDL^T stays below 0.1 of it."""
    for nb in (1, 2, 5, 11, 17, 29):
        for kappa in sg.KAPPAS + (1e13,):
            S, g = sg.conditioned(nb, kappa)
            be = sg.backward_error(S, sg.yardstick(S, g), g)
            assert be <= 0.1*6*nb*2.0**-53, (nb, kappa, be/(6*nb*2.0**-53))


@pytest.mark.parametrize("nb", [1, 2, 5, 11])
def test_longdouble_reference_against_mpmath(nb):
    """The long-double reference lies at least 100 times closer to a 200-bit Cholesky solve than the float64 yardstick does."""
    mp = pytest.importorskip("mpmath")
    n = 6*nb
    for kappa in sg.KAPPAS:
        S, g = sg.conditioned(nb, kappa)
        with mp.workprec(200):
            A = mp.matrix(n, n)
            for i in range(n):
                for j in range(n):
                    A[i, j] = mp.mpf(float(S[max(i, j), min(i, j)]))                     # the lower triangle, as the solver reads it
            xe = mp.cholesky_solve(A, mp.matrix([mp.mpf(-float(v)) for v in g]))
            ref, _ = sg.reference(S, g)
            y = sg.yardstick(S, g)

            def to_mp(v):                                                                # a long double exactly: high double + remainder
                hi = float(v)
                return mp.mpf(hi) + mp.mpf(float(v - np.longdouble(hi)))
            nx = max(abs(xe[i]) for i in range(n))
            e_ref = max(abs(to_mp(ref[i]) - xe[i]) for i in range(n))/nx
            e_y = max(abs(mp.mpf(float(y[i])) - xe[i]) for i in range(n))/nx
            assert e_y > 0 and e_ref*100 <= e_y, (nb, kappa, float(e_ref), float(e_y))
