"""textslam_amd/csrc/tsjacobi.h on the CPU: tests/cxx/jacobi_host.hip includes that header ALONE (so it stands on its own), is built with the host sanitizers (address,
undefined) and run as a child process on seeded and special matrices; numpy checks properties of what it returns.  No GPU.

The one-sided iteration returns G = A Q with orthogonal columns and the index of the shortest one; the two-sided rotation is run in the loops of its two callers
(pnp_sym3_eig's on the 3 x 3, horn_sim3's on the 4 x 4) and returns the diagonal form and V.

Tolerances.  ||Q^T Q - I||, ||A Q - G|| (and their two-sided likes) are held to 1e-14 relative to ||A||, the column products of G to the iteration's own stopping
rule, evaluated in the iteration's own order of operations -- so that rule is asserted exactly.  The two comparisons with numpy (singular values against
numpy.linalg.svd, eigenvalues against numpy.linalg.eigvalsh), relative to the largest one, were measured on the same seeded matrices with the functions these
replaced (tv_turn3, rec_turn4, pnp_polar3_turn, pnp_sym3_rotate, jacobi_rotate, compiled into this program once): the largest difference was 1.13e-15 for the
singular values (the 4 x 4; 8.4e-16 on the 3 x 3) and 1.86e-15 for the eigenvalues (the 4 x 4; 1.26e-15 on the 3 x 3); asserted at 10 x that, 1.13e-14 and
1.86e-14, to leave room for a different compiler's association of exact operations.  This header's functions give the same figures."""
import math
import os
import struct
import subprocess
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SV_MEASURED, EV_MEASURED = 1.13e-15, 1.86e-15
SV_TOL, EV_TOL = 10*SV_MEASURED, 10*EV_MEASURED
N_SEEDED = 200
ORTHO, TINY = 1e-14, 1e-17


# ------------------------------------------------------------------ the inputs
def seeded(N, symmetric):
    """200 well-conditioned matrices (condition number at most 100) of a fixed seed, scales from 1e-3 to 1e3."""
    g = np.random.default_rng(1000*N + (7 if symmetric else 0)); out = []
    while len(out) < N_SEEDED:
        A = g.standard_normal((N, N))
        if symmetric:
            A = A + A.T
        if np.linalg.cond(A) <= 100.0:
            out.append(A*10.0**g.uniform(-3, 3))
    return out


def specials(N, symmetric):
    g = np.random.default_rng(77 + N)
    u, v = g.standard_normal(N), g.standard_normal(N)
    d = np.diag([3.0, 1.0, 1.0] if N == 3 else [2.0, 1.0, 1.0, 3.0])                 # two equal smallest: the first of them is column 1
    perm = np.eye(N)[:, ::-1]*np.array([2.0, 1.0, 1.0, 5.0][:N])                      # orthogonal columns that are no diagonal; lengths 2 1 1 (5): again column 1
    nan = (lambda A: (A + A.T) if symmetric else A)(g.standard_normal((N, N)))
    nan[1, 2] = np.nan
    if symmetric:
        nan[2, 1] = np.nan
    out = {"zero": np.zeros((N, N)), "diagonal": d, "rank1": np.outer(u, u) if symmetric else np.outer(u, v), "nan": nan}
    if not symmetric:
        out["orthogonal"] = perm
    return out


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """Builds the program, runs it ONCE on every record of the module, and hands out the answers by key."""
    tmp = tmp_path_factory.mktemp("jacobi_host"); exe = str(tmp / "jacobi_host")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "cxx", "jacobi_host.hip")])
    recs = []                                                          # (key, kind, N, matrix)
    for N in (3, 4):
        for i, A in enumerate(seeded(N, False)):
            recs.append((("one", N, i), 0, N, A))
        for i, A in enumerate(seeded(N, True)):
            recs.append((("sym", N, i), 1, N, A))
        for name, A in specials(N, False).items():
            recs.append((("one", N, name), 0, N, A))
        for name, A in specials(N, True).items():
            recs.append((("sym", N, name), 1, N, A))
    for i, A in enumerate(seeded(3, False)[:50]):
        recs.append((("polar", 3, i), 2, 3, A))
    for i, A in enumerate(seeded(4, False)[:50]):
        recs.append((("null", 4, i), 3, 4, A))
    g = np.random.default_rng(5)
    signs = [g.standard_normal((N, N)) for N in (3, 4) for _ in range(20)]
    signs += [np.array([[1.0, -1.0, 0.5], [-2.0, 2.0, -2.0], [0.0, -0.0, 0.0]]), np.array([[-3.0, 3.0, 1.0], [1.0, 2.0, -2.0], [np.nan, -1.0, 0.5]])]    # ties, zeros, a NaN
    for i, A in enumerate(signs):
        recs.append((("sign", A.shape[0], i), 4, A.shape[0], A))
    inp, outp = str(tmp / "in.bin"), str(tmp / "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<i", len(recs)))
        for _, kind, N, A in recs:
            f.write(struct.pack("<ii", kind, N)); f.write(np.ascontiguousarray(A, np.float64).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")             # (the HIP runtime's own start-up allocations are not this program's)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "jacobi host: ok" in r.stdout, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    raw = open(outp, "rb").read(); off = 0; out = {}

    def take(dt, k):
        nonlocal off
        a = np.frombuffer(raw, dt, k, off); off += a.nbytes
        return a
    for key, kind, N, A in recs:
        if kind in (0, 1, 2):
            out[key] = (A, take(np.float64, N*N).reshape(N, N), take(np.float64, N*N).reshape(N, N), int(take(np.int32, 1)[0]))
        elif kind == 3:
            out[key] = (A, take(np.float64, 4))
        else:
            out[key] = (A, take(np.int32, N), take(np.int32, 3) if N == 3 else None)
    out["pairs9"] = take(np.int32, 9*5*2).reshape(9, 5, 2); out["pairs11"] = take(np.int32, 11*6*2).reshape(11, 6, 2)
    assert off == len(raw)
    return out


# ------------------------------------------------------------------ the iteration's own arithmetic, in its order
def col_products(G, p, q):
    al = be = ga = 0.0
    for i in range(G.shape[0]):
        al += G[i, p]*G[i, p]; be += G[i, q]*G[i, q]; ga += G[i, p]*G[i, q]
    return float(al), float(be), float(ga)


def would_turn(G, p, q, ortho=ORTHO, tiny=TINY):
    al, be, ga = col_products(G, p, q)
    return abs(ga) > ortho*math.sqrt(al*be) and abs(ga) > tiny*(al + be)          # (a NaN compares false)


def length2(G, j):
    s = G[0, j]*G[0, j] + G[1, j]*G[1, j]
    for i in range(2, G.shape[0]):
        s = s + G[i, j]*G[i, j]
    return float(s)


def first_shortest(G):
    return int(np.argmin([length2(G, j) for j in range(G.shape[0])]))              # argmin: the first of equal ones


def pairs(N):
    return [(p, q) for p in range(N) for q in range(p + 1, N)]


def fro(M):
    return float(np.linalg.norm(M))


def check_one_sided(A, G, Q, jmin, ortho=ORTHO, tiny=TINY):
    N = A.shape[0]
    assert fro(Q.T @ Q - np.eye(N)) <= 1e-14
    assert fro(A @ Q - G) <= 1e-14*fro(A)
    assert not any(would_turn(G, p, q, ortho, tiny) for p, q in pairs(N))          # converged inside the sweep bound: the stopping rule holds, exactly
    assert jmin == first_shortest(G)


# ------------------------------------------------------------------ one-sided
@pytest.mark.parametrize("N", [3, 4])
def test_one_sided_on_seeded_matrices(run, N):
    worst = 0.0
    for i in range(N_SEEDED):
        A, G, Q, jmin = run[("one", N, i)]
        check_one_sided(A, G, Q, jmin)
        for p, q in pairs(N):                                                       # well-conditioned: the first test of the rule alone
            al, be, ga = col_products(G, p, q)
            assert abs(ga) <= ORTHO*math.sqrt(al*be)
        sv = np.linalg.svd(A, compute_uv=False)
        d = float(np.abs(np.sort(np.sqrt([length2(G, j) for j in range(N)]))[::-1] - sv).max()/sv[0]); worst = max(worst, d)
        assert np.sqrt(length2(G, jmin)) <= sv[-1]*(1 + 1e-12)
    print("N = %d: largest relative difference of a singular value from numpy.linalg.svd: %.2e (tolerance %.2e)" % (N, worst, SV_TOL))
    assert worst <= SV_TOL


@pytest.mark.parametrize("N", [3, 4])
def test_one_sided_special_matrices(run, N):
    I = np.eye(N)
    A, G, Q, jmin = run[("one", N, "zero")]
    assert not G.any() and Q.tobytes() == I.tobytes() and jmin == 0
    for name in ("diagonal", "orthogonal"):                                         # nothing to turn: zero turns, G and Q as they were, bit for bit; of the two
        A, G, Q, jmin = run[("one", N, name)]                                       # equal shortest columns the first
        assert G.tobytes() == A.tobytes() and Q.tobytes() == I.tobytes() and jmin == 1
    A, G, Q, jmin = run[("one", N, "rank1")]
    check_one_sided(A, G, Q, jmin)
    sv = np.sort(np.sqrt([length2(G, j) for j in range(N)]))[::-1]
    assert abs(sv[0] - fro(A)) <= SV_TOL*fro(A) and (sv[1:] <= 1e-14*fro(A)).all()
    # one NaN entry, at (1, 2): column 2 never turns -- it and its column and row of Q are as they were -- and the other columns are turned among themselves
    A, G, Q, jmin = run[("one", N, "nan")]
    rest = [j for j in range(N) if j != 2]
    assert G[:, 2].tobytes() == A[:, 2].tobytes() and Q[:, 2].tobytes() == I[:, 2].tobytes() and Q[2, :].tobytes() == I[2, :].tobytes()
    assert np.isfinite(G[:, rest]).all() and np.isfinite(Q).all()
    Qr = Q[np.ix_(rest, rest)]
    assert fro(Qr.T @ Qr - np.eye(N - 1)) <= 1e-14 and fro(A[:, rest] @ Qr - G[:, rest]) <= 1e-14*fro(A[:, rest])
    assert not any(would_turn(G, p, q) for p, q in pairs(N))


def test_polar_thresholds_and_no_second_test(run):
    """pnp_polar3's thresholds: 1e-17 relative and tiny = 0.0 (no second test).  1e-17 is below a double's rounding, so this iteration turns on rounding noise until
    a sweep happens to turn nothing or the bound ends it: its own rule is not asserted, the callers' rule (1e-14) and the two norms are."""
    for i in range(50):
        A, G, Q, jmin = run[("polar", 3, i)]
        assert fro(Q.T @ Q - np.eye(3)) <= 1e-14 and fro(A @ Q - G) <= 1e-14*fro(A) and jmin == first_shortest(G)
        for p, q in pairs(3):
            al, be, ga = col_products(G, p, q)
            assert abs(ga) <= ORTHO*math.sqrt(al*be)


def test_null_vector_of_a_4x4(run):
    for i in range(50):
        A, v = run[("null", 4, i)]
        _, G, Q, jmin = run[("one", 4, i)]
        assert v.tobytes() == np.ascontiguousarray(Q[:, jmin]).tobytes()            # the same iteration, the column under the shortest one
        sv = np.linalg.svd(A, compute_uv=False)
        assert abs(fro(A @ v) - sv[-1]) <= 1e-14*fro(A) + SV_TOL*sv[0] and abs(fro(v) - 1.0) <= 1e-14      # | |A v| - |g| | <= |A Q - G|, and |g| is the singular value


# ------------------------------------------------------------------ two-sided
@pytest.mark.parametrize("N", [3, 4])
def test_two_sided_on_seeded_matrices(run, N):
    worst = 0.0; most = 0
    for i in range(N_SEEDED):
        A, D, V, sweeps = run[("sym", N, i)]
        assert sweeps < (40 if N == 3 else 24); most = max(most, sweeps)            # it left because nothing was left to rotate
        assert not (D - np.diag(np.diag(D))).any()                                  # ... every off-diagonal entry exactly zero
        assert fro(V.T @ V - np.eye(N)) <= 1e-14
        assert fro(A @ V - V @ D) <= 1e-14*fro(A)
        ev = np.linalg.eigvalsh(A)
        worst = max(worst, float(np.abs(np.sort(np.diag(D)) - ev).max()/np.abs(ev).max()))
    print("N = %d: largest relative difference of an eigenvalue from numpy.linalg.eigvalsh: %.2e (tolerance %.2e); most sweeps %d" % (N, worst, EV_TOL, most))
    assert worst <= EV_TOL


@pytest.mark.parametrize("N", [3, 4])
def test_two_sided_special_matrices(run, N):
    I = np.eye(N)
    for name in ("zero", "diagonal"):                                               # nothing to rotate: A bit-unchanged, no sweep
        A, D, V, sweeps = run[("sym", N, name)]
        assert D.tobytes() == A.tobytes() and V.tobytes() == I.tobytes() and sweeps == 0
    A, D, V, sweeps = run[("sym", N, "rank1")]
    assert not (D - np.diag(np.diag(D))).any() and fro(V.T @ V - I) <= 1e-14 and fro(A @ V - V @ D) <= 1e-14*fro(A)
    ev = np.sort(np.abs(np.diag(D)))[::-1]
    assert abs(ev[0] - fro(A)) <= EV_TOL*fro(A) and (ev[1:] <= 1e-14*fro(A)).all()
    A, D, V, sweeps = run[("sym", N, "nan")]                                        # a NaN: nothing to gain, nothing touched
    assert D.tobytes() == A.tobytes() and V.tobytes() == I.tobytes() and sweeps == 0


# ------------------------------------------------------------------ the sign rule and the round-robin order
def test_sign_rule(run):
    for key, val in run.items():
        if isinstance(key, tuple) and key[0] == "sign":
            A, neg, neg3 = val
            for i, row in enumerate(A):
                k = 0
                for j in range(1, len(row)):
                    if abs(row[j]) > abs(row[k]):                                   # strictly greater: the first on ties; a NaN is never greater
                        k = j
                assert neg[i] == int(row[k] < 0)
            if neg3 is not None:
                assert np.array_equal(neg, neg3)                                    # three scalars: the same rule


@pytest.mark.parametrize("M", [9, 11])
def test_round_robin_order(run, M):
    P = run["pairs%d" % M]; n = M if M == 9 else M + 1                               # M = 9: nine indices and a bye; M = 11: twelve indices
    seen = set()
    for r in range(M):
        step = [tuple(int(x) for x in P[r, i]) for i in range(P.shape[1])]
        assert all(0 <= p < q <= M for p, q in step)
        assert step[0] == (r, M)                                                    # pair 0: step r's index with index M (the bye, or the index that stays)
        real = step[1:] if M == 9 else step
        assert all(q < n for _, q in real)
        used = [x for pq in real for x in pq]
        assert len(set(used)) == len(used)                                          # the pairs of a step are disjoint
        assert not seen & set(real); seen |= set(real)
    assert seen == {(p, q) for p in range(n) for q in range(p + 1, n)}              # every pair exactly once per sweep
