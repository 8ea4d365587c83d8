"""The one-workgroup LDL^T solver of a window (tsba_solve.h: solve_body) on GIVEN systems, through tsba_debug_solve_given: the systems the synthetic
windows produce are all well conditioned and positive definite, so neither a failed factorisation nor the solver's own error under poor conditioning is
ever seen by the window tests.  Inputs and references: tests/solve_given_ref.py (checked without a GPU by tests/test_solve_given_ref.py).

Contexts of 4, 11, 20 and 31 keyframes (31: the largest window the LDS solver takes), every number of free blocks from 1 to the context's keyframes: both
sides of the back-substitution's 10-block register sets, of the 16-row MFMA tiles, of the 58 rows of one round of a panel wave and of the loader waves'
first batches; the rows a load clamps to the system's last differ with the context's size, which is why one context is not enough.

Schedules: production (k_solve_back: the solver workgroup alone, solve_body<false, true>, step and flag published to slots that hold NaN) and
tsba_debug_options.solve_variant 1 - 6.  Variants 5 and 6 publish like production; 3 and 4 run k_solve_t (plain stores); 1 and 2 run k_solve_la -- at
these sizes its LDS need (solve_la_lds_doubles(186) = 154832 bytes) is within the 160 KB of a workgroup, so neither falls back to k_solve_t."""
import functools

import numpy as np
import pytest

from textslam_amd import synth, abi
import solve_given_ref as sg

pytestmark = pytest.mark.gpu

N_KF = (4, 11, 20, 31)
SCHEDULES = (0, 1, 2, 3, 4, 5, 6)                     # solve_variant; 0 = production
POLLING = (0, 5, 6)
ZERO = np.uint64(0)


@pytest.fixture(scope="module")
def gpu():
    from textslam_amd.optimizer import Optimizer
    g = Optimizer(0)
    yield g
    g.close()


def _window(n_kf):
    """Any small window of n_kf keyframes: only its size matters to the hook."""
    P = synth.make_problem(n_kf=n_kf, n_pt=30*n_kf, n_text=0, seed=60 + n_kf, n_levels=1)
    o = abi.options_local(); o.n_passes = 1; o.levels[0] = 0
    return P, o


class _Ctx:
    """The window of n_kf keyframes uploaded under solve_variant `var`, for the length of a with-block."""
    def __init__(self, gpu, n_kf, var):
        self.gpu, self.n_kf, self.var = gpu, n_kf, var

    def __enter__(self):
        P, o = _window(self.n_kf)
        self.gpu.debug_set(**({"solve_variant": self.var} if self.var else {}))
        self.gpu.upload(P, o)
        info = self.gpu.solver_info()
        assert info["lds_solver"] == 1 and info["band_storage"] == 0, info
        return self

    def __exit__(self, *a):
        self.gpu.debug_set()

    def solve(self, S, g, what, assembly_failed=False, failed=0):
        """One call of the hook; the flags are checked here: LmState.step_fail and the published flag agree (-1: the schedule does not poll)."""
        r = self.gpu.solve_given(S, g, assembly_failed)
        assert r["failed"] == failed, (what, r["failed"], r["published"])
        assert r["published"] == (failed if self.var in POLLING else -1), (what, r["failed"], r["published"])
        assert np.all(r["rest"].view(np.uint64) == ZERO), (what, "constant keyframes", r["rest"])       # +0.0 in every slot of a constant keyframe
        return r["dp"]

    def exact(self, nfree, what):
        S, g, x = _exact(nfree)
        dp = self.solve(S, g, what)
        assert np.array_equal(dp.view(np.uint64), x.view(np.uint64)), (what, np.abs(dp - x).max(), np.nonzero(dp != x)[0][:8])


@functools.lru_cache(maxsize=None)
def _exact(nfree):
    return sg.exact(nfree, 0)


@functools.lru_cache(maxsize=None)
def _conditioned(nfree, kappa):
    """-> S, g, long-double reference, forward errors of the float64 yardstick and of np.linalg.solve (computed once, shared by every context and schedule)."""
    S, g = sg.conditioned(nfree, kappa)
    ref, _ = sg.reference(S, g)
    return S, g, ref, sg.forward_error(sg.yardstick(S, g), ref), sg.forward_error(np.linalg.solve(S, -g), ref)


@pytest.mark.parametrize("var", SCHEDULES)
@pytest.mark.parametrize("n_kf", N_KF)
def test_exact_family_every_bit(gpu, n_kf, var):
    """S = L D L^T of small dyadic numbers: no operation of an unpivoted LDL^T rounds, in any order, with or without FMA / MFMA -- dp == x bit for bit."""
    with _Ctx(gpu, n_kf, var) as c:
        for nfree in range(1, n_kf + 1):
            c.exact(nfree, (n_kf, var, nfree))


@pytest.mark.parametrize("var", SCHEDULES)
@pytest.mark.parametrize("n_kf", N_KF)
def test_bad_pivot_fails_the_step(gpu, n_kf, var):
    """One pivot -1, 0.0 or NaN at row r of block b (first, second, middle, last but one, last): the flag is raised in the LM state and, where the step
    is published, in the flag's slot; the step is +0.0 in every slot; the exact member afterwards on the same context (after the three values of each
    pivot) is exact again."""
    with _Ctx(gpu, n_kf, var) as c:
        for nfree in range(1, n_kf + 1):
            for b in sorted({0, min(1, nfree - 1), nfree//2, max(nfree - 2, 0), nfree - 1}):
                for r in range(6):
                    for v in (-1.0, 0.0, np.nan):
                        what = (n_kf, var, nfree, b, r, v)
                        S, g, _ = sg.exact(nfree, 0, bad=(b, r, v))
                        dp = c.solve(S, g, what, failed=1)
                        assert np.all(dp.view(np.uint64) == ZERO), (what, dp)
                    c.exact(nfree, (n_kf, var, nfree, b, r, "exact member afterwards"))


@pytest.mark.parametrize("var", SCHEDULES)
@pytest.mark.parametrize("n_kf", N_KF)
def test_assembly_failure_fails_the_step(gpu, n_kf, var):
    """The flag an assembly raises (inv_sym3 in k_schur_t) is LmState.step_fail on entry: even the exact system is then a failed step of zeros."""
    with _Ctx(gpu, n_kf, var) as c:
        for nfree in sorted({1, n_kf//2, n_kf}):
            S, g, _ = _exact(nfree)
            dp = c.solve(S, g, (n_kf, var, nfree), assembly_failed=True, failed=1)
            assert np.all(dp.view(np.uint64) == ZERO), (n_kf, var, nfree, dp)
            c.exact(nfree, (n_kf, var, nfree, "exact member afterwards"))


@pytest.mark.parametrize("var", SCHEDULES)
@pytest.mark.parametrize("n_kf", N_KF)
def test_conditioned_family_errors(gpu, n_kf, var):
    """S = Q diag(1 .. 1/kappa) Q^T, kappa = 1e2, 1e6, 1e10, n = 6 nfree rows.
    Backward error |S dp + g| / (|S| |dp| + |g|) (infinity norms, residual in long double) <= n 2^-53: the first-order Cholesky bound without its
    constant, not a measurement; the float64 yardstick (a plain LDL^T) stays below a tenth of it (tests/test_solve_given_ref.py).
    Forward error against the long-double reference, relative to |ref|: <= 8 x the larger of the yardstick's and np.linalg.solve's on the same
    system -- the two float64 solvers themselves lie several times apart on these systems, in either direction (up to 18 x at these seeds), so
    neither alone is the yardstick; the margin of 8 is over the worse of the two.  The measured ratios device / yardstick per
    (nfree, kappa) are in profiles/solve_given_accuracy.txt (tools/diag/gpu_solve_given_accuracy.py writes it)."""
    worst = (0.0, None); worst_be = (0.0, None)
    with _Ctx(gpu, n_kf, var) as c:
        for nfree in range(1, n_kf + 1):
            n = 6*nfree
            for kappa in sg.KAPPAS:
                S, g, ref, fe_y, fe_np = _conditioned(nfree, kappa)
                dp = c.solve(S, g, (n_kf, var, nfree, kappa))
                be, fe = sg.backward_error(S, dp, g), sg.forward_error(dp, ref)
                worst = max(worst, (fe/max(fe_y, fe_np), (nfree, kappa))); worst_be = max(worst_be, (be/(n*2.0**-53), (nfree, kappa)))
                assert be <= n*2.0**-53, (n_kf, var, nfree, kappa, "backward error / bound", be/(n*2.0**-53))
                assert fe <= 8.0*max(fe_y, fe_np), (n_kf, var, nfree, kappa, "forward error: device, yardstick, numpy", fe, fe_y, fe_np)
    print("n_kf %d variant %d: largest forward error / max(yardstick, numpy) %.3f at %s; largest backward error / bound %.4f at %s"
          % (n_kf, var, worst[0], worst[1], worst_be[0], worst_be[1]))


@pytest.mark.parametrize("var", SCHEDULES)
@pytest.mark.parametrize("n_kf", N_KF)
def test_non_finite_right_hand_side(gpu, n_kf, var):
    """The exact S with one NaN in g is NOT a failed step (every pivot is positive).  The solver's arithmetic is dense -- a zero of L is multiplied like
    any other entry -- so the NaN reaches every row from its own on in the forward substitution and from there every slot of the step in the back
    substitution, as it does in the float64 yardstick: every free slot is non-finite in every schedule.  The schedules that publish the step (production,
    5, 6) store +Inf where the others store NaN (co_store): NaN means "not there yet" to the blocks that poll, so a polled slot is never left NaN -- the
    back-substitution blocks would otherwise wait out their bound."""
    with _Ctx(gpu, n_kf, var) as c:
        for nfree in sorted({1, n_kf//2 + 1, n_kf}):
            S, g0, _ = _exact(nfree)
            for k in sorted({0, 3*nfree, 6*nfree - 1}):
                g = g0.copy(); g[k] = np.nan
                L, d, badk = sg.ldlt(S)
                assert badk < 0 and not np.isfinite(sg._substitute(L, d, -g)).any()          # (the yardstick: every slot)
                dp = c.solve(S, g, (n_kf, var, nfree, k))                                   # failed == 0, published flag 0: the flag's slot is not NaN either
                assert not np.isfinite(dp).any(), (n_kf, var, nfree, k, dp)
                if var in POLLING:
                    assert np.all(dp == np.inf), (n_kf, var, nfree, k, dp)
                else:
                    assert np.all(np.isnan(dp)), (n_kf, var, nfree, k, dp)
            c.exact(nfree, (n_kf, var, nfree, "exact member afterwards"))


@pytest.mark.parametrize("var", (0, 3))
def test_solve_after_the_hook_is_a_fresh_contexts(gpu, var):
    """tsba_debug_solve_given puts S, g, dp, the free blocks and the LM state back: tsba_solve afterwards gives the bits of a solve without the hook."""
    P, o = _window(11)
    try:
        gpu.debug_set(**({"solve_variant": var} if var else {}))
        gpu.upload(P, o)
        rep0 = gpu.solve(); G0 = gpu.download(P.copy()); tr0 = gpu.lm_trace(0)
        assert rep0["iters"][0] > 0 and rep0["accepted"][0] > 0
        gpu.upload(P, o)
        for nfree, bad in ((11, None), (7, (3, 2, np.nan)), (1, (0, 0, -1.0)), (5, None)):
            S, g, x = sg.exact(nfree, 0, bad=bad)
            r = gpu.solve_given(S, g)
            assert r["failed"] == (bad is not None)
        rep1 = gpu.solve(); G1 = gpu.download(P.copy()); tr1 = gpu.lm_trace(0)
        S, g, x = sg.exact(4, 0, bad=(3, 5, 0.0))                  # ... and between two solves of one upload
        assert gpu.solve_given(S, g)["failed"] == 1
        rep2 = gpu.solve(); G2 = gpu.download(P.copy()); tr2 = gpu.lm_trace(0)
    finally:
        gpu.debug_set()
    for rep, G, tr in ((rep1, G1, tr1), (rep2, G2, tr2)):
        assert rep["poll_timeouts"] == 0 and rep["status"] == rep0["status"]
        for f in ("iters", "accepted", "termination", "cost0", "cost1"):
            assert rep[f] == rep0[f], (f, rep[f], rep0[f])
        for f in ("pose", "rho"):
            assert np.array_equal(getattr(G, f).view(np.uint64), getattr(G0, f).view(np.uint64)), f
        assert tr.shape == tr0.shape and np.array_equal(tr.view(np.uint64), tr0.view(np.uint64))


def test_the_hook_refuses_what_it_is_not_for(gpu):
    from textslam_amd.optimizer import TsbaError
    P, o = _window(4)
    gpu.upload(P, o)
    S, g, _ = sg.exact(5, 0)
    with pytest.raises(TsbaError):                                 # more free blocks than keyframes
        gpu.solve_given(S, g)
    Q = synth.make_problem(1, 50, 0, seed=2, frozen_frac=1.0, n_levels=1)      # PoseOptim: no window
    oq = abi.options_pose(); oq.n_passes = 1; oq.levels[0] = 0
    gpu.upload(Q, oq)
    S, g, _ = sg.exact(1, 0)
    with pytest.raises(TsbaError, match="failed with -4"):
        gpu.solve_given(S, g)
