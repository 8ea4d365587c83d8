"""The solver workgroup of k_solve_back (tsba_solve.h: solve_body): the panel waves load block column 0 and run block step 0 while the other ten waves load
everything right of it by rows, in one global round trip; the pose step is stored by one thread per slot, which looks its keyframe's free block up while the
back-substitution runs (constant keyframes' zeros and the flag leave at once); a back block sums its two partials in one pass.  None of that changes an
operation or its operands, so production must equal, bit for bit, the schedule it replaced (tsba_debug_options.solve_variant = 6: element-by-element load behind
a barrier, a store loop of one thread per keyframe) and the solver with the back-substitution as a launch of its own (solve_variant = 3: k_solve_t + k_back +
k_decide).

The windows are those of test_small_window_solver_schedules_agree: 4, 5, 7, 20 (C4) and 31 keyframes = 1, 2, 4, 17 and 28 free poses -- one block (no step
behind step 0), fewer rows than one round of the panel lanes, rows past the loader waves' first batch and past one round of the panel lanes (28 free poses:
168 rows), and 10 / 20 blocks of the back-substitution's register sets.

(A numerically failed factorisation -- a non-positive pivot -- under the same schedules: tests/test_gpu_window_failed_steps.py.)"""
import numpy as np
import pytest

from textslam_amd import synth, abi

pytestmark = pytest.mark.gpu

REPORT_FIELDS = ("iters", "accepted", "termination", "cost0", "cost1")
PARAMS = ("pose", "rho", "theta")


@pytest.fixture(scope="module")
def gpu():
    from textslam_amd.optimizer import Optimizer
    g = Optimizer(0)
    yield g
    g.close()


def _problem(n_kf):
    return synth.config_c4() if n_kf == 20 else synth.make_problem(n_kf=n_kf, n_pt=60*n_kf, n_text=max(2, n_kf//2), seed=40 + n_kf, feats=(16, 8, 6))


def _run(gpu, P, o, n_solves=1, **dbg):
    """Upload under the debug switches `dbg`, the first reduced system's step, then n_solves solves -> [(dp, report, parameters, traces)]."""
    out = []
    try:
        gpu.debug_set(**dbg)
        gpu.upload(P, o)
        dp = gpu.reduced_system(o.initial_radius)["dp"].copy()
        for _ in range(n_solves):
            rep = gpu.solve(); G = gpu.download(P.copy())
            out.append((dp, rep, G, [gpu.lm_trace(ps) for ps in range(o.n_passes)]))
    finally:
        gpu.debug_set()
    return out


def _same(run, ref, what):
    dp, rep, G, traces = run; dp0, rep0, G0, traces0 = ref
    assert rep["poll_timeouts"] == 0 and rep0["poll_timeouts"] == 0, what
    assert np.array_equal(dp.view(np.uint64), dp0.view(np.uint64)), (what, "dp")
    for f in REPORT_FIELDS:
        assert rep[f] == rep0[f], (what, f, rep[f], rep0[f])
    for f in PARAMS:
        assert np.array_equal(getattr(G, f), getattr(G0, f)), (what, f)
    assert len(traces) == len(traces0)
    for ps, (a, b) in enumerate(zip(traces, traces0)):          # (raw bit patterns: an invalid step's cost is NaN)
        assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), (what, "lm_trace", ps, a, b)


@pytest.fixture(scope="module")
def production(gpu):
    """The production result of each window, computed once: n_kf -> (problem, options, run)."""
    cache = {}

    def get(n_kf):
        if n_kf not in cache:
            P, o = _problem(n_kf), abi.options_local()
            cache[n_kf] = (P, o, _run(gpu, P, o)[0])
        return cache[n_kf]
    return get


@pytest.mark.parametrize("n_kf", [4, 5, 7, 20, 31])
def test_same_bits_as_the_old_schedule(gpu, production, n_kf):
    P, o, ref = production(n_kf)
    assert np.abs(ref[0]).max() > 0 and sum(ref[1]["iters"]) > 0
    for var in (6, 3):
        _same(_run(gpu, P, o, solve_variant=var)[0], ref, "solve_variant %d" % var)
        assert gpu.solver_info()["lds_solver"] == 1


def test_constant_keyframes_between_free_ones(gpu):
    """Keyframes 5 and 7 of ten held constant through the problem's own flags: free blocks on both sides of each, so a slot's free block is not its keyframe
    shifted, and the constant keyframes' slots are the zeros stored before the back-substitution ends."""
    P = synth.make_problem(n_kf=10, n_pt=600, n_text=5, seed=50, feats=(16, 8, 6))
    P.kf_initial[5] = 1; P.kf_initial[7] = 1
    o = abi.options_local()
    ref = _run(gpu, P, o)[0]
    free = gpu.reduced_system(o.initial_radius)["free"] != 0
    assert free[4] and not free[5] and free[6] and not free[7] and free[8] and free[9], free
    dp = ref[0].reshape(-1, 6)
    assert np.all(dp[~free] == 0.0) and np.all(np.abs(dp[free]).max(axis=1) > 0)
    assert sum(ref[1]["iters"]) > 0
    for var in (6, 3):
        _same(_run(gpu, P, o, solve_variant=var)[0], ref, "solve_variant %d" % var)


@pytest.mark.parametrize("n_kf", [5, 20, 31])
def test_every_lds_word_the_factorisation_uses_is_written(gpu, production, n_kf):
    """tsba_debug_options.lds_poison: NaNs / 1e300 / 0x5a bytes in the LDS of every compute unit before every launch."""
    P, o, ref = production(n_kf)
    for pz in (1, 2, 3):
        _same(_run(gpu, P, o, lds_poison=pz)[0], ref, "lds_poison %d" % pz)


@pytest.mark.parametrize("n_kf", [7, 20])
def test_repeated_solves_on_one_upload(gpu, production, n_kf):
    """Three solves in a row: every trial finds the step's slots NaN ("not there yet") although some stores of the trial before left before its step was solved."""
    P, o, ref = production(n_kf)
    for k, r in enumerate(_run(gpu, P, o, n_solves=3)):
        _same(r, ref, "solve %d" % k)
