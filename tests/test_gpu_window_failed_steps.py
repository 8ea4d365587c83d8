"""Invalid LM steps end to end.  The invalid branch of lm_decide (tsba_kernels_step.h: `s.step_fail || !(mcc > 0.0)`) -- the halved radius, the counter, the
exit with termination 5 after five invalid steps in a row, TSBA_ERR_NUMERIC, parameters left at the last accepted state -- is taken under test only by large
maps (an iteration cap on the conjugate gradients, test_gpu_far.py, through k_decide).  A window takes the decision in the decision block of k_mid, in k_schur_t
and in k_pass_end, the fused pose-only kernel in a fourth place (tsba_pose.h).  Two recipes drive all of them into that branch, and the CPU oracle's
solve_traced says what must come out.  Both have no text planes and one pass at level 0.

(a) a step whose model change is not positive.  Every pose is the identity, K = (512, 512, 320, 240), every point sits at inverse depth 0.25 on the ray of an
    INTEGER pixel and is observed at exactly that pixel: the ray (u - 320)/512, the point ray/rho = 4 ray, the identity transform, the projection
    512 x/z + 320 are all exact in float64, so every residual is an exact 0, g = 0, dp = 0 and the model change is 0.  gradient_tolerance = -1 keeps the
    gradient test from ending the pass before its first trial.  Five invalid steps: radii 5000, 2500, 1250, 625, 625, termination 5.
(b) a failed factorisation.  One NaN in the u of a good scene observation of keyframe k -- the first, a middle and the last free block of an ordinary
    8-keyframe window -- makes that keyframe's diagonal block of S NaN: a pivot that is not positive.  The observation's coordinates reach the kernels
    only as operands of the scene residual (tsba_kernels_lin.h, tsba_kernels_step.h, tsba_pose.h: L.sc_uv), never an address.
    What (b) shows: the failed trial's zeros and flag reach every polling block (no poll runs into its bound), every schedule ends as the oracle does.
    What it cannot show: whether the decision needs `step_fail` -- the NaN that fails the factorisation makes the model change NaN as well, so the trial
    is invalid either way (with the term removed from lm_decide, or the solver's `if (bad)` store removed, (b) still passes: tried by hand).  In a window a
    pivot fails only through a NaN (S is a Gram matrix plus positive damping); the flag itself is tested on given systems, tests/test_gpu_solve_given.py.

Schedules: production, solve_variant = 3 (k_solve_t + k_back + k_decide), solve_variant = 6, pass_launches = 1, trial_launches = 1 -- report, trace and
parameters equal production's bit for bit (tests/test_gpu_solve_load.py's statement, for the case that file lacks)."""
import numpy as np
import pytest

from textslam_amd import synth, abi

pytestmark = pytest.mark.gpu

TSBA_ERR_NUMERIC = -3
SCHEDULES = ({}, {"solve_variant": 3}, {"solve_variant": 6}, {"pass_launches": 1}, {"trial_launches": 1})
RADII = [5000.0, 2500.0, 1250.0, 625.0, 625.0]
REPORT_FIELDS = ("iters", "accepted", "termination", "cost0", "cost1", "status")
PARAMS = ("pose", "rho", "sgood")


@pytest.fixture(scope="module")
def gpu():
    from textslam_amd.optimizer import Optimizer
    g = Optimizer(0)
    yield g
    g.close()


def one_pass(o):
    o.n_passes = 1; o.levels[0] = 0
    return o


def zero_residual_problem(n_kf):
    """Recipe (a): the co-visibility of a small synthetic problem, its geometry replaced by one whose residuals are exact zeros."""
    if n_kf == 1:
        P, o = synth.make_problem(1, 60, 0, seed=2, frozen_frac=1.0, n_levels=1), abi.options_pose()
    else:
        P, o = synth.make_problem(n_kf=n_kf, n_pt=40*n_kf, n_text=0, seed=70 + n_kf, n_levels=1), abi.options_local()
    rng = np.random.default_rng(7000 + n_kf)
    px = np.stack([rng.integers(16, 624, P.n_pt), rng.integers(16, 464, P.n_pt)], 1).astype(np.float64)
    P.K = np.array([512.0, 512.0, 320.0, 240.0])
    P.pose = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0]), (n_kf, 1))
    P.pt_host_Trw = np.tile(np.concatenate([np.eye(3), np.zeros((3, 1))], 1).reshape(-1), (P.n_pt, 1))
    P.pt_ray = np.stack([(px[:, 0] - 320.0)/512.0, (px[:, 1] - 240.0)/512.0], 1)
    P.rho = np.full(P.n_pt, 0.25)
    P.sobs_uv0[0] = px[P.sobs_pt[0]].copy()
    o = one_pass(o); o.gradient_tolerance = -1.0
    return P, o


def nan_observation_problem(k):
    """Recipe (b): one NaN in the u of the first good scene observation of keyframe k whose point is not hosted by k."""
    P = synth.make_problem(n_kf=8, n_pt=320, n_text=0, seed=3, n_levels=1)
    o = one_pass(abi.options_local())
    cand = np.nonzero((P.sobs_kf[0] == k) & (P.sgood[P.sobs_flag[0]] != 0) & (P.pt_host[P.sobs_pt[0]] != k))[0]
    assert cand.size > 0
    P.sobs_uv0[0][cand[0], 0] = np.nan
    return P, o


def _bits(v):
    return np.asarray(v, np.float64).view(np.uint64)


def _run(gpu, P, o, pose_only=False, **dbg):
    try:
        gpu.debug_set(**dbg)
        G = P.copy()
        if pose_only:
            rep = gpu.PoseOptim(G, options=o); tr = None
        else:
            gpu.upload(P, o); rep = gpu.solve(); gpu.download(G); tr = gpu.lm_trace(0)
    finally:
        gpu.debug_set()
    return rep, G, tr


def _same(run, ref, what):
    rep, G, tr = run; rep0, G0, tr0 = ref
    assert rep["poll_timeouts"] == 0, what
    for f in REPORT_FIELDS:                                       # (bit patterns: recipe (b)'s costs are NaN)
        a, b = np.atleast_1d(rep[f]), np.atleast_1d(rep0[f])
        assert np.array_equal(_bits(a), _bits(b)) if a.dtype.kind == "f" else np.array_equal(a, b), (what, f, rep[f], rep0[f])
    for f in PARAMS:
        a, b = getattr(G, f), getattr(G0, f)
        assert np.array_equal(_bits(a), _bits(b)) if a.dtype.kind == "f" else np.array_equal(a, b), (what, f)
    if tr0 is not None:
        assert tr.shape == tr0.shape and np.array_equal(_bits(tr), _bits(tr0)), (what, "lm_trace", tr, tr0)


def _five_invalid(rep, tr, what):
    assert rep["iters"][0] == 5 and rep["accepted"][0] == 0 and rep["termination"][0] == 5, (what, rep)
    if tr is not None:
        assert tr.shape == (5, 4) and np.all(tr[:, 3] == -1.0) and np.all(np.isnan(tr[:, 0])) and list(tr[:, 2]) == RADII, (what, tr)


def test_oracle_takes_the_invalid_branch(oracle_lib):
    """What the recipes give on the CPU oracle (no device involved): the expectations the device tests below compare with."""
    for n_kf in (5, 1):
        P, o = zero_residual_problem(n_kf)
        Q = P.copy(); rep, tr = oracle_lib.solve_traced(Q, o)
        assert rep["cost0"][0] == 0.0 and rep["n_sblock"][0] > 0, rep
        _five_invalid(rep, tr[0], ("oracle", "a", n_kf))
        assert np.all(tr[0][:, 1] == 0.0)                         # the model change is an exact zero
        assert np.array_equal(Q.pose, P.pose) and np.array_equal(Q.rho, P.rho)
    for k in (3, 5, 7):
        P, o = nan_observation_problem(k)
        Q = P.copy(); rep, tr = oracle_lib.solve_traced(Q, o)
        assert np.isnan(rep["cost0"][0]), rep
        _five_invalid(rep, tr[0], ("oracle", "b", k))
        assert np.array_equal(Q.pose, P.pose) and np.array_equal(Q.rho, P.rho)


def test_zero_model_change_window(gpu, oracle_lib):
    P, o = zero_residual_problem(5)
    Q = P.copy(); rep_o, tr_o = oracle_lib.solve_traced(Q, o)
    ref = _run(gpu, P, o)
    rep, G, tr = ref
    assert rep["cost0"][0] == 0.0, rep["cost0"]                   # (else an operation of the recipe rounds on the device: change the inputs, not the kernel)
    assert gpu.solver_info()["lds_solver"] == 1 and gpu.solver_info()["pose_kernel"] == 0
    _five_invalid(rep, tr, "production")
    assert np.array_equal(_bits(tr), _bits(tr_o[0])), (tr, tr_o[0])
    for f in ("iters", "accepted", "termination", "cost0", "cost1", "n_sblock"):
        assert rep[f] == rep_o[f], (f, rep[f], rep_o[f])
    assert rep["status"] == TSBA_ERR_NUMERIC and rep["poll_timeouts"] == 0
    assert np.array_equal(G.pose, P.pose) and np.array_equal(G.rho, P.rho) and np.array_equal(G.sgood, Q.sgood)
    for dbg in SCHEDULES[1:]:
        _same(_run(gpu, P, o, **dbg), ref, dbg)


def test_zero_model_change_pose_only(gpu, oracle_lib):
    """The fused pose-only kernel keeps no trace: report and pose.  pass_launches = 1: a launch per LM step (k_pose_iter); no_pose_kernel: the general pipeline."""
    P, o = zero_residual_problem(1)
    Q = P.copy(); rep_o, tr_o = oracle_lib.solve_traced(Q, o)
    for dbg in ({}, {"pass_launches": 1}):
        rep, G, _ = _run(gpu, P, o, pose_only=True, **dbg)
        assert rep["cost0"][0] == 0.0, (dbg, rep["cost0"])
        _five_invalid(rep, None, dbg)
        for f in ("iters", "accepted", "termination", "cost0", "cost1", "n_sblock"):
            assert rep[f] == rep_o[f], (dbg, f, rep[f], rep_o[f])
        assert rep["status"] == TSBA_ERR_NUMERIC and rep["poll_timeouts"] == 0, (dbg, rep)
        assert np.array_equal(G.pose, P.pose) and np.array_equal(G.rho, P.rho) and np.array_equal(G.sgood, Q.sgood), dbg
    rep, G, tr = _run(gpu, P, o, no_pose_kernel=1)                # the same problem through the window kernels (one free block): these keep a trace
    assert rep["cost0"][0] == 0.0
    _five_invalid(rep, tr, "no_pose_kernel")
    assert np.array_equal(_bits(tr), _bits(tr_o[0])) and rep["status"] == TSBA_ERR_NUMERIC and np.array_equal(G.pose, P.pose)


@pytest.mark.parametrize("k", [3, 5, 7])
def test_failed_factorisation_window(gpu, oracle_lib, k):
    P, o = nan_observation_problem(k)
    Q = P.copy(); rep_o, tr_o = oracle_lib.solve_traced(Q, o)
    ref = _run(gpu, P, o)
    rep, G, tr = ref
    free = gpu.reduced_system(o.initial_radius)["free"]
    assert list(np.nonzero(free)[0]) == [3, 4, 5, 6, 7]           # free blocks 0 .. 4 are keyframes 3 .. 7
    assert np.isnan(rep["cost0"][0]) and np.isnan(rep_o["cost0"][0])
    _five_invalid(rep, tr, "production"); _five_invalid(rep_o, tr_o[0], "oracle")
    assert np.array_equal(tr[:, 2:], tr_o[0][:, 2:])              # verdicts and radii
    assert rep["termination"] == rep_o["termination"] and rep["iters"] == rep_o["iters"] and rep["accepted"] == rep_o["accepted"]
    assert rep["status"] == TSBA_ERR_NUMERIC and rep["poll_timeouts"] == 0
    assert np.array_equal(G.pose, P.pose) and np.array_equal(G.rho, P.rho)
    for dbg in SCHEDULES[1:]:
        _same(_run(gpu, P, o, **dbg), ref, dbg)
