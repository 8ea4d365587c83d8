"""The decision block of k_mid's launch (windows on one GPU, tsba_kernels_lin.h: decision_block): the light part of an LM trial's decision -- accept / reject,
the trust-region radius, the linearisation that becomes current -- is taken by one more wave of the speculative k_mid launch and handed to the next k_schur_t<4>
in a small record (Work::dec); the full decision stays in k_schur_t, with a workgroup that assembles nothing.  Nothing is computed differently, so production
must equal, bit for bit, the schedule that takes every decision with k_decide as a launch of its own (tsba_debug_options.solve_variant = 3)."""
import numpy as np
import pytest

from textslam_amd import synth, abi

pytestmark = pytest.mark.gpu

REPORT_FIELDS = ("iters", "accepted", "termination", "cost0", "cost1", "n_sblock", "n_tblock", "n_bad_scene", "n_bad_tfeat", "n_bad_text")
PARAMS = ("pose", "rho", "theta", "sgood", "tobs_good", "tfgood")


@pytest.fixture(scope="module")
def gpu():
    from textslam_amd.optimizer import Optimizer
    return Optimizer(0)


def _case(name):
    o = abi.options_local()
    if name == "transitions":
        P = synth.make_problem(n_kf=5, n_pt=300, n_text=2, seed=45, feats=(16, 8, 6)); o.its[0] = 30
    elif name == "tiny":
        P = synth.tiny()
    elif name == "no_outlier":
        P = synth.make_problem(n_kf=12, n_pt=900, n_text=6, seed=92, feats=(16, 8, 6)); o.outlier_scene = o.outlier_text = 0
    elif name == "no_text":
        P = synth.make_problem(n_kf=9, n_pt=700, n_text=0, seed=91, feats=(16, 8, 6))
        o.n_passes = 2; o.levels[0] = 0; o.levels[1] = 0          # (a scene-only synthetic problem has one pyramid level: two passes on it)
    else:
        n_kf = int(name[2:])
        P = synth.make_problem(n_kf=n_kf, n_pt=60*n_kf, n_text=max(2, n_kf//2), seed=40 + n_kf, feats=(16, 8, 6))
    return P, o


def _same(run, ref, what):
    rep, G, traces = run; rep0, G0, traces0 = ref
    for f in REPORT_FIELDS:
        assert rep[f] == rep0[f], (what, f, rep[f], rep0[f])
    for f in PARAMS:
        assert np.array_equal(getattr(G, f), getattr(G0, f)), (what, f)
    assert len(traces) == len(traces0)
    for ps, (a, b) in enumerate(zip(traces, traces0)):          # (raw bit patterns: an invalid step's cost is NaN)
        assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), (what, "lm_trace", ps, a, b)


@pytest.mark.parametrize("case", ["transitions", "tiny", "no_outlier", "kf31", "kf32", "kf33", "no_text"])
def test_decision_block_equals_k_decide(gpu, case):
    """Production against solve_variant = 3, bit for bit: parameters, flags, every per-pass report field and the LM trace of every pass -- solved twice on one
    upload with the two settings interleaved (0, 3, 0), and through the one-shot LocalBundleAdjustment call.  No poll may run into its bound.
    transitions: a window whose first pass rejects and re-accepts (the CPU oracle's verdicts of pass 0 with 30 trials allowed: 1 1 1 1 1 1 0 0 0 0 0 1 0 1 2); what
                 is asserted about the trajectory is asserted on the PARTNER's trace: at least two trials not accepted, an accepted trial directly after one that
                 was not, and one that was not directly after an accepted one -- every transition of lcur / fresh / radius that the record carries.
    tiny:        function-tolerance exits.        no_outlier: the outlier passes off.        no_text: no plane blocks, no text groups under any pair.
    kf31, kf32:  the largest windows of the path (SCHUR_KEEP_KF = 32); kf33 takes k_decide in both settings and must simply agree."""
    P, o = _case(case)
    fused = P.n_kf <= 32                                        # (SCHUR_KEEP_KF)
    runs = {0: [], 3: []}
    try:
        for var in (0, 3, 0):
            gpu.debug_set(solve_variant=var)
            gpu.upload(P, o)
            if var == 0 and case != "kf33":
                assert gpu.solver_info()["lds_solver"] == 1 and fused      # (the reduced system in LDS and at most 32 keyframes: the trials' decisions are fused)
            for rep_no in range(2):
                G = P.copy(); rep = gpu.solve(); gpu.download(G)
                runs[var].append((rep, G, [gpu.lm_trace(ps) for ps in range(o.n_passes)]))
            G = P.copy(); rep = gpu.LocalBundleAdjustment(G, options=o)
            runs[var].append((rep, G, [gpu.lm_trace(ps) for ps in range(o.n_passes)]))
    finally:
        gpu.debug_set()
    ref = runs[3][0]
    assert sum(ref[0]["iters"]) > 0
    assert all(r[0]["poll_timeouts"] == 0 for v in runs.values() for r in v)
    if case == "transitions":
        v = ref[2][0][:, 3]; bad = (v == 0.0) | (v == -1.0); ok = v == 1.0
        print("partner's verdicts of pass 0:", v)
        assert bad.sum() >= 2 and np.any(bad[:-1] & ok[1:]) and np.any(ok[:-1] & bad[1:]), v
    if case == "tiny":
        assert 1 in ref[0]["termination"], ref[0]["termination"]          # (a function-tolerance exit)
    for k, r in enumerate(runs[3][1:]):
        _same(r, ref, "solve_variant 3, run %d" % (k + 1))
    for k, r in enumerate(runs[0]):
        _same(r, ref, "production, run %d" % k)
