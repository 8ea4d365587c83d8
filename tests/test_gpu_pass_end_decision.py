"""The decision on a pass's LAST trial inside k_pass_end (windows on one GPU whose k_mid launches carry the decision block, tsba_kernels_pass.h): one more
workgroup of the pass's end-launch does what k_decide did as a launch of its own -- on the state in place, with the same sums in the same order -- while the
outlier waves, the next level's mu / sigma and the clearing workgroup take the one thing they need of its outcome, `cur`, from the record the last trial's
decision block left (Work::dec).  Nothing is computed differently, so production must equal, bit for bit, the generic pass driver
(tsba_debug_options.pass_launches = 1), which keeps k_decide behind every pass's last trial."""
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
    """(problem, options, one-shot call or None)"""
    o, oneshot = abi.options_local(), None
    if name == "tiny":                                          # (function-tolerance exits before the iteration limit)
        P = synth.tiny()
    elif name in ("c4", "c4_oneshot"):
        P = synth.config_c4()
        if name == "c4_oneshot":
            oneshot = "LocalBundleAdjustment"
    elif name == "init":
        P, o = synth.init_pair(), abi.options_init()
    elif name == "landmarker":
        P, o = synth.landmark_refine(), abi.options_landmarker()
    elif name == "no_text":
        P = synth.make_problem(n_kf=9, n_pt=700, n_text=0, seed=91, feats=(16, 8, 6))
        o.n_passes = 2; o.levels[0] = 0; o.levels[1] = 0          # (a scene-only synthetic problem has one pyramid level: two passes on it)
    elif name == "no_outlier":
        P = synth.make_problem(n_kf=12, n_pt=900, n_text=6, seed=92, feats=(16, 8, 6)); o.outlier_scene = o.outlier_text = 0
    elif name == "transitions":                                 # (rejected and re-accepted trials in pass 0: test_gpu_decision_block.py)
        P = synth.make_problem(n_kf=5, n_pt=300, n_text=2, seed=45, feats=(16, 8, 6)); o.its[0] = 30
    elif name == "one_trial":                                   # (every pass is its first trial: no decision before the end-launch's)
        P = synth.make_problem(n_kf=5, n_pt=300, n_text=2, seed=45, feats=(16, 8, 6))
        for ps in range(o.n_passes):
            o.its[ps] = 1
    elif name == "no_blocks":                                   # (every observation flagged bad: the passes are over at their first linearisation, no record is written)
        P = synth.tiny(seed=4); P.sgood[:] = 0; P.tobs_good[:] = 0
    else:
        raise ValueError(name)
    return P, o, oneshot


def _run(gpu, P, o, oneshot, first):
    G = P.copy()
    if oneshot:
        rep = getattr(gpu, oneshot)(G, options=o)
    else:
        if first:
            gpu.upload(P, o)
        rep = gpu.solve(); gpu.download(G)
    return rep, G, [gpu.lm_trace(ps) for ps in range(o.n_passes)]


def _same(run, ref, what):
    rep, G, traces = run; rep0, G0, traces0 = ref
    for f in REPORT_FIELDS:
        assert rep[f] == rep0[f], (what, f, rep[f], rep0[f])
    for f in PARAMS:
        assert np.array_equal(getattr(G, f), getattr(G0, f)), (what, f)
    assert len(traces) == len(traces0)
    for ps, (a, b) in enumerate(zip(traces, traces0)):          # (raw bit patterns: an invalid step's cost is NaN)
        assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), (what, "lm_trace", ps, a, b)


@pytest.mark.parametrize("case", ["tiny", "c4", "c4_oneshot", "init", "landmarker", "no_text", "no_outlier", "transitions", "one_trial", "no_blocks"])
def test_pass_end_decision_equals_k_decide(gpu, case):
    """Production (0) against pass_launches = 1, interleaved (0, 1, 0); a resident problem is solved three times per upload in production and must give the
    same bits every time.  Report fields, parameters, flags and the LM trace of every pass are compared bit for bit; no poll may run into its bound."""
    P, o, oneshot = _case(case)
    runs = {0: [], 1: []}
    try:
        for old in (0, 1, 0):
            gpu.debug_set(pass_launches=old)
            for rep_no in range(2 if old else 3):
                runs[old].append(_run(gpu, P, o, oneshot, rep_no == 0))
    finally:
        gpu.debug_set()
    ref = runs[1][0]
    assert all(r[0]["poll_timeouts"] == 0 for v in runs.values() for r in v)
    its = [o.its[ps] for ps in range(o.n_passes)]
    print(case, "iters", ref[0]["iters"], "of", its, "accepted", ref[0]["accepted"], "termination", ref[0]["termination"])
    if case == "no_blocks":
        assert ref[0]["iters"] == [0]*o.n_passes and np.array_equal(ref[1].pose, P.pose) and np.array_equal(ref[1].rho, P.rho)
    else:
        assert sum(ref[0]["iters"]) > 0
    if case == "tiny":                                          # (a pass that leaves on a tolerance before its iteration limit)
        assert any(t in (1, 2, 3) and n < m for t, n, m in zip(ref[0]["termination"], ref[0]["iters"], its)), (ref[0]["termination"], ref[0]["iters"])
    if case == "one_trial":
        assert ref[0]["iters"] == [1]*o.n_passes, ref[0]["iters"]
    if case == "transitions":                                   # (the last decisions of the passes are not all of one kind)
        assert 0 < sum(ref[0]["accepted"]) < sum(ref[0]["iters"]), (ref[0]["accepted"], ref[0]["iters"])
    for k, r in enumerate(runs[1][1:]):
        _same(r, ref, "pass_launches 1, run %d" % (k + 1))
    for k, r in enumerate(runs[0]):
        _same(r, ref, "production, run %d" % k)
