"""GPU tests: the solves against the REFERENCE's differentiation of the text residuals.

The reference differentiates every photometric functor numerically (ceres::NumericDiffCostFunction<CENTRAL>: nume_BAText.h,
nume_PoseOptimText.h, nume_IniBAText.h, nume_thetaText.h); the HIP kernels use the analytic bilinear Jacobian ("Text Jacobians
are analytic").  tests/test_gpu_parity.py pins the kernels to the oracle in analytic mode; here the oracle runs the reference's way
(tsba_options.text_jacobian = 1) and each solve is held to how far it may sit from that.

Chained, as the caller runs it -- per pass:
  iters, accepted, termination   equal
  LM decision of every trial     equal (accepted / rejected / invalid step / tolerance exit).  The fused pose-only kernel and the batched
                                 theta kernel keep no per-trial trace: there the counts above
  cost0 of pass 0                rel 1e-12 (no Jacobian in it)
  theta covariance               rel 1e-6
  flags                          every flag that differs is NEAR ITS THRESHOLD: at a pass that judged it, its outlier statistic
                                 (oracle.outlier_stats) at the numeric run's parameters lies within FLAG_MARGIN (relative) of chi2_mono /
                                 chi2_text; a text observation that differs has enough such borderline features to cross
                                 text_bad_ratio, and the features of that observation follow it (flag_distances)
  parameters, final cost         no further from the numeric run than the oracle's analytic run is, plus test_gpu_parity.py's tolerance of
                                 the GPU against the analytic oracle (triangle inequality): the Jacobian choice explains the whole gap.
                                 The gaps are printed ("Against the reference's numeric differentiation").
Per pass from a common start (C4, init_pair, C1) -- pass k from the numeric run's state after pass k - 1 (oracle.pass_options):
  the same decisions, near-threshold flags only, and the reference objective at the two end points (the cost0 of a zero-iteration pass
  over the start's flags) no further apart than at the analytic oracle's end point, plus 1e-9 relative.  This comparison is blind to the
  flat directions, along which theta may move 1e-2 in a level-2 pass that does not converge.
"""
import numpy as np
import pytest

from textslam_amd import synth, abi

pytestmark = pytest.mark.gpu

FLAG_MARGIN = 0.1        # |statistic - threshold| / threshold of a flag the two runs decide differently


@pytest.fixture(scope="module")
def gpu():
    from textslam_amd.optimizer import Optimizer
    return Optimizer(0)


def _tiny(seed, n_text=5):
    return synth.tiny(seed=seed, n_kf=6, n_pt=150, n_text=n_text)


# name -> (problem, options, entry point, parameter tolerance and final-cost tolerance of the GPU against the analytic oracle (test_gpu_parity.py))
CASES = {
    "tiny7": (lambda: _tiny(7), abi.options_local, "local", 1e-8, 1e-9),
    "tiny21": (lambda: _tiny(21), abi.options_local, "local", 1e-8, 1e-9),
    "tiny33": (lambda: _tiny(33), abi.options_local, "local", 1e-8, 1e-9),
    "tiny31_6texts": (lambda: _tiny(31, 6), abi.options_local, "local", 1e-8, 1e-9),
    "c1": (synth.config_c1, abi.options_local, "local", 1e-7, 1e-9),
    "c3_resident": (synth.config_c3, abi.options_pose, "pose_resident", 1e-7, 1e-9),
    "c3_oneshot": (synth.config_c3, abi.options_pose, "pose", 1e-7, 1e-9),
    "c4": (synth.config_c4, abi.options_local, "local", 1e-7, 1e-9),
    "init_pair": (lambda: synth.init_pair(seed=5), abi.options_init, "init", 1e-4, 1e-5),
    "landmark_refine": (lambda: synth.landmark_refine(seed=9), abi.options_landmarker, "landmarker", 1e-8, 1e-9),
}
_CACHE = {}


def _numeric(o):
    on = type(o).from_buffer_copy(o)
    on.text_jacobian = 1
    return on


def _oracle_runs(oracle, name):
    """The case's problem, options, the numeric oracle run pass by pass (report, traces, start of every pass, end) and the analytic one."""
    if name not in _CACHE:
        make, opts = CASES[name][:2]
        P, o = make(), opts()
        N = P.copy()
        rep_n, tr_n, starts = oracle.solve_by_pass(N, _numeric(o))
        A = P.copy()
        rep_a = oracle.solve(A, o)
        _CACHE[name] = (P, o, (rep_n, tr_n, starts, N), (rep_a, A))
    return _CACHE[name]


def run_gpu(gpu, kind, P, o):
    """One solve through the entry point the caller uses; -> (end state, report, per-pass LM traces or None where the kernel keeps none)."""
    G = P.copy()
    if kind == "local":
        rep = gpu.LocalBundleAdjustment(G, options=o)
    elif kind == "pose":
        rep = gpu.PoseOptim(G, options=o)
    elif kind == "pose_resident":
        gpu.upload(P, o); rep = gpu.solve(); gpu.download(G)
    elif kind == "init":
        rep = gpu.InitBA(G, options=o)
    else:
        rep = gpu.OptimizeLandmarker(G, options=o)
    traces = None if kind.startswith("pose") else [gpu.lm_trace(ps) for ps in range(o.n_passes)]
    return G, rep, traces


def flag_distances(oracle, o, starts, ends, G, N):
    """For every flag that G and N (the numeric run's end) decide differently: the smallest distance to its threshold over the passes that
    judged it, at the numeric run's parameters (relative: |statistic - chi2| / chi2).  A text observation that the two runs decide
    differently gets, instead, the distance of its flagged-feature count from the count that flips it (bad > text_bad_ratio * blocks) less the
    number of its features within FLAG_MARGIN of chi2_text -- <= 0 when the borderline features alone can flip it.  A feature of such an
    observation is not judged on its own: from that pass on, the observation is in one run and not in the other.  -> dict name -> array."""
    diff = {"sgood": np.nonzero(G.sgood != N.sgood)[0], "tfgood": np.nonzero(G.tfgood != N.tfgood)[0],
            "tobs_good": np.nonzero(G.tobs_good != N.tobs_good)[0]}
    obs_of = np.searchsorted(N.tobs_fgood_off, diff["tfgood"], side="right") - 1
    diff["tfgood"] = diff["tfgood"][~np.isin(obs_of, diff["tobs_good"])]
    out = {k: np.full(v.size, np.inf) for k, v in diff.items()}
    if not any(v.size for v in diff.values()):
        return out
    for ps in range(len(starts)):
        st = oracle.outlier_stats(starts[ps], oracle.pass_options(o, ps), 0, end=ends[ps])
        with np.errstate(invalid="ignore"):
            if o.outlier_scene:
                d = np.abs(st["s_stat"][diff["sgood"]] - st["chi2_mono"]) / st["chi2_mono"]
                out["sgood"] = np.fmin(out["sgood"], np.where(np.isnan(d), np.inf, d))
            if o.outlier_text:
                d = np.abs(st["tf_stat"][diff["tfgood"]] - st["chi2_text"]) / st["chi2_text"]
                out["tfgood"] = np.fmin(out["tfgood"], np.where(np.isnan(d), np.inf, d))
                for i, t in enumerate(diff["tobs_good"]):
                    f = st["tf_stat"][N.tobs_fgood_off[t]:N.tobs_fgood_off[t + 1]]
                    f = f[~np.isnan(f)]
                    if f.size == 0:
                        continue
                    bad = int(np.sum(f > st["chi2_text"]))
                    near = int(np.sum(np.abs(f - st["chi2_text"]) <= FLAG_MARGIN * st["chi2_text"]))
                    out["tobs_good"][i] = min(out["tobs_good"][i], abs(bad - st["text_bad_ratio"] * f.size) - near)
    return out


def assert_near_threshold(dist):
    for k, d in dist.items():
        lim = 0.0 if k == "tobs_good" else FLAG_MARGIN
        assert np.all(d <= lim), (k, d[d > lim], lim)


def gaps(X, N, rep_x, rep_n):
    return {"pose": float(np.abs(X.pose - N.pose).max()),
            "rho": float(np.abs(X.rho - N.rho).max()) if X.rho.size else 0.0,
            "theta": float(np.abs(X.theta - N.theta).max()) if X.theta.size else 0.0,
            "cost": abs(rep_x["cost1"][-1] - rep_n["cost1"][-1]) / rep_n["cost1"][-1]}


def _flags(X):
    return np.concatenate([X.sgood, X.tfgood, X.tobs_good])


def check_chained(oracle, name, G, rep_g, tr_g, run_prefix):
    """run_prefix(n) -> the end state of the same call with only its first n passes (where the two runs' flags first part)."""
    P, o, (rep_n, tr_n, starts, N), (rep_a, A) = _oracle_runs(oracle, name)
    tol, tol_cost = CASES[name][3:]
    assert rep_g["iters"] == rep_n["iters"] and rep_g["accepted"] == rep_n["accepted"], (rep_g, rep_n)
    assert rep_g["termination"] == rep_n["termination"]
    if tr_g is not None:
        for ps in range(o.n_passes):
            assert np.array_equal(tr_g[ps][:, 3], tr_n[ps][:, 3]), (ps, tr_g[ps][:, 3], tr_n[ps][:, 3])
    np.testing.assert_allclose(rep_g["cost0"][0], rep_n["cost0"][0], rtol=1e-12)
    # flags: judged at the first pass after which the two runs' flags differ; the passes after it solve different problems (the flags
    # decide which blocks take part), they are compared from a common start in test_per_pass_from_common_start_against_numeric_mode
    ends = starts[1:] + [N]
    first = next((ps for ps in range(o.n_passes) if not np.array_equal(_flags(run_prefix(ps + 1) if ps + 1 < o.n_passes else G), _flags(ends[ps]))), None)
    dist = {}
    if first is not None:
        Gf = run_prefix(first + 1) if first + 1 < o.n_passes else G
        dist = flag_distances(oracle, oracle.pass_options(o, first), [starts[first]], [ends[first]], Gf, ends[first])
    n_end = {"sgood": int(np.sum(G.sgood != N.sgood)), "tfgood": int(np.sum(G.tfgood != N.tfgood)), "tobs_good": int(np.sum(G.tobs_good != N.tobs_good))}
    g_gpu, g_ana = gaps(G, N, rep_g, rep_n), gaps(A, N, rep_a, rep_n)
    print(f"\n{name}: GPU vs numeric {g_gpu}; analytic oracle vs numeric {g_ana}; flags differing at the end {n_end}; "
          f"first parted after pass {first}: {[(k, v.size, float(v.max())) for k, v in dist.items() if v.size]}")
    assert_near_threshold(dist)
    for k in ("pose", "rho", "theta"):
        assert g_gpu[k] <= g_ana[k] + tol, (k, g_gpu[k], g_ana[k])
    assert g_gpu["cost"] <= g_ana["cost"] + tol_cost, (g_gpu["cost"], g_ana["cost"])
    return g_gpu, n_end


def prefix_options(o, n):
    on = type(o).from_buffer_copy(o)
    on.n_passes = n
    return on


@pytest.mark.parametrize("name", list(CASES))
def test_chained_solve_against_numeric_mode(gpu, oracle_lib, name):
    P, o = _oracle_runs(oracle_lib, name)[:2]
    kind = CASES[name][2]
    G, rep_g, tr_g = run_gpu(gpu, kind, P, o)
    check_chained(oracle_lib, name, G, rep_g, tr_g, lambda n: run_gpu(gpu, kind, P, prefix_options(o, n))[0])


def _theta_numeric(oracle, P, o, text):
    R = P.copy()
    buf = np.full((4, 64, 4), np.nan)
    oracle.set_trace(buf, 64)
    try:
        rc, rep, cov = oracle.theta_optim(R, _numeric(o), text)
    finally:
        oracle.set_trace()
    return R, rc, rep, cov, [buf[k, :min(rep["iters"][k], 64)] for k in range(rep["n_passes"])]


def test_theta_optim_against_numeric_mode(gpu, oracle_lib):
    """ThetaOptimMultiFs (single plane, through the window pipeline): decisions, theta and the covariance against nume_thetaText's numeric
    derivative."""
    P = synth.landmark_refine(seed=3, n_pt=0, n_text=2)
    o = abi.options_theta()
    R, rc, rep_n, cov_n, tr_n = _theta_numeric(oracle_lib, P, o, 1)
    A = P.copy(); _, rep_a, cov_a = oracle_lib.theta_optim(A, o, 1)
    G = P.copy(); rep_g, cov_g = gpu.ThetaOptimMultiFs(G, text=1, options=o)
    assert rc == 0 and rep_g["cov_valid"] == 1
    assert rep_g["iters"] == rep_n["iters"] and rep_g["accepted"] == rep_n["accepted"] and rep_g["termination"] == rep_n["termination"]
    for ps in range(o.n_passes):
        assert np.array_equal(gpu.lm_trace(ps)[:, 3], tr_n[ps][:, 3])
    np.testing.assert_allclose(rep_g["cost0"][0], rep_n["cost0"][0], rtol=1e-12)
    np.testing.assert_allclose(cov_g, cov_n, rtol=1e-6)
    gap, gap_a = np.abs(G.theta - R.theta).max(), np.abs(A.theta - R.theta).max()
    print(f"\ntheta single: GPU vs numeric theta {gap:.1e} (analytic oracle {gap_a:.1e}), covariance {np.abs(cov_g - cov_n).max() / np.abs(cov_n).max():.1e}")
    assert gap <= gap_a + 1e-8


def test_theta_optim_batch_against_numeric_mode(gpu, oracle_lib):
    """tsba_theta_optim_batch (k_theta_batch) on twelve planes, each against its own numeric oracle run."""
    planes = synth.theta_planes(seed=5, n=12)
    o = abi.options_theta()
    work = [P.copy() for P in planes]
    reps, covs = gpu.ThetaOptimMultiFsBatch(work, options=o)
    worst = [0.0, 0.0]
    for i, P in enumerate(planes):
        R, rc, rep_n, cov_n, _ = _theta_numeric(oracle_lib, P, o, 0)
        A = P.copy(); oracle_lib.theta_optim(A, o, 0)
        r = reps[i]
        assert r["iters"] == rep_n["iters"] and r["accepted"] == rep_n["accepted"] and r["termination"] == rep_n["termination"], (i, r, rep_n)
        np.testing.assert_allclose(r["cost0"][0], rep_n["cost0"][0], rtol=1e-12)
        assert r["cov_valid"] == (1 if rc == 0 else 0)
        if rc == 0:
            np.testing.assert_allclose(covs[i], cov_n, rtol=1e-6)
            worst[1] = max(worst[1], float(np.abs(covs[i] - cov_n).max() / np.abs(cov_n).max()))
        gap = np.abs(work[i].theta - R.theta).max()
        assert gap <= np.abs(A.theta - R.theta).max() + 1e-8, i
        worst[0] = max(worst[0], float(gap))
    print(f"\ntheta batch: GPU vs numeric theta {worst[0]:.1e}, covariance {worst[1]:.1e}")


def _objective(oracle, start, X, o1):
    """The reference objective at X's parameters over start's flags: cost0 of a zero-iteration pass (mu / sigma at X)."""
    Q = start.copy()
    Q.pose, Q.rho, Q.theta = X.pose.copy(), X.rho.copy(), X.theta.copy()
    oz = type(o1).from_buffer_copy(o1)
    oz.its[0], oz.text_jacobian = 0, 0
    return oracle.solve(Q, oz)["cost0"][0]


def check_per_pass(oracle, name, run_one):
    """Every pass of `name` from the numeric run's state after the previous pass: run_one(start, options) -> (end, report, trace of the pass)."""
    P, o, (rep_n, tr_n, starts, N), _ = _oracle_runs(oracle, name)
    ends = starts[1:] + [N]
    rows = []
    for ps in range(o.n_passes):
        o1 = oracle.pass_options(o, ps)
        G, rep_g, tr_g = run_one(starts[ps], o1)
        A = starts[ps].copy(); oracle.solve(A, o1)
        assert rep_g["iters"] == [rep_n["iters"][ps]] and rep_g["accepted"] == [rep_n["accepted"][ps]], (ps, rep_g, rep_n)
        assert rep_g["termination"] == [rep_n["termination"][ps]]
        assert np.array_equal(tr_g[:, 3], tr_n[ps][:, 3]), (ps, tr_g[:, 3], tr_n[ps][:, 3])
        dist = flag_distances(oracle, o1, [starts[ps]], [ends[ps]], G, ends[ps])
        assert_near_threshold(dist)
        fn, fg, fa = (_objective(oracle, starts[ps], X, o1) for X in (ends[ps], G, A))
        rows.append((ps, abs(fg - fn) / fn, abs(fa - fn) / fn, float(np.abs(G.theta - ends[ps].theta).max()) if G.theta.size else 0.0,
                     {k: int(v.size) for k, v in dist.items()}))
        assert abs(fg - fn) / fn <= abs(fa - fn) / fn + 1e-9, rows[-1]
    print(f"\n{name} per pass (pass, objective GPU vs numeric, analytic oracle vs numeric, theta gap, flags differing): {rows}")
    return rows


PER_PASS = {"c4": "local", "init_pair": "init", "c1": "local"}


@pytest.mark.parametrize("name", list(PER_PASS))
def test_per_pass_from_common_start_against_numeric_mode(gpu, oracle_lib, name):
    kind = PER_PASS[name]

    def run_one(start, o1):
        G, rep, tr = run_gpu(gpu, kind, start, o1)
        return G, rep, tr[0]
    check_per_pass(oracle_lib, name, run_one)
