"""CPU diagnostic (not a pytest): the oracle against itself, analytic text Jacobians (the HIP kernels' choice) against the reference's
Ceres central differences (tsba_options.text_jacobian = 1).  One row per case: LM decisions, final-cost gap, largest parameter gaps,
flags decided differently; then C4 pass by pass from the numeric run's state (tests/test_gpu_reference_mode.py holds the GPU to these).
Output kept in profiles/reference_mode_gaps.txt."""
import os
import sys
import time
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import oracle                                            # noqa: E402
from textslam_amd import synth, abi                      # noqa: E402


def numeric(o):
    on = type(o).from_buffer_copy(o)
    on.text_jacobian = 1
    return on


def gap(a, b):
    return float(np.abs(a - b).max()) if a.size else 0.0


def row(name, P, o):
    A, N = P.copy(), P.copy()
    ra, ta = oracle.solve_traced(A, o)
    rn, tn = oracle.solve_traced(N, numeric(o))
    same = ra["iters"] == rn["iters"] and all(np.array_equal(x[:, 3], y[:, 3]) for x, y in zip(ta, tn))
    flags = (int(np.sum(A.sgood != N.sgood)), int(np.sum(A.tfgood != N.tfgood)), int(np.sum(A.tobs_good != N.tobs_good)))
    print(f"{name:18s} {'equal' if same else 'DIFFER':8s} {abs(ra['cost1'][-1] - rn['cost1'][-1]) / rn['cost1'][-1]:9.1e} "
          f"{gap(A.pose, N.pose):9.1e} {gap(A.rho, N.rho):9.1e} {gap(A.theta, N.theta):9.1e}   {flags}  iters {rn['iters']}", flush=True)


def theta_row(name, P, o, text):
    A, N = P.copy(), P.copy()
    _, ra, ca = oracle.theta_optim(A, o, text)
    _, rn, cn = oracle.theta_optim(N, numeric(o), text)
    print(f"{name:18s} {'equal' if ra['iters'] == rn['iters'] and ra['accepted'] == rn['accepted'] else 'DIFFER':8s} "
          f"{abs(ra['cost1'][-1] - rn['cost1'][-1]) / rn['cost1'][-1]:9.1e} {'-':>9s} {'-':>9s} {gap(A.theta, N.theta):9.1e}   "
          f"covariance rel {np.abs(ca - cn).max() / np.abs(cn).max():.1e}", flush=True)


t0 = time.time()
print(f"{'case':18s} {'LM':8s} {'cost rel':>9s} {'pose':>9s} {'rho':>9s} {'theta':>9s}   flags differing (sgood, tfgood, tobs_good)")
for s in (7, 21, 33):
    row(f"tiny seed {s}", synth.tiny(seed=s, n_kf=6, n_pt=150, n_text=5), abi.options_local())
row("tiny seed 31, 6 tx", synth.tiny(seed=31, n_kf=6, n_pt=150, n_text=6), abi.options_local())
row("C1", synth.config_c1(), abi.options_local())
row("C3 pose-only", synth.config_c3(), abi.options_pose())
row("init_pair", synth.init_pair(seed=5), abi.options_init())
row("landmark_refine", synth.landmark_refine(seed=9), abi.options_landmarker())
theta_row("theta single", synth.landmark_refine(seed=3, n_pt=0, n_text=2), abi.options_theta(), 1)
row("C4", synth.config_c4(), abi.options_local())

print("\nC4 pass by pass, each from the numeric run's state after the previous pass (objective = cost0 of a zero-iteration pass at the end point)")
P, o = synth.config_c4(), abi.options_local()
N = P.copy()
rep, tr, starts = oracle.solve_by_pass(N, numeric(o))
ends = starts[1:] + [N]
for ps in range(o.n_passes):
    o1 = oracle.pass_options(o, ps)
    A = starts[ps].copy(); ra, ta = oracle.solve_traced(A, o1)

    def objective(X):
        Q = starts[ps].copy(); Q.pose, Q.rho, Q.theta = X.pose.copy(), X.rho.copy(), X.theta.copy()
        oz = oracle.pass_options(o, ps); oz.its[0] = 0
        return oracle.solve(Q, oz)["cost0"][0]
    fa, fn = objective(A), objective(ends[ps])
    print(f"pass {ps} (level {o.levels[ps]}): decisions {'equal' if np.array_equal(ta[0][:, 3], tr[ps][:, 3]) else 'DIFFER'}, "
          f"cost1 rel {abs(ra['cost1'][0] - rep['cost1'][ps]) / rep['cost1'][ps]:.1e}, objective rel {abs(fa - fn) / fn:.1e}, "
          f"theta gap {gap(A.theta, ends[ps].theta):.1e}, flags differing (tfgood, tobs_good) "
          f"({int(np.sum(A.tfgood != ends[ps].tfgood))}, {int(np.sum(A.tobs_good != ends[ps].tobs_good))})", flush=True)
print(f"\n{time.time() - t0:.0f} s on one core")
