"""GPU diagnostic (not a pytest): the window solver's forward error on the conditioned family of tests/solve_given_ref.py, per (free blocks, kappa), as a
ratio to the float64 yardstick's -- the table in profiles/solve_given_accuracy.txt.  Usage: python tools/diag/gpu_solve_given_accuracy.py [out.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                                        # noqa: E402
from textslam_amd import synth, abi                       # noqa: E402
from textslam_amd.optimizer import Optimizer              # noqa: E402
import solve_given_ref as sg                              # noqa: E402

N_KF = 31
SCHEDULES = (0, 1, 3, 6)                                  # production; k_solve_la; k_solve_t; production's former load and publication
out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
gpu = Optimizer(0)
P = synth.make_problem(n_kf=N_KF, n_pt=30*N_KF, n_text=0, seed=60 + N_KF, n_levels=1)
o = abi.options_local(); o.n_passes = 1; o.levels[0] = 0
rows = {}
for var in SCHEDULES:
    gpu.debug_set(**({"solve_variant": var} if var else {}))
    gpu.upload(P, o)
    for nfree in range(1, N_KF + 1):
        for kappa in sg.KAPPAS:
            S, g = sg.conditioned(nfree, kappa)
            ref, _ = sg.reference(S, g)
            fy, fn = sg.forward_error(sg.yardstick(S, g), ref), sg.forward_error(np.linalg.solve(S, -g), ref)
            r = gpu.solve_given(S, g)
            assert r["failed"] == 0
            rows.setdefault((nfree, kappa), [fy, fn, sg.backward_error(S, sg.yardstick(S, g), g)/(6*nfree*2.0**-53)]).extend(
                [sg.forward_error(r["dp"], ref)/fy, sg.backward_error(S, r["dp"], g)/(6*nfree*2.0**-53)])
gpu.debug_set()
print("# Window LDL^T solver (tsba_solve.h) on S = Q diag(1 .. 1/kappa) Q^T, n = 6 nfree rows, context of %d keyframes (tsba_debug_solve_given)." % N_KF, file=out)
print("# fe: forward error against a long-double LDL^T with two refinement steps, relative to |ref|_inf.  be: backward error / (n 2^-53).", file=out)
print("# yard: float64 LDL^T on the CPU; numpy: np.linalg.solve; v0 production (k_solve_back), v1 k_solve_la, v3 k_solve_t, v6 production's former load.", file=out)
print("# The test's bound: fe(device) <= 8 max(fe(yard), fe(numpy)), be(device) <= 1.", file=out)
print("# nfree kappa   fe(yard)  fe(numpy)/fe(yard) be(yard) | " + " | ".join("fe(v%d)/fe(yard) be(v%d)" % (v, v) for v in SCHEDULES), file=out)
worst = 0.0
for (nfree, kappa), v in sorted(rows.items()):
    worst = max(worst, max(v[3::2])/max(1.0, v[1]/v[0]))
    print("%5d %5.0e  %9.3e  %8.3f  %8.4f | " % (nfree, kappa, v[0], v[1]/v[0], v[2]) + " | ".join("%8.3f %8.4f" % (v[3 + 2*i], v[4 + 2*i]) for i in range(len(SCHEDULES))), file=out)
print("# largest fe(device) / max(fe(yard), fe(numpy)): %.3f" % worst, file=out)
