"""GPU diagnostic (not a pytest): tsba_theta_optim_batch against N calls of tsba_theta_optim on the same single-plane problems
(tracking::TextUpdate's immature planes of one frame).  For N in {1, 4, 16, 64}: median of warm calls, in ms per call."""
import os
import sys
import time
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from textslam_amd import synth, abi                      # noqa: E402
from textslam_amd.optimizer import Optimizer             # noqa: E402

REPS = int(os.environ.get("THETA_BATCH_REPS", "25"))
g = Optimizer(0)
o = abi.options_theta()
pool = synth.theta_planes(seed=3, n=64)
print(f"library {os.environ.get('TSBA_LIB', 'textslam_amd/libtsba.so')}; {REPS} warm calls per figure (median)")
for N in (1, 4, 16, 64):
    probs = pool[:N]
    works = [[P.copy() for P in probs] for _ in range(REPS + 2)]
    tb, parts = [], []
    for k, w in enumerate(works):
        t0 = time.perf_counter(); reps, _ = g.ThetaOptimMultiFsBatch(w, options=o); t1 = time.perf_counter()
        if k >= 2:
            tb.append((t1 - t0) * 1e3); parts.append((reps[0]["t_upload_ms"], reps[0]["t_solve_ms"], reps[0]["t_download_ms"]))
    ts = []
    for k in range(REPS + 2):
        w = [P.copy() for P in probs]
        t0 = time.perf_counter()
        for P in w:
            g.ThetaOptimMultiFs(P, text=0, options=o)
        t1 = time.perf_counter()
        if k >= 2:
            ts.append((t1 - t0) * 1e3)
    its = sum(sum(r["iters"]) for r in reps)
    up, sv, dn = np.median(np.array(parts), axis=0)
    print(f"N={N:3d}  batch {np.median(tb):7.3f} ms  (upload {up:.3f} / kernel+sync {sv:.3f} / download {dn:.3f})   "
          f"{N} x tsba_theta_optim {np.median(ts):8.3f} ms   LM iterations in the batch {its}")
