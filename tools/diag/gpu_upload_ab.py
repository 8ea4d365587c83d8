"""Cold-call figures of the upload path for A/B runs of two builds (run once per build in a fresh process, alternating): the one-shot tsba_local_ba call on the
C4 window and the one-shot tsba_pose_optim call on C3, context warm, as bench.py --full times them -- wall time through the Python mirror and the library's own
upload / solve clocks -- every repetition listed.  --dump DIR writes what the last call of each computed as DIR/<name>.npy."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from textslam_amd import synth, abi                                    # noqa: E402
from textslam_amd.optimizer import Optimizer                           # noqa: E402

FIELDS = ("pose", "rho", "theta", "sgood", "tobs_good", "tfgood")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--dump", default=None)
    args = ap.parse_args()
    g = Optimizer(0)
    out = {}
    for name, P, o, call in (("c4_local_ba", synth.config_c4(), abi.options_local(), "LocalBundleAdjustment"), ("c3_pose_optim", synth.config_c3(), abi.options_pose(), "PoseOptim")):
        q = P.copy(); getattr(g, call)(q, options=o)                     # (the context's first call: slabs, attributes)
        wall, up, solve = [], [], []
        for _ in range(args.reps):
            q = P.copy(); t0 = time.perf_counter(); r = getattr(g, call)(q, options=o); wall.append((time.perf_counter() - t0)*1e3)
            up.append(r["t_upload_ms"]); solve.append(r["t_solve_ms"])
        out[name] = {"call_ms": wall, "upload_plan_ms": up, "solve_ms": solve, "iters": r["iters"], "solver_info": g.solver_info()}
        if args.dump:
            os.makedirs(args.dump, exist_ok=True)
            for f in FIELDS:
                np.save(os.path.join(args.dump, "%s_%s.npy" % (name, f)), np.asarray(getattr(q, f)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
