"""One one-shot call on a fresh context, for a profiler to count what it launches and copies: `local` = tsba_local_ba on the C4 window, `pose` = tsba_pose_optim on C3
(rocprofv3 --kernel-trace --memory-copy-trace -- python tools/diag/gpu_one_shot_call.py local; tools/diag/rocprof_counts.py sums the traces up)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from textslam_amd import synth, abi                                    # noqa: E402
from textslam_amd.optimizer import Optimizer                           # noqa: E402

kind = sys.argv[1] if len(sys.argv) > 1 else "local"
g = Optimizer(0)
if kind == "local":
    P = synth.config_c4(); rep = g.LocalBundleAdjustment(P, options=abi.options_local())
else:
    P = synth.config_c3(); rep = g.PoseOptim(P, options=abi.options_pose())
print(kind, rep["iters"], rep["cost1"])
g.close()
