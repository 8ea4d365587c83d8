"""GPU diagnostic (not a pytest): what loop closing pays for step 3 of ComputeSim3 -- one tsloop_sim3_batch call (RANSAC + LM of every candidate, copies
included) for 1 / 4 / 8 candidates of 300 matches and 8 of 1500, beside, in the same process, the loop of n_cand tsloop_optimize_sim3 calls on the same slices
from the same starts (the device side of step 3 before the batch call existed: it leaves the host RANSAC out, which favours it) and the numpy restatement's
time for the RANSAC (for scale only).  Host clock around calls that end in a stream synchronisation; the median after a warm-up.

    python tools/diag/gpu_sim3_batch.py [--calls 50] [--out profiles/sim3_batch_timing.txt]
    python tools/diag/gpu_sim3_batch.py --stats [--stats-out profiles/sim3_batch_kernel_stats.txt]     the same workload under rocprofv3 --kernel-trace --stats"""
import argparse
import ctypes as C
import glob
import os
import subprocess
import sys
import tempfile
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3_batch_timing.txt"))
ap.add_argument("--stats", action="store_true")
ap.add_argument("--stats-out", default=os.path.join(ROOT, "profiles", "sim3_batch_kernel_stats.txt"))
args = ap.parse_args()


def measure():
    import sim3_ransac_ref as S
    from textslam_amd import loop
    lo = loop.LoopOptimizer(0)
    o = lo.default_options_sim3()
    med = lambda v: float(np.median(v))
    lines = ["# per call, copies included; median of %d calls after a warm-up of 3; single = the loop of n_cand tsloop_optimize_sim3 calls from the batch's own" % args.calls,
             "# selections (no RANSAC in it); numpy = the restatement's RANSAC on the CPU, for scale",
             "# shape                          batch_ms   single_loop_ms   single/batch   numpy_ransac_ms   (ok candidates, LM inliers)"]
    for n_cand, n, bad3d in ((1, 300, 0.3), (4, 300, 0.3), (8, 300, 0.3), (8, 1500, 0.4)):
        worlds = []; seed = 1
        while len(worlds) < n_cand:                                    # candidates the RANSAC accepts, so that every LM runs
            w = S.world(seed, n, bad3d); seed += 1
            if S.run_world(w)["ok"]:
                worlds.append(w)
        cands = [{"P1": w["P1"], "P2": w["P2"], "pred1": w["pred1"], "pred2": w["pred2"], "uv1": w["uv1"], "uv2": w["uv2"], "triples": w["triples"], "K2": w["K2"]} for w in worlds]
        K1, K = worlds[0]["K1"], worlds[0]["K"]
        start = lo.Sim3Batch(cands, K1, K, optimise=False)
        p, A = loop.make_sim3_batch_problem(cands, K1, K, True)
        tb = []
        for it in range(args.calls + 3):
            t0 = time.perf_counter(); rc = lo.lib.tsloop_sim3_batch(lo.ctx, C.byref(p), C.byref(o)); t1 = time.perf_counter()
            assert rc == 0
            if it >= 3:
                tb.append((t1 - t0)*1e3)
        n_ok = int(A["ok"].sum()); n_lm = [int(A["rep"][k].n_inlier) for k in range(n_cand)]
        singles = [loop.make_sim3_problem(w["P1"], w["P2"], w["uv1"], w["uv2"], s["inlier"].astype(np.uint8), s["sim_ransac"], K) for w, s in zip(worlds, start)]
        ts = []; rep = loop.TsloopReport()
        for it in range(args.calls + 3):
            for (sp, keep, inl), s in zip(singles, start):             # in / out arguments back to the start
                inl[:] = s["inlier"]
                for k in range(8):
                    sp.sim[k] = float(s["sim_ransac"][k])
            t0 = time.perf_counter()
            for sp, keep, inl in singles:
                rc = lo.lib.tsloop_optimize_sim3(lo.ctx, C.byref(sp), C.byref(o), C.byref(rep))
            t1 = time.perf_counter()
            assert rc == 0
            if it >= 3:
                ts.append((t1 - t0)*1e3)
        assert [int(inl.sum()) for sp, keep, inl in singles] == n_lm  # the same answers both ways
        tn = []
        for it in range(5):
            t0 = time.perf_counter()
            for w in worlds:
                S.run_world(w)
            tn.append((time.perf_counter() - t0)*1e3)
        lines.append("%d candidate(s) of %4d matches   %9.3f   %14.3f   %12.2f   %15.3f   (%d ok, LM inliers %s)"
                     % (n_cand, n, med(tb), med(ts), med(ts)/med(tb), med(tn), n_ok, " ".join(map(str, n_lm))))
    return "\n".join(lines) + "\n"


if not args.stats:
    table = measure()
    sys.stdout.write(table)
    with open(args.out, "w") as f:
        f.write("loopClosing::ComputeSim3 step 3: tsloop_sim3_batch beside the loop of tsloop_optimize_sim3 calls (tools/diag/gpu_sim3_batch.py); milliseconds\n" + table)
else:
    with tempfile.TemporaryDirectory() as tmp:
        prof = os.path.join(tmp, "prof")
        res = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", prof, "-o", "sim3_batch", "--", sys.executable, os.path.abspath(__file__),
                              "--calls", str(args.calls), "--out", os.path.join(tmp, "timing.txt")], capture_output=True, text=True, timeout=400)
        if res.returncode != 0:
            sys.stderr.write(res.stdout + res.stderr); sys.exit(res.returncode)
        dbs = glob.glob(os.path.join(prof, "**", "*.db"), recursive=True)
        if not dbs:
            sys.stderr.write("no rocprofv3 database written\n" + res.stderr); sys.exit(1)
        top = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "rocpd_top_kernels.py"), dbs[0]], capture_output=True, text=True, timeout=120)
        sys.stdout.write(top.stdout); sys.stderr.write(top.stderr)
        if top.returncode != 0:
            sys.exit(top.returncode)
        with open(args.stats_out, "w") as f:
            f.write("rocprofv3 --kernel-trace --stats of tools/diag/gpu_sim3_batch.py --calls %d (1 / 4 / 8 candidates of 300 matches, 8 of 1500: %d + 4 batch calls each, "
                    "and n_cand single calls per round)\n" % (args.calls, args.calls) + top.stdout)
