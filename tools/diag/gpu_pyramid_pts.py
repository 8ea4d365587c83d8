"""GPU diagnostic (not a pytest): what frame construction pays for its per-level feature subsets -- the loop of tsframe_pyramid_pts calls (one per text
detection and one for the scene observations: frame::TextFeaProc and tracking.cc:420) against ONE tsframe_pyramid_pts_batch call on the same inputs.
The single call is the batch of one set, so the loop pays one upload, launch and download per set where the batch call pays them once.

Frame: 640 x 480, 4 levels.  Rows: one text set alone, and 1 / 8 / 16 / 32 text sets of about 60 features each plus a scene set of 1000.  Both sides are
timed at the C ABI through ctypes on arrays prepared beforehand (no numpy work inside the clock), host clock around calls that end in a stream
synchronisation, the loop and the batch call alternating in one loop, median of --calls rounds after a warm-up.  Before a row is timed the batch
call's output is compared, byte for byte, with the loop's.  Writes the table to --out (default profiles/pyramid_pts_timing.txt).

    python tools/diag/gpu_pyramid_pts.py [--calls 300] [--out profiles/pyramid_pts_timing.txt]
For the kernels' own times and the launches per call:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/diag/gpu_pyramid_pts.py --calls 50 --out /dev/null --count-file DIR/calls.txt
    python tools/diag/gpu_pyramid_pts.py --stats-from DIR [--stats-out profiles/pyramid_pts_kernel_stats.txt]"""
import argparse
import collections
import csv
import ctypes as C
import glob
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=300)
ap.add_argument("--warmup", type=int, default=30)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pyramid_pts_timing.txt"))
ap.add_argument("--count-file", default=None, help="write the number of calls made of either kind (for the run under rocprofv3)")
ap.add_argument("--stats-from", default=None, help="directory of a rocprofv3 --kernel-trace --stats --output-format csv run of this script: write the excerpt and stop")
ap.add_argument("--stats-out", default=os.path.join(ROOT, "profiles", "pyramid_pts_kernel_stats.txt"))
args = ap.parse_args()


def stats_excerpt(d, out):
    """Per kernel of libtsframe's feature selection: launches, total and mean time, from the kernel trace of one profiled run of this script."""
    per = collections.OrderedDict()
    for f in sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                name = re.sub(r"\s*\[clone.*$", "", r["Kernel_Name"])
                per.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))/1e3)
    calls = open(os.path.join(d, "calls.txt")).read().strip() if os.path.exists(os.path.join(d, "calls.txt")) else "(calls.txt missing)"
    lines = ["rocprofv3 --kernel-trace --stats of tools/diag/gpu_pyramid_pts.py --calls 50 (a run of its own; every row's calls, warm-up and the equality check included)",
             "calls made by the script: " + calls,
             "%-64s %8s %12s %9s" % ("kernel", "calls", "total_us", "avg_us")]
    for name, t in sorted(per.items(), key=lambda kv: -sum(kv[1])):
        if name.startswith("k_pts"):
            lines.append("%-64s %8d %12.1f %9.2f" % (name[:64], len(t), sum(t), sum(t)/len(t)))
    nb = len(per.get(next((k for k in per if k.startswith("k_pts_batch")), ""), []))
    lines.append("k_pts_batch launches: %d -- one per tsframe_pyramid_pts_batch call and one per tsframe_pyramid_pts call (the batch of one set)" % nb)
    text = "\n".join(lines) + "\n"
    print(text)
    with open(out, "w") as fh:
        fh.write(text)


if args.stats_from:
    stats_excerpt(args.stats_from, args.stats_out)
    sys.exit(0)

assert args.calls >= 200 or args.out == "/dev/null", "the table wants the median of at least 200 rounds"
from textslam_amd.frame import Frame                    # noqa: E402
from textslam_amd.orbextractor import synthetic_frame   # noqa: E402

L = 4
INV = np.array([1.0, 0.5, 0.25, 0.125])
img = synthetic_frame(1)
assert img.shape == (480, 640)
fr = Frame(0)
fr.GetPyrMat(img, L)
lib, ctx = fr.lib, fr.ctx
rng = np.random.default_rng(5)
ip, dp, fp, up = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_uint8)
PINV = INV.ctypes.data_as(dp)
lines = []
n_single = n_batch = 0


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def make_sets(n_text, scene):
    sets = []
    for _ in range(n_text):
        bw, bh = rng.uniform(80, 200), rng.uniform(30, 70)
        x0, y0 = rng.uniform(5, 635 - bw), rng.uniform(5, 475 - bh)
        n = int(rng.integers(50, 71))
        xy = np.stack([rng.uniform(x0, x0 + bw, n), rng.uniform(y0, y0 + bh, n)], 1).astype(np.float32)
        sets.append((0, xy, np.array([x0, y0, x0 + bw, y0 + bh])))
    if scene:
        sets.append((1, np.stack([rng.uniform(0, 639, scene), rng.uniform(0, 479, scene)], 1).astype(np.float32), np.zeros(4)))
    return sets


class Out:
    def __init__(self, cap, rows):
        self.lo = np.zeros((rows, L + 1), np.int32); self.u = np.zeros(cap); self.v = np.zeros(cap); self.idx = np.zeros(cap, np.int32)
        self.I = np.zeros(cap); self.inn = np.zeros(cap, np.uint8)

    def ptrs(self, at=0, row=0):
        return (self.lo[row:].ctypes.data_as(ip), self.u[at:].ctypes.data_as(dp), self.v[at:].ctypes.data_as(dp), self.idx[at:].ctypes.data_as(ip),
                self.I[at:].ctypes.data_as(dp), self.inn[at:].ctypes.data_as(up))


def prepare(sets):
    ns = len(sets)
    mode = np.array([s[0] for s in sets], np.int32)
    off = np.zeros(ns + 1, np.int32); off[1:] = np.cumsum([len(s[1]) for s in sets])
    xy = np.ascontiguousarray(np.concatenate([s[1] for s in sets]))
    box = np.ascontiguousarray(np.stack([s[2] for s in sets]))
    cap = int(off[ns])*L
    a, b = Out(cap, ns), Out(cap, ns)
    # the loop: set i writes where the batch call puts set i (its base xy_off[i] * L, its level_off row), so the two results compare directly
    single = [(int(mode[i]), xy[off[i]:].ctypes.data_as(fp), int(off[i + 1] - off[i]), box[i:].ctypes.data_as(dp)) + a.ptrs(int(off[i])*L, i) for i in range(ns)]
    batch = (ns, mode.ctypes.data_as(ip), off.ctypes.data_as(ip), xy.ctypes.data_as(fp), box.ctypes.data_as(dp), PINV) + b.ptrs()
    keep = (mode, off, xy, box, a, b)
    return single, batch, keep


def run_loop(single):
    global n_single
    for m, pxy, n, pbox, lo, u, v, idx, I, inn in single:
        rc = lib.tsframe_pyramid_pts(ctx, m, pxy, n, pbox, PINV, lo, u, v, idx, I, inn)
        assert rc == 0, lib.tsframe_last_error(ctx)
    n_single += len(single)


def run_batch(batch):
    global n_batch
    rc = lib.tsframe_pyramid_pts_batch(ctx, *batch)
    assert rc == 0, lib.tsframe_last_error(ctx)
    n_batch += 1


say("per-level feature subsets of one 640 x 480 frame, 4 levels: the loop of tsframe_pyramid_pts calls vs one tsframe_pyramid_pts_batch call; C ABI through ctypes, "
    "host clock, median of %d alternating rounds (p10 .. p90), microseconds" % args.calls)
say("%-38s %5s %9s | %-30s | %-30s | %s" % ("sets", "calls", "features", "loop of single calls", "batch call", "batch / loop"))
ratios = {}
for name, n_text, scene in (("1 text set alone", 1, 0), ("1 text set + scene 1000", 1, 1000), ("8 text sets + scene 1000", 8, 1000),
                            ("16 text sets + scene 1000", 16, 1000), ("32 text sets + scene 1000", 32, 1000)):
    sets = make_sets(n_text, scene)
    single, batch, keep = prepare(sets)
    a, b = keep[4], keep[5]
    run_loop(single); run_batch(batch)
    for x, y in ((a.lo, b.lo), (a.u, b.u), (a.v, b.v), (a.idx, b.idx), (a.I, b.I), (a.inn, b.inn)):       # the same results (untouched tails are zeros on both sides)
        assert x.tobytes() == y.tobytes(), name
    assert int(b.lo[:, L].sum()) > int(keep[1][-1])                                                         # coarse levels are not empty
    t_loop, t_batch = [], []
    for it in range(args.warmup + args.calls):
        t0 = time.perf_counter(); run_loop(single); t1 = time.perf_counter(); run_batch(batch); t2 = time.perf_counter()
        if it >= args.warmup:
            t_loop.append((t1 - t0)*1e6); t_batch.append((t2 - t1)*1e6)
    q = lambda t: "%8.1f (%8.1f .. %8.1f)" % (np.median(t), np.percentile(t, 10), np.percentile(t, 90))
    ratios[name] = float(np.median(t_batch)/np.median(t_loop))
    say("%-38s %5d %9d | %-30s | %-30s | %.3f" % (name, len(sets), int(keep[1][-1]), q(t_loop), q(t_batch), ratios[name]))
say()
r1, r8 = ratios["1 text set alone"], ratios["8 text sets + scene 1000"]
say("single set: batch call / single call = %.3f (both are one k_pts_batch launch of one set: the ratio compares the two entry points' host paths)" % r1)
say("8 text sets + scene: batch call / loop of 9 calls = %.3f, the loop takes %.1f times as long -- %s (expected: several times faster than the loop)"
    % (r8, 1.0/r8, "holds" if r8 <= 1.0/3.0 else "does NOT hold"))
say("(the ctypes call overhead, about a microsecond per call, is inside both columns)")
if args.out != "/dev/null":
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
if args.count_file:
    with open(args.count_file, "w") as f:
        f.write("tsframe_pyramid_pts %d, tsframe_pyramid_pts_batch %d\n" % (n_single, n_batch))
