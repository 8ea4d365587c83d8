"""GPU diagnostic (not a pytest): what the label step behind PoseOptim / LocalBundleAdjustment costs its caller -- tsba_text_label_image (the whole image:
one workgroup paints it, 1.2 MB cross the bus, 1.2 MB are copied again into the caller's Mat) against tsba_text_label_at (the labels at the detection centres).

States: a 640 x 480 PoseOptim frame and a 20-keyframe LocalBundleAdjustment window, each with about 4 / 16 / 32 planes visible in the queried keyframe; 1 / 8 / 32
centres.  Host clock around each call (both end in a stream synchronisation), the two calls alternating in one loop, median of --calls calls after a warm-up.
Writes the table to --out (default profiles/label_at_timing.txt).  Acceptance: at 8 centres / 16 planes the new call's median is at most half the image call's.

    python tools/diag/gpu_label_at.py [--calls 300] [--out profiles/label_at_timing.txt]
For the kernels' own times run it under  rocprofv3 --kernel-trace --stats -- python tools/diag/gpu_label_at.py --calls 50 --out /dev/null  (k_label, k_label_at)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from textslam_amd import synth, abi                      # noqa: E402
from textslam_amd.optimizer import Optimizer             # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=300)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "label_at_timing.txt"))
args = ap.parse_args()
assert args.calls >= 200 or args.out == "/dev/null", "the table wants the median of at least 200 calls"

g = Optimizer(0)
rng = np.random.default_rng(1)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def states():
    for planes in (4, 16, 32):
        P = synth.make_problem(1, 300, planes, 40 + planes, feats=(8, 6, 4), frozen_frac=1.0, n_out=4, max_targets=1, text_targets=1)
        yield "PoseOptim frame", P, 0, lambda G: g.PoseOptim(G, options=abi.options_pose())
    for planes, n_text in ((4, 16), (16, 64), (32, 128)):
        P = synth.make_problem(20, 1500, n_text, 50 + planes, feats=(16, 8, 6))
        cnt = np.bincount(P.tobs_kf, minlength=P.n_kf)
        kf = int(np.argmin(np.abs(cnt - planes)))
        yield "LocalBA window (20 KF, %d planes)" % n_text, P, kf, lambda G: g.LocalBundleAdjustment(G, options=abi.options_local())


say("label step: tsba_text_label_image vs tsba_text_label_at, level 0 (640 x 480), host clock around the call, median of %d alternating calls (p10 .. p90), microseconds" % args.calls)
say("%-36s %7s %8s | %-28s | %-28s | %s" % ("state", "planes", "centres", "label_image", "label_at", "label_at / label_image"))
accept = None
for name, P, kf, solve in states():
    G = P.copy()
    solve(G)
    h, w = int(P.img[0].shape[1]), int(P.img[0].shape[2])
    planes = int((np.asarray(P.tobs_kf) == kf).sum())
    img = g.TextLabelImage(kf, 0, (h, w))
    ys, xs = np.nonzero(img >= 0)
    for n in (1, 8, 32):
        pick = rng.integers(0, len(ys), n)
        px = np.stack([xs[pick], ys[pick]], 1).astype(np.int32)
        kfs = np.full(n, kf, np.int32)
        assert np.array_equal(g.TextLabelAt(0, kfs, px).astype(np.float32), img[px[:, 1], px[:, 0]])     # the same labels
        t_img, t_at = [], []
        for it in range(args.warmup + args.calls):
            t0 = time.perf_counter(); g.TextLabelImage(kf, 0, (h, w)); t1 = time.perf_counter(); g.TextLabelAt(0, kfs, px); t2 = time.perf_counter()
            if it >= args.warmup:
                t_img.append((t1 - t0)*1e6); t_at.append((t2 - t1)*1e6)
        q = lambda t: "%8.1f (%7.1f .. %7.1f)" % (np.median(t), np.percentile(t, 10), np.percentile(t, 90))
        ratio = float(np.median(t_at)/np.median(t_img))
        say("%-36s %7d %8d | %-28s | %-28s | %.3f" % (name, planes, n, q(t_img), q(t_at), ratio))
        if n == 8 and abs(planes - 16) <= 4 and name.startswith("PoseOptim"):
            accept = ratio
say()
if accept is None:
    say("acceptance (8 centres / 16 planes, PoseOptim frame): no such row")
else:
    say("acceptance (8 centres / 16 planes, PoseOptim frame): label_at / label_image = %.3f -- %s (at most 0.5 asked)" % (accept, "met" if accept <= 0.5 else "NOT met: no gain claimed"))
say("(Python call overhead -- ctypes, numpy allocation of the output -- is inside both columns; the image call's includes allocating its 1.2 MB result.)")
if args.out != "/dev/null":
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
