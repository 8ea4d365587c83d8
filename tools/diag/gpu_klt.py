"""GPU diagnostic (not a pytest): tsframe_klt_track (tracking::TrackNewTextFeat's cv::calcOpticalFlowPyrLK for all points of a frame, one launch)
per call, both copies included, for 64 / 256 / 1024 points on a 640 x 480 pair (tests/klt_ref.py: shift (3.3, -2.6), strongest-gradient grid
points, tiled with sub-pixel offsets).  20 warm-up calls, median of 200, in ms; 'raw' = the C call through prebuilt ctypes arguments, 'py' =
Frame.TrackKLT.  Beside it the CPU time of the restatement (tests/klt_ref.py: a numpy restatement of docs/klt_recalled.md, NOT OpenCV) for the
same calls, with the pyramids and derivative planes already built.

  python tools/diag/gpu_klt.py [out.txt]       timing table (also written to out.txt)
  KLT_ONLY_CALLS=N python tools/diag/gpu_klt.py  only N calls of 256 points (the workload for rocprofv3 --kernel-trace --stats)"""
import ctypes as C
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from textslam_amd import frame                             # noqa: E402
import klt_ref as R                                        # noqa: E402

REPS = int(os.environ.get("KLT_REPS", "200"))
ONLY = int(os.environ.get("KLT_ONLY_CALLS", "0"))
name, M, t = R.PAIRS[0]
A, B = R.pair(M, t)
base = R.interior_points(A)
fa, fb = frame.Frame(0), frame.Frame(0)
fa.GetPyrMat(A, 4); fb.GetPyrMat(B, 4)
fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
rng = np.random.default_rng(11)


def points(n):
    reps = -(-n//len(base))
    p = np.concatenate([base + rng.uniform(-1.5, 1.5, base.shape).astype(np.float32) for _ in range(reps)])[:n]
    return np.ascontiguousarray(p, np.float32)


lines = []


def say(s):
    print(s); lines.append(s)


if ONLY:
    p = points(256); nxt = np.zeros_like(p); st = np.zeros(len(p), np.uint8)
    for _ in range(ONLY):
        assert fb.lib.tsframe_klt_track(fa.ctx, fb.ctx, len(p), p.ctypes.data_as(fp), 21, 3, 30, 0.01, 1e-4, nxt.ctypes.data_as(fp), st.ctypes.data_as(up)) == 0
    print("ran", ONLY, "calls of 256 points; tracked", int(st.sum()))
    sys.exit(0)

say(f"tsframe_klt_track, pair {name} 640 x 480, win 21, max_level 3, 30 iterations, eps 0.01; 20 warm-up calls, median of {REPS}")
pI, pJ = R.build_pyramid(A), R.build_pyramid(B); der = [R.scharr(x) for x in pI]
for n in (64, 256, 1024):
    p = points(n); nxt = np.zeros_like(p); st = np.zeros(n, np.uint8)
    args = (fa.ctx, fb.ctx, n, p.ctypes.data_as(fp), 21, 3, 30, 0.01, 1e-4, nxt.ctypes.data_as(fp), st.ctypes.data_as(up))
    f = fb.lib.tsframe_klt_track
    for _ in range(20):
        assert f(*args) == 0
    tr = []
    for _ in range(REPS):
        t0 = time.perf_counter(); f(*args); tr.append((time.perf_counter() - t0)*1e3)
    tp = []
    for _ in range(max(REPS//4, 10)):
        t0 = time.perf_counter(); fb.TrackKLT(fa, p); tp.append((time.perf_counter() - t0)*1e3)
    t0 = time.perf_counter(); ref_xy, ref_st, info = R.track(pI, pJ, p, der=der); t_cpu = (time.perf_counter() - t0)*1e3
    same = bool(np.array_equal(ref_xy.view(np.uint32), nxt.view(np.uint32)) and np.array_equal(ref_st, st))
    truth = p.astype(np.float64) @ np.asarray(M).T + np.asarray(t)
    err = np.hypot(*(nxt - truth).T)
    its = sum(e[2] for i in info for e in i)/n
    say(f"n={n:5d}  raw {np.median(tr):.4f} ms (p10 {np.percentile(tr, 10):.4f}, p90 {np.percentile(tr, 90):.4f})   py {np.median(tp):.4f} ms   "
        f"restatement on the CPU (numpy, not OpenCV) {t_cpu:.0f} ms   bit-equal to it: {same}   status 1: {int(st.sum())}/{n}   "
        f"within 0.5 px of the warp: {int(((err < 0.5) & (st == 1)).sum())}   iterations per point (all levels): {its:.1f}")
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
