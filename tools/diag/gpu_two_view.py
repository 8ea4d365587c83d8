"""GPU diagnostic (not a pytest): what the two-view initializer's H / F RANSAC costs per frame -- tsorb_match_two_view_ransac for n = 100 / 300 / 1000 / 3000 matches (30 %
outliers, 0.5 px noise, a 640 x 480 image) at 200 hypotheses (2 x 200 fits, 2 x 200 scorings over all matches), copies included, timed through the raw C call (host clock
around a call that ends in a stream synchronisation: the median after a warm-up with its 10th and 90th percentiles).  Beside it the only host baseline there is without
OpenCV: tests/cxx/two_view_host.hip, a single-thread -O2 build of the SAME __host__ __device__ functions (textslam_amd/csrc/tstwoview.h) running the same loop (the
reference has no early stop: all 400 models are fitted and scored) on the same worlds, on the same machine.  It is NOT OpenCV's float cv::SVDecomp: a one-sided Jacobi
iteration in fp64 stands where OpenCV runs its float SVD.  Every shape is reported.

    python tools/diag/gpu_two_view.py [--calls 300] [--out profiles/two_view_timing.txt]
    python tools/diag/gpu_two_view.py --stats [--stats-out profiles/two_view_kernel_stats.txt]     the device calls alone under rocprofv3 --kernel-trace --stats
    python tools/diag/gpu_two_view.py --build-only                                                 compile the host program (tools/bin/two_view_host_o2) and stop"""
import argparse
import ctypes as C
import glob
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=300)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_view_timing.txt"))
ap.add_argument("--stats", action="store_true")
ap.add_argument("--stats-out", default=os.path.join(ROOT, "profiles", "two_view_kernel_stats.txt"))
ap.add_argument("--build-only", action="store_true")
ap.add_argument("--device-only", action="store_true")
ap.add_argument("--sizes", default="100,300,1000,3000", help="the match counts, comma-separated")
args = ap.parse_args()
SIZES = tuple(int(x) for x in args.sizes.split(","))
NHYP = 200
HOST = os.path.join(ROOT, "tools", "bin", "two_view_host_o2")
SRC = os.path.join(ROOT, "tests", "cxx", "two_view_host.hip")

import two_view_io as IO                                              # noqa: E402


def build_host():
    deps = [SRC, os.path.join(ROOT, "textslam_amd", "csrc", "tstwoview.h"), os.path.join(ROOT, "textslam_amd", "csrc", "tsjacobi.h"), os.path.join(ROOT, "include", "tsorb.h")]
    if not os.path.exists(HOST) or any(os.path.getmtime(d) > os.path.getmtime(HOST) for d in deps):
        os.makedirs(os.path.dirname(HOST), exist_ok=True)
        IO.build_host(HOST, sanitize=False)


if args.build_only:
    build_host(); sys.exit(0)

if args.stats:                                                         # one profiled run per match count: a kernel's mean is then that shape's
    out = ["rocprofv3 --kernel-trace --stats of tools/diag/gpu_two_view.py --device-only --calls %d --sizes <n>, one run per n (%d hypotheses; %d + 20 calls each)" % (args.calls, NHYP, args.calls)]
    with tempfile.TemporaryDirectory() as tmp:
        for n in SIZES:
            prof = os.path.join(tmp, "prof%d" % n)
            res = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", prof, "-o", "two_view", "--", sys.executable, os.path.abspath(__file__), "--device-only",
                                  "--sizes", str(n), "--calls", str(args.calls), "--out", os.path.join(tmp, "timing.txt")], capture_output=True, text=True, timeout=300)
            if res.returncode != 0:
                sys.stderr.write(res.stdout + res.stderr); sys.exit(res.returncode)
            dbs = glob.glob(os.path.join(prof, "**", "*.db"), recursive=True)
            if not dbs:
                sys.stderr.write("no rocprofv3 database written\n" + res.stderr); sys.exit(1)
            top = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "rocpd_top_kernels.py"), dbs[0]], capture_output=True, text=True, timeout=120)
            sys.stderr.write(top.stderr)
            if top.returncode != 0:
                sys.exit(top.returncode)
            out.append("n = %d matches\n" % n + top.stdout.rstrip())
    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    with open(args.stats_out, "w") as f:
        f.write(text)
    sys.exit(0)

import numpy as np                                                     # noqa: E402
import two_view_ref as R                                              # noqa: E402
from textslam_amd.orbextractor import ORBextractor                    # noqa: E402

if not args.device_only:
    build_host()
ex = ORBextractor()
F32, I32, U8 = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
lines = ["# per call, copies included; device = the median of %d calls after 20 warm-up calls with their 10th and 90th percentiles (2 x %d fits, 2 x %d scorings, three launches);" % (args.calls, NHYP, NHYP),
         "# host = one thread, hipcc -O2 host build of the same functions, the same loop (no early stop in the reference), mean of the runs of 0.5 s or more; fit + score = its two parts",
         "# n x hypotheses      device_ms (p10 - p90)         host_ms (fit + score)                  host/device     (sel H, sel F, RH)"]
with tempfile.TemporaryDirectory() as tmp:
    for n in SIZES:
        g = np.random.default_rng(n)
        w = R.world("general", 0, n, 0.3, 1, K=(520.0, 520.0, 320.0, 240.0), w=640, h=480)
        w["subsets"] = np.stack([g.choice(n, 8, replace=False) for _ in range(NHYP)]).astype(np.int32)      # drawn as the reference draws: no condition on a subset
        xy1, xy2, n1, n2, sub = w["xy1"], w["xy2"], w["norm1"], w["norm2"], w["subsets"]
        ih = np.zeros(n, np.uint8); jf = np.zeros(n, np.uint8); H21 = np.zeros(9, np.float32); F21 = np.zeros(9, np.float32); sc = np.zeros(2, np.float32); sel = np.zeros(2, np.int32)
        a = (ex.ctx, n, xy1.ctypes.data_as(F32), xy2.ctypes.data_as(F32), n1.ctypes.data_as(F32), n2.ctypes.data_as(F32), NHYP, sub.ctypes.data_as(I32), 1.0,
             ih.ctypes.data_as(U8), jf.ctypes.data_as(U8), H21.ctypes.data_as(F32), F21.ctypes.data_as(F32), sc.ctypes.data_as(F32), sel.ctypes.data_as(I32), None, None)
        fn = ex.lib.tsorb_match_two_view_ransac
        for _ in range(20):
            assert fn(*a) == 0
        ts = []
        for _ in range(args.calls):
            t0 = time.perf_counter(); fn(*a); ts.append((time.perf_counter() - t0)*1e3)
        ts.sort(); dev = ts[len(ts)//2]; p10, p90 = ts[len(ts)//10], ts[(9*len(ts))//10]
        host_txt, ratio = "not run", ""
        if not args.device_only:
            inp, outp = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
            IO.write_host(inp, w)
            reps = 5
            while True:
                r = subprocess.run([HOST, inp, outp, str(reps)], capture_output=True, text=True, timeout=300)
                if r.returncode != 0:
                    sys.stderr.write(r.stdout + r.stderr); sys.exit(r.returncode)
                m = re.search(r"loop_ms ([0-9.]+) fit_ms ([0-9.]+) score_ms ([0-9.]+)", r.stdout)
                ms, fit_ms, score_ms = float(m.group(1)), float(m.group(2)), float(m.group(3))
                if ms*reps >= 500.0 or reps >= 20000:
                    break
                reps = int(reps*max(2.0, 600.0/max(ms*reps, 1e-3)))
            o = IO.read_host(outp, n, NHYP)
            same = o["sel"].tolist() == sel.tolist() and o["score"].tobytes() == sc.tobytes() and np.array_equal(o["inlier_h"], ih.astype(bool)) and np.array_equal(o["inlier_f"], jf.astype(bool))
            host_txt = "%8.3f (%.3f + %.3f, %d runs)" % (ms, fit_ms, score_ms, reps) + ("" if same else "  [host and device results differ on this world]"); ratio = "%8.1f" % (ms/dev)
        with np.errstate(invalid="ignore", divide="ignore"):
            rh = float(sc[0]/np.float32(sc[0] + sc[1]))
        line = "%5d x %d          %8.3f (%.3f - %.3f)        %s    %s     (%d, %d, %.3f)" % (n, NHYP, dev, p10, p90, host_txt, ratio, sel[0], sel[1], rh)
        print(line); lines.append(line)
with open(args.out, "w") as f:
    f.write("the two-view initializer's H / F RANSAC in one call (tools/diag/gpu_two_view.py); milliseconds\n" + "\n".join(lines) + "\n")
