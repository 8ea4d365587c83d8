"""GPU diagnostic (not a pytest): what tracking::CheckMatch's PnP RANSAC costs per frame -- tsorb_match_pnp_ransac for n = 100 / 300 / 1000 / 3000 matches (30 % outliers,
0.5 px noise, 5 px threshold) at 100 hypotheses, copies included, timed through the raw C call (host clock around a call that ends in a stream synchronisation: the median
after a warm-up with its 10th and 90th percentiles).  Beside it the only host baseline there is without OpenCV: tests/cxx/pnp_host.hip, a single-thread -O2 build of the
SAME __host__ __device__ functions (textslam_amd/csrc/tspnp.h) running the reference's loop WITH its early stop (a hypothesis is formed and counted only when the loop
reaches it) on the same worlds, on the same machine.  It is not OpenCV's EPnP: the Jacobi eigen-solve stands where OpenCV calls its SVD.  Every shape is reported.

    python tools/diag/gpu_pnp_ransac.py [--calls 500] [--out profiles/pnp_ransac_timing.txt]
    python tools/diag/gpu_pnp_ransac.py --stats [--stats-out profiles/pnp_ransac_kernel_stats.txt]     the device calls alone under rocprofv3 --kernel-trace --stats
    python tools/diag/gpu_pnp_ransac.py --build-only                                                   compile the host program (tools/bin/pnp_host_o2) and stop"""
import argparse
import ctypes as C
import glob
import os
import re
import struct
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=500)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pnp_ransac_timing.txt"))
ap.add_argument("--stats", action="store_true")
ap.add_argument("--stats-out", default=os.path.join(ROOT, "profiles", "pnp_ransac_kernel_stats.txt"))
ap.add_argument("--build-only", action="store_true")
ap.add_argument("--device-only", action="store_true")
args = ap.parse_args()
SIZES = (100, 300, 1000, 3000)
HOST = os.path.join(ROOT, "tools", "bin", "pnp_host_o2")
SRC = os.path.join(ROOT, "tests", "cxx", "pnp_host.hip")


def build_host():
    deps = [SRC, os.path.join(ROOT, "textslam_amd", "csrc", "tspnp.h"), os.path.join(ROOT, "textslam_amd", "csrc", "tsjacobi.h"), os.path.join(ROOT, "include", "tsorb.h")]
    if not os.path.exists(HOST) or any(os.path.getmtime(d) > os.path.getmtime(HOST) for d in deps):
        os.makedirs(os.path.dirname(HOST), exist_ok=True)
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O2", "-ffp-contract=off", "-o", HOST, SRC])


if args.build_only:
    build_host(); sys.exit(0)

if args.stats:
    with tempfile.TemporaryDirectory() as tmp:
        prof = os.path.join(tmp, "prof")
        res = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", prof, "-o", "pnp_ransac", "--", sys.executable, os.path.abspath(__file__), "--device-only",
                              "--calls", str(args.calls), "--out", os.path.join(tmp, "timing.txt")], capture_output=True, text=True, timeout=500)
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
            f.write("rocprofv3 --kernel-trace --stats of tools/diag/gpu_pnp_ransac.py --device-only --calls %d (n = %s matches x 100 hypotheses; %d + 20 calls per shape)\n"
                    % (args.calls, " / ".join(str(n) for n in SIZES), args.calls) + top.stdout)
    sys.exit(0)

import numpy as np                                                     # noqa: E402
import pnp_ransac_ref as R                                            # noqa: E402
from textslam_amd.orbextractor import ORBextractor                    # noqa: E402

if not args.device_only:
    build_host()
ex = ORBextractor()
F32, F64, I32, U8 = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
lines = ["# per call, copies included; device = the median of %d calls after 20 warm-up calls with their 10th and 90th percentiles (all 100 hypotheses evaluated, three launches);" % args.calls,
         "# host = one thread, hipcc -O2 host build of the same functions, the reference's loop with its early stop (n_run hypotheses formed and counted), mean of the runs of 0.5 s or more",
         "# n x hypotheses      device_ms (p10 - p90)         host_ms (early stop, n_run)      host/device     (inliers, sel)"]
with tempfile.TemporaryDirectory() as tmp:
    for n in SIZES:
        w = R.world(0, n, 0.3, 0.5, 100)
        Pw, uv, K, sub = w["Pw"], w["uv"], w["K"], np.ascontiguousarray(w["subsets"], np.int32)
        inl = np.zeros(n, np.uint8); res = np.zeros(4, np.int32); pose = np.zeros(12); hc = np.zeros(100, np.int32)
        a = (ex.ctx, n, Pw.ctypes.data_as(F32), uv.ctypes.data_as(F32), K.ctypes.data_as(F64), 100, sub.ctypes.data_as(I32), 5.0, 0.98,
             inl.ctypes.data_as(U8), res.ctypes.data_as(I32), pose.ctypes.data_as(F64), hc.ctypes.data_as(I32), None)
        fn = ex.lib.tsorb_match_pnp_ransac
        for _ in range(20):
            assert fn(*a) == 0
        ts = []
        for _ in range(args.calls):
            t0 = time.perf_counter(); fn(*a); ts.append((time.perf_counter() - t0)*1e3)
        ts.sort(); dev = ts[len(ts)//2]; p10, p90 = ts[len(ts)//10], ts[(9*len(ts))//10]
        host_txt, ratio = "not run", ""
        if not args.device_only:
            inp, outp = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
            with open(inp, "wb") as f:
                f.write(struct.pack("<ii", n, 100)); f.write(K.tobytes()); f.write(struct.pack("<dd", 5.0, 0.98)); f.write(Pw.tobytes()); f.write(uv.tobytes()); f.write(sub.tobytes())
            reps = 20
            while True:
                r = subprocess.run([HOST, inp, outp, str(reps)], capture_output=True, text=True, timeout=300)
                if r.returncode != 0:
                    sys.stderr.write(r.stdout + r.stderr); sys.exit(r.returncode)
                m = re.search(r"early_stop_ms ([0-9.]+) n_run (\d+)", r.stdout)
                ms, n_run = float(m.group(1)), int(m.group(2))
                if ms*reps >= 500.0 or reps >= 20000:
                    break
                reps = int(reps*max(2.0, 600.0/max(ms*reps, 1e-3)))
            raw = open(outp, "rb").read()
            same = np.array_equal(np.frombuffer(raw, np.int32, 100, 9600), hc) and np.array_equal(np.frombuffer(raw, np.int32, 4, 10000), res) and n_run == res[3]
            host_txt = "%8.3f (n_run %d, %d runs)" % (ms, n_run, reps) + ("" if same else "  [host and device decisions differ on this world]"); ratio = "%8.1f" % (ms/dev)
        line = "%5d x 100          %8.3f (%.3f - %.3f)        %s    %s     (%d, %d)" % (n, dev, p10, p90, host_txt, ratio, res[1], res[2])
        print(line); lines.append(line)
with open(args.out, "w") as f:
    f.write("tracking::CheckMatch's PnP RANSAC in one call (tools/diag/gpu_pnp_ransac.py); milliseconds\n" + "\n".join(lines) + "\n")
