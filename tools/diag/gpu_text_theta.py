"""GPU diagnostic (not a pytest): what the planes of a keyframe's new text detections cost -- tsorb_match_text_theta_ransac for 1 / 8 / 16 planes of 20 / 60 / 200
features and 200 hypotheses each, triangulation on the device, copies included, timed through the raw C call with the optional outputs NULL, as the adapter calls it
(host clock around a call that ends in a stream synchronisation: the median after a warm-up with its 10th and 90th percentiles).  Beside it the only host baseline
there is without OpenCV: tests/cxx/text_theta_host.hip, a single-thread -O2 build of the SAME __host__ __device__ functions (textslam_amd/csrc/tstexttheta.h) running
the reference's loop on the same worlds, on the same machine.  It is NOT OpenCV's cv::triangulatePoints: a one-sided Jacobi iteration in fp64 stands where OpenCV runs
its SVD of each 4 x 4; the 200 x n plane transfers are the reference's own arithmetic.  Every shape is reported.

    python tools/diag/gpu_text_theta.py [--calls 300] [--out profiles/text_theta_timing.txt]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/diag/gpu_text_theta.py --device-only --planes 8 --sizes 60      the device calls alone, as a profiler's workload
    python tools/diag/gpu_text_theta.py --build-only                                                                         compile the host program and stop"""
import argparse
import ctypes as C
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_theta_timing.txt"))
ap.add_argument("--build-only", action="store_true")
ap.add_argument("--device-only", action="store_true")
ap.add_argument("--planes", default="1,8,16", help="the plane counts, comma-separated")
ap.add_argument("--sizes", default="20,60,200", help="the features per plane, comma-separated")
ap.add_argument("--hyp", type=int, default=200)
args = ap.parse_args()
PLANES = tuple(int(x) for x in args.planes.split(",")); SIZES = tuple(int(x) for x in args.sizes.split(","))
HOST = os.path.join(ROOT, "tools", "bin", "text_theta_host_o2")
SRC = os.path.join(ROOT, "tests", "cxx", "text_theta_host.hip")

import text_theta_io as IO                                            # noqa: E402


def build_host():
    deps = [SRC, os.path.join(ROOT, "include", "tsorb.h")] + [os.path.join(ROOT, "textslam_amd", "csrc", h) for h in ("tstexttheta.h", "tsjacobi.h")]
    if not os.path.exists(HOST) or any(os.path.getmtime(d) > os.path.getmtime(HOST) for d in deps):
        os.makedirs(os.path.dirname(HOST), exist_ok=True)
        IO.build_host(HOST, sanitize=False)


if args.build_only:
    build_host(); sys.exit(0)

import numpy as np                                                     # noqa: E402
import text_theta_ref as R                                            # noqa: E402
from textslam_amd.orbextractor import ORBextractor                    # noqa: E402

if not args.device_only:
    build_host()
ex = ORBextractor()
F32, F64, I32 = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)
lines = ["# per call, copies included, p3d / rho_out / hyp_* NULL; device = the median of %d calls after 20 warm-up calls with their 10th and 90th percentiles (three launches);" % args.calls,
         "# host = one thread, hipcc -O2 host build of the same functions running the reference's loop, mean of the runs of 0.5 s or more; %d hypotheses per plane" % args.hyp,
         "# planes  features     device_ms (p10 - p90)         host_ms                      host/device     kept (of the planes)"]
with tempfile.TemporaryDirectory() as tmp:
    for P in PLANES:
        for n in SIZES:
            w = R.batch_world(100 + P + n, [n]*P, [args.hyp]*P)
            off = np.asarray(w["off"], np.int32); hoff = np.asarray(w["hyp_off"], np.int32); hxy = np.ascontiguousarray(w["host_xy"], np.float32)
            txy = np.ascontiguousarray(w["targ_xy"], np.float32); T = np.ascontiguousarray(w["Tcr"], np.float64).reshape(12); K = np.asarray(w["K"], np.float64)
            tri = np.ascontiguousarray(w["triple"], np.int32); sel = np.zeros(P, np.int32); theta = np.zeros((P, 3)); score = np.zeros(P)
            a = (ex.ctx, P, off.ctypes.data_as(I32), hxy.ctypes.data_as(F32), txy.ctypes.data_as(F32), None, T.ctypes.data_as(F64), K.ctypes.data_as(F64), hoff.ctypes.data_as(I32),
                 tri.ctypes.data_as(I32), sel.ctypes.data_as(I32), theta.ctypes.data_as(F64), score.ctypes.data_as(F64), None, None, None, None)
            fn = ex.lib.tsorb_match_text_theta_ransac
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
                    ms = float(re.search(r"loop_ms ([0-9.]+)", r.stdout).group(1))
                    if ms*reps >= 500.0 or reps >= 20000:
                        break
                    reps = int(reps*max(2.0, 600.0/max(ms*reps, 1e-3)))
                o = IO.read_host(outp, w)
                same = o["sel"].tolist() == sel.tolist() and o["theta"].tobytes() == theta.tobytes() and o["score"].tobytes() == score.tobytes()
                host_txt = "%8.3f (%d runs)" % (ms, reps) + ("" if same else "  [host and device results differ on this world]"); ratio = "%8.2f" % (ms/dev)
            line = "  %5d    %5d       %8.3f (%.3f - %.3f)        %s    %s     %d" % (P, n, dev, p10, p90, host_txt, ratio, int((sel >= 0).sum()))
            print(line, flush=True); lines.append(line)
with open(args.out, "w") as f:
    f.write("the planes of a keyframe's new text detections in one call (tools/diag/gpu_text_theta.py); milliseconds\n" + "\n".join(lines) + "\n")
