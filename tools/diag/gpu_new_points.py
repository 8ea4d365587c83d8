"""GPU diagnostic (not a pytest): what a new keyframe's scene points cost -- tsorb_match_new_points for 500 / 1000 / 2000 queries against 1000 / 2000 features of a
640 x 480 frame with the reference's 96-px radius and the level filter, and the initializer's shape (tsorb_match_search_claim: octave 0, a 100-px window, the ratio
test), copies included, timed through the raw C call (host clock around a call that ends in a stream synchronisation: the median after a warm-up with its 10th and
90th percentiles).  The grid is set once before the calls (tsorb_match_set_features is the caller's step after extraction and is not in the time).
Beside it the only host baseline there is without OpenCV: tests/cxx/new_points_host.hip, a single-thread -O2 build of the SAME __host__ __device__ functions
(textslam_amd/csrc/tsclaim.h) running the reference's loop on the same worlds, on the same machine.  It is NOT OpenCV (a one-sided Jacobi iteration in fp64 stands
where cv::triangulatePoints runs its SVD) and NOT the reference binary, and it is given every query's candidate list with the distances: the window walk and the
256-bit Hamming distances, which the device call does itself, are NOT in the host time.  Every shape is reported.

    python tools/diag/gpu_new_points.py [--calls 300] [--out profiles/new_points_timing.txt]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/diag/gpu_new_points.py --device-only --queries 1000 --features 1000      the device calls alone
    python tools/diag/gpu_new_points.py --build-only                                                                                  compile the host program and stop"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "new_points_timing.txt"))
ap.add_argument("--build-only", action="store_true")
ap.add_argument("--device-only", action="store_true")
ap.add_argument("--queries", default="500,1000,2000", help="the query counts, comma-separated")
ap.add_argument("--features", default="1000,2000", help="the searched sets' sizes, comma-separated")
args = ap.parse_args()
QUERIES = tuple(int(x) for x in args.queries.split(",")); FEATURES = tuple(int(x) for x in args.features.split(","))
HOST = os.path.join(ROOT, "tools", "bin", "new_points_host_o2")
SRC = os.path.join(ROOT, "tests", "cxx", "new_points_host.hip")

import new_points_io as IO                                            # noqa: E402


def build_host():
    deps = [SRC, os.path.join(ROOT, "include", "tsorb.h")] + [os.path.join(ROOT, "textslam_amd", "csrc", h) for h in ("tsclaim.h", "tstexttheta.h", "tsjacobi.h")]
    if not os.path.exists(HOST) or any(os.path.getmtime(d) > os.path.getmtime(HOST) for d in deps):
        os.makedirs(os.path.dirname(HOST), exist_ok=True)
        IO.build_host(HOST, sanitize=False)


if args.build_only:
    build_host(); sys.exit(0)

import numpy as np                                                     # noqa: E402
import new_points_ref as R                                            # noqa: E402
from textslam_amd.orbextractor import ORBextractor                    # noqa: E402

if not args.device_only:
    build_host()
ex = ORBextractor(nfeatures=2000)
FP, DP, IP, UP = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
lines = ["# per call, copies included, the grid set before; device = the median of %d calls after 20 warm-up calls with their 10th and 90th percentiles (three launches, two for the" % args.calls,
         "# initializer's search); host = one thread, hipcc -O2 host build of the same functions running the reference's loop over GIVEN candidate lists: the window walk and the",
         "# Hamming distances are not in the host time; mean of the runs of 0.5 s or more.  cand = the mean and the largest number of candidates of a query.",
         "# shape        queries  features  cand mean / max     device_ms (p10 - p90)         host_ms                      host/device     matches  good"]
shapes = [("keyframe", q, n) for n in FEATURES for q in QUERIES] + [("initializer", 1000, 1000)]
with tempfile.TemporaryDirectory() as tmp:
    for kind, nq, n2 in shapes:
        init = kind == "initializer"
        w = R.scene_world(200 + nq + n2, n2, nq, init=init, qr=100.0 if init else R.RADIUS, elig="all" if init else "half", bad_every=0 if init else 7)
        ex.match_set_features(w["kp6"], w["desc2"], w["bounds"])
        a = {k: np.ascontiguousarray(w[k], dt) for k, dt in (("qxy", np.float32), ("qr", np.float32), ("qlev", np.int32), ("qdesc", np.uint8), ("q_px", np.float32), ("K", np.float64))}
        a["Trw"] = np.ascontiguousarray(w["Trw"], np.float64); a["Tcw"] = np.ascontiguousarray(w["Tcw"], np.float64)
        elig = None if w["elig2"] is None else np.ascontiguousarray(w["elig2"], np.uint8)
        m12 = np.zeros(nq, np.int32); cnt = np.zeros(2, np.int32); p3d = np.zeros((nq, 3), np.float32); good = np.zeros(nq, np.uint8)
        head = (ex.ctx, nq, a["qxy"].ctypes.data_as(FP), a["qr"].ctypes.data_as(FP), a["qlev"].ctypes.data_as(IP), a["qdesc"].ctypes.data_as(UP),
                None if elig is None else elig.ctypes.data_as(UP), 50, int(init), 0.9)
        if init:
            fn = ex.lib.tsorb_match_search_claim; call = head + (m12.ctypes.data_as(IP), None, cnt[0:1].ctypes.data_as(IP))
        else:
            fn = ex.lib.tsorb_match_new_points
            call = head + (a["q_px"].ctypes.data_as(FP), a["Trw"].ctypes.data_as(DP), a["Tcw"].ctypes.data_as(DP), a["K"].ctypes.data_as(DP), 9, m12.ctypes.data_as(IP),
                           cnt[0:1].ctypes.data_as(IP), p3d.ctypes.data_as(FP), good.ctypes.data_as(UP), cnt[1:2].ctypes.data_as(IP))
        for _ in range(20):
            assert fn(*call) == 0
        ts = []
        for _ in range(args.calls):
            t0 = time.perf_counter(); fn(*call); ts.append((time.perf_counter() - t0)*1e3)
        ts.sort(); dev = ts[len(ts)//2]; p10, p90 = ts[len(ts)//10], ts[(9*len(ts))//10]
        host_txt, ratio, cand_txt = "not run", "", "-"
        if not args.device_only:
            cands = R.lists(w); nc = [len(c) for c, _ in cands]; cand_txt = "%6.1f / %4d" % (float(np.mean(nc)), max(nc))
            inp, outp = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
            IO.write_host(inp, w, cands)
            reps = 5
            while True:
                r = subprocess.run([HOST, inp, outp, str(reps)], capture_output=True, text=True, timeout=300)
                if r.returncode != 0:
                    sys.stderr.write(r.stdout + r.stderr); sys.exit(r.returncode)
                ms = float(re.search(r"loop_ms ([0-9.]+)", r.stdout).group(1))
                if ms*reps >= 500.0 or reps >= 20000:
                    break
                reps = int(reps*max(2.0, 600.0/max(ms*reps, 1e-3)))
            o = IO.read_host(outp, nq)
            same = o["match12"].tobytes() == m12.tobytes() and o["n_match"] == int(cnt[0]) and (init or (o["good"].astype(np.uint8).tobytes() == good.tobytes() and o["p3d"].tobytes() == p3d.tobytes()))
            host_txt = "%8.3f (%d runs)" % (ms, reps) + ("" if same else "  [host and device results differ on this world]"); ratio = "%8.2f" % (ms/dev)
        line = "  %-11s  %5d    %5d    %s       %8.3f (%.3f - %.3f)        %s    %s     %5d  %5d" % (kind, nq, n2, cand_txt, dev, p10, p90, host_txt, ratio, int(cnt[0]), int(cnt[1]))
        print(line, flush=True); lines.append(line)
with open(args.out, "w") as f:
    f.write("a new keyframe's scene points in one call, and the initializer's window search (tools/diag/gpu_new_points.py); milliseconds\n" + "\n".join(lines) + "\n")
