"""GPU diagnostic (not a pytest): what the two-view initializer's reconstruction costs per frame -- tsorb_match_two_view_reconstruct for n = 100 / 300 / 1000 / 3000
matches and both models (ReconstructH: 8 hypotheses, ReconstructF: 4), copies included, timed through the raw C call with the hyp_* outputs NULL, as the adapter calls
it (host clock around a call that ends in a stream synchronisation: the median after a warm-up with its 10th and 90th percentiles).  Beside it the only host baseline
there is without OpenCV: tests/cxx/two_view_reconstruct_host.hip, a single-thread -O2 build of the SAME __host__ __device__ functions
(textslam_amd/csrc/tstwoview_rec.h) on the same worlds, on the same machine.  It is NOT OpenCV's float cv::SVD::compute: a one-sided Jacobi iteration in fp64 stands
where OpenCV runs its float SVD of each 4 x 4.  Every shape is reported.

    python tools/diag/gpu_two_view_reconstruct.py [--calls 300] [--out profiles/two_view_reconstruct_timing.txt]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/diag/gpu_two_view_reconstruct.py --device-only      the device calls alone, as a profiler's workload
    python tools/diag/gpu_two_view_reconstruct.py --build-only                                                     compile the host program and stop"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_view_reconstruct_timing.txt"))
ap.add_argument("--build-only", action="store_true")
ap.add_argument("--device-only", action="store_true")
ap.add_argument("--sizes", default="100,300,1000,3000", help="the match counts, comma-separated")
args = ap.parse_args()
SIZES = tuple(int(x) for x in args.sizes.split(","))
HOST = os.path.join(ROOT, "tools", "bin", "two_view_reconstruct_host_o2")
SRC = os.path.join(ROOT, "tests", "cxx", "two_view_reconstruct_host.hip")

import two_view_reconstruct_io as IO                                  # noqa: E402


def build_host():
    deps = [SRC, os.path.join(ROOT, "include", "tsorb.h")] + [os.path.join(ROOT, "textslam_amd", "csrc", h) for h in ("tstwoview_rec.h", "tsjacobi.h")]
    if not os.path.exists(HOST) or any(os.path.getmtime(d) > os.path.getmtime(HOST) for d in deps):
        os.makedirs(os.path.dirname(HOST), exist_ok=True)
        IO.build_host(HOST, sanitize=False)


if args.build_only:
    build_host(); sys.exit(0)

import numpy as np                                                     # noqa: E402
import two_view_reconstruct_ref as R                                  # noqa: E402
from textslam_amd.orbextractor import ORBextractor                    # noqa: E402

if not args.device_only:
    build_host()
ex = ORBextractor()
F32, I32, U8 = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
lines = ["# per call, copies included, hyp_* outputs NULL; device = the median of %d calls after 20 warm-up calls with their 10th and 90th percentiles (three launches);" % args.calls,
         "# host = one thread, hipcc -O2 host build of the same functions, mean of the runs of 0.5 s or more",
         "# model  n          device_ms (p10 - p90)         host_ms                      host/device     result"]
with tempfile.TemporaryDirectory() as tmp:
    for model in (0, 1):
        for n in SIZES:
            w = R.scene_world("planar" if model == 0 else "general", n, n, model, K=(520.0, 520.0, 320.0, 240.0), w=640, h=480, drop=0.2)
            xy1, xy2 = np.ascontiguousarray(w["xy1"], np.float32), np.ascontiguousarray(w["xy2"], np.float32); inl = np.asarray(w["inlier"], np.uint8)
            M = np.ascontiguousarray(w["M21"], np.float32).reshape(9); K = np.asarray(w["K"], np.float32)
            res = np.zeros(6, np.int32); R21 = np.zeros(9, np.float32); t21 = np.zeros(3, np.float32); p3d = np.zeros((n, 3), np.float32); tri = np.zeros(n, np.uint8)
            a = (ex.ctx, n, xy1.ctypes.data_as(F32), xy2.ctypes.data_as(F32), inl.ctypes.data_as(U8), model, M.ctypes.data_as(F32), K.ctypes.data_as(F32), 1.0, 1.0, 50,
                 res.ctypes.data_as(I32), R21.ctypes.data_as(F32), t21.ctypes.data_as(F32), p3d.ctypes.data_as(F32), tri.ctypes.data_as(U8), None, None, None, None, None, None)
            fn = ex.lib.tsorb_match_two_view_reconstruct
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
                o = IO.read_host(outp, n)
                same = o["result"].tolist() == res.tolist() and o["p3d"].tobytes() == p3d.tobytes() and np.array_equal(o["triangulated"], tri.astype(bool))
                host_txt = "%8.3f (%d runs)" % (ms, reps) + ("" if same else "  [host and device results differ on this world]"); ratio = "%8.1f" % (ms/dev)
            line = "  %s    %5d       %8.3f (%.3f - %.3f)        %s    %s     %s" % ("HF"[model], n, dev, p10, p90, host_txt, ratio, res.tolist())
            print(line); lines.append(line)
with open(args.out, "w") as f:
    f.write("the two-view initializer's ReconstructH / ReconstructF in one call (tools/diag/gpu_two_view_reconstruct.py); milliseconds\n" + "\n".join(lines) + "\n")
