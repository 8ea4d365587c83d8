"""GPU diagnostic (not a pytest): what loop detection pays per keyframe for its string scan and vote -- tsloop_detect_loop for 8 / 16 / 32 queries against 500 / 5000 /
20 000 map texts of 3 - 16 bytes, copies included, beside a single-thread g++ -O2 restatement of the reference's loop (std::string texts, the DP, a stable sort per
query) on the same machine.  Both are timed inside tools/diag/detect_loop_time.cpp (a program of its own over the suite's mock world and restatement, tests/cxx/loop_detect_plain.hpp: host clock around calls that end in a stream synchronisation, the
median after a warm-up with its 10th and 90th percentiles, every shape's window a fraction of a second or more; the two sides' match counts and candidates are compared on every shape); this script compiles it into a temporary directory, runs it as a
child process and keeps the table.  Every shape is reported, also one at which the host loop wins.

    python tools/diag/gpu_detect_loop.py [--calls 2000] [--out profiles/detect_loop_timing.txt]
    python tools/diag/gpu_detect_loop.py --stats [--stats-out profiles/detect_loop_kernel_stats.txt]     the same workload under rocprofv3 --kernel-trace --stats"""
import argparse
import glob
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=2000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detect_loop_timing.txt"))
ap.add_argument("--stats", action="store_true")
ap.add_argument("--stats-out", default=os.path.join(ROOT, "profiles", "detect_loop_kernel_stats.txt"))
args = ap.parse_args()

with tempfile.TemporaryDirectory() as tmp:
    exe = os.path.join(tmp, "detect_loop_time")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "adapter"),
                           "-I" + os.path.join(ROOT, "tests", "cxx"), "-o", exe, os.path.join(ROOT, "tools", "diag", "detect_loop_time.cpp"),
                           "-L" + os.path.join(ROOT, "textslam_amd"), "-ltsloop", "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.join(ROOT, "textslam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    if not args.stats:
        res = subprocess.run([exe, str(args.calls)], capture_output=True, text=True, timeout=400)
        sys.stdout.write(res.stdout); sys.stderr.write(res.stderr)
        if res.returncode != 0:
            sys.exit(res.returncode)
        with open(args.out, "w") as f:
            f.write("loopClosing::DetectLoop's string scan, match lists, vote and candidates in one call (tools/diag/gpu_detect_loop.py); milliseconds\n" + res.stdout)
    else:
        prof = os.path.join(tmp, "prof")
        res = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", prof, "-o", "detect_loop", "--", exe, str(args.calls)],
                             capture_output=True, text=True, timeout=500)
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
            f.write("rocprofv3 --kernel-trace --stats of detect_loop_time %d (8 / 16 / 32 queries x 500 / 5000 / 20000 map texts; %d + 5 calls per shape)\n"
                    % (args.calls, args.calls) + top.stdout)
