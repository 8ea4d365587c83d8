"""GPU diagnostic (not a pytest): what loop closing pays per call for its all-pairs matching -- tsorb_match_brute_scene at 1000 x 1000 features for 1, 4 and
8 candidates, tsorb_match_brute_text for 8 and 32 pairs of 60 x 60 -- copies included, beside a single-thread g++ -O2 transcription of the reference's loops
on the same machine.  Both are timed inside tests/cxx/loop_match_from_cxx (mode --time: host clock around calls that end in a stream synchronisation, the
median after a warm-up); this script compiles it into a temporary directory, runs it as a child process and keeps the table.

    python tools/diag/gpu_loop_match.py [--calls 50] [--out profiles/loop_match_timing.txt]
    python tools/diag/gpu_loop_match.py --stats [--stats-out profiles/loop_match_kernel_stats.txt]     the same workload under rocprofv3 --kernel-trace --stats"""
import argparse
import glob
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loop_match_timing.txt"))
ap.add_argument("--stats", action="store_true")
ap.add_argument("--stats-out", default=os.path.join(ROOT, "profiles", "loop_match_kernel_stats.txt"))
args = ap.parse_args()

with tempfile.TemporaryDirectory() as tmp:
    exe = os.path.join(tmp, "loop_match_from_cxx")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "adapter"),
                           "-o", exe, os.path.join(ROOT, "tests", "cxx", "loop_match_from_cxx.cpp"), "-L" + os.path.join(ROOT, "textslam_amd"), "-ltsorb",
                           "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.join(ROOT, "textslam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    if not args.stats:
        res = subprocess.run([exe, "--time", str(args.calls)], capture_output=True, text=True, timeout=240)
        sys.stdout.write(res.stdout); sys.stderr.write(res.stderr)
        if res.returncode != 0:
            sys.exit(res.returncode)
        with open(args.out, "w") as f:
            f.write("loopClosing::SearchMatch's matchers, one call for all candidates (tools/diag/gpu_loop_match.py); milliseconds\n" + res.stdout)
    else:
        prof = os.path.join(tmp, "prof")
        res = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", prof, "-o", "loop_match", "--", exe, "--time", str(args.calls)],
                             capture_output=True, text=True, timeout=400)
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
            f.write("rocprofv3 --kernel-trace --stats of loop_match_from_cxx --time %d (scene: 1000 x 1000 for 1 / 4 / 8 candidates, text: 8 / 32 pairs of 60 x 60; %d + 2 calls each)\n"
                    % (args.calls, args.calls) + top.stdout)
