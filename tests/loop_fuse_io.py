"""TEST INFRASTRUCTURE: builds and runs tests/cxx/loop_fuse_from_cxx.cpp (loop fusion's window searches through adapter/tsorb_loop_fuse.hpp over mock types) and reads
what it writes: the line of branch counters and the record file of the two calls' arrays (tests/cxx/dump_io.hpp: name, dtype 0 f64 / 1 i32 / 2 u8, count, bytes; the
float arrays are stored as their bits in i32)."""
import os
import re
import struct
import subprocess
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRANCHES = ("skipped", "source_changed", "added", "not_old", "neg_depth", "outside", "empty")       # the branches the world must make the transcription take
FLOATS = ("kp6", "qxy", "qr")


def build(tmp_path):
    exe = str(tmp_path / "loop_fuse_from_cxx")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "adapter"),
                           "-I" + os.path.join(ROOT, "tests", "cxx"), "-o", exe, os.path.join(ROOT, "tests", "cxx", "loop_fuse_from_cxx.cpp"),
                           "-L" + os.path.join(ROOT, "textslam_amd"), "-ltsorb", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "textslam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def run(exe, out_path, host):
    res = subprocess.run([exe] + (["--host"] if host else []) + [out_path], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    m = re.search(r"^loop fuse from C\+\+: ok (.*)$", res.stdout, re.M)
    assert m, res.stdout
    counters = dict(kv.split("=") for kv in m.group(1).split())
    assert counters.pop("mode") == ("host" if host else "device")
    return {k: int(v) for k, v in counters.items()}


def read_records(path):
    raw = open(path, "rb").read()
    out, at = {}, 0
    while at < len(raw):
        (nl,) = struct.unpack_from("<I", raw, at); at += 4
        name = raw[at:at + nl].decode(); at += nl
        dt, cnt = struct.unpack_from("<BQ", raw, at); at += 9
        t = {0: np.float64, 1: np.int32, 2: np.uint8}[dt]
        a = np.frombuffer(raw, t, cnt, at).copy(); at += a.nbytes
        out[name] = a.view(np.float32) if name.split("_", 1)[1] in FLOATS else a
    return out


def check_counters(c):
    for k in BRANCHES:
        assert c[k] > 0, (k, c)
    assert c["redone"] == c["source_changed"], c                # exactly the queries whose descriptor source changed were redone on the host
    assert c["fused"] > 0 and c["queries"] > 300 and c["mm_queries"] > 100 and c["mm_matches"] > 20 and c["mm_text"] > 0, c
