"""GPU diagnostic (not a pytest): what loop fusion pays for its window searches -- tsorb_match_search_sets for 1, 4, 8 and 24 sets of 1200 features at 640 x 480 with
1500 queries of radius 15 per set sharing one descriptor table, beside the loop it replaces (tsorb_match_set_features + tsorb_match_search per set), both through the
C ABI (ctypes, host clock around calls that end in a stream synchronisation), medians of alternating rounds.

    python tools/diag/gpu_window_sets.py [--rounds 200] [--commit TEXT] [--out profiles/window_sets_timing.txt]
    python tools/diag/gpu_window_sets.py --stats [--stats-out profiles/window_sets_kernel_stats.txt]     the same workload under rocprofv3 --kernel-trace --stats
    python tools/diag/gpu_window_sets.py --single-compare PARENT_LIB [--single-out profiles/grid_build_parent_vs_branch.txt]
        the single grid with the parent commit's libtsorb.so and with this tree's, alternating child processes.  Shape "search": tsorb_match_search alone (1000 queries of
        40-px radius in a 1000-feature frame, bench.py's also.orb_window_search).  Shapes "build N": the grid build on the timed path -- tsorb_match_set_features of N
        features, then a tsorb_match_search of 64 queries whose synchronisation waits for the build; N = 1000 and 1400 (the bench's frame, the fused set of the documented
        tsorb_fuse_frame shape) are gated against the parent's own spread, 4000 and 65536 are reported.
    python tools/diag/gpu_window_sets.py --single LIB        (the child of --single-compare: prints its medians per shape, microseconds)"""
import argparse
import ctypes as C
import glob
import os
import subprocess
import sys
import tempfile
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=200)
ap.add_argument("--commit", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_sets_timing.txt"))
ap.add_argument("--stats", action="store_true")
ap.add_argument("--stats-out", default=os.path.join(ROOT, "profiles", "window_sets_kernel_stats.txt"))
ap.add_argument("--single", default=None)
ap.add_argument("--single-compare", default=None)
ap.add_argument("--single-out", default=os.path.join(ROOT, "profiles", "grid_build_parent_vs_branch.txt"))
ap.add_argument("--no-write", action="store_true")
args = ap.parse_args()
VP, I32, U8, F32, F64 = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_double)
BOUNDS = (0.0, 640.0, 0.0, 480.0)


def commit_text():
    if args.commit:
        return args.commit
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        return "unknown (no git metadata beside the tree)"


def p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def open_lib(path):
    L = C.CDLL(path)
    L.tsorb_create.argtypes = [C.POINTER(VP), C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int]
    L.tsorb_destroy.argtypes = [VP]
    L.tsorb_match_set_features.argtypes = [VP, F32, U8, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double]
    L.tsorb_match_search.argtypes = [VP, C.c_int, F32, F32, I32, U8, C.c_int, I32, I32, I32, I32, I32, I32]
    ctx = VP()
    rc = L.tsorb_create(C.byref(ctx), 1000, 1.2, 8, 20, 7, 0)
    if rc != 0:
        sys.exit("tsorb_create failed with %d" % rc)
    return L, ctx


def features(rng, n):
    kp = np.zeros((n, 6), np.float32)
    kp[:, 0] = rng.uniform(0, 640, n); kp[:, 1] = rng.uniform(0, 480, n); kp[:, 2] = 31.0; kp[:, 5] = rng.integers(0, 8, n)
    return kp, rng.integers(0, 256, (n, 32), dtype=np.uint8)


def pct(t):
    t = np.sort(np.asarray(t)) * 1e6
    return float(np.median(t)), float(t[int(0.1 * (len(t) - 1))]), float(t[int(0.9 * (len(t) - 1))])


# ------------------------------------------------------------------ the single grid, one library
BUILD_N = (1000, 1400, 4000, 65536)
GATED = ("search", "build 1000", "build 1400")


def single(lib_path, groups=5, calls=300):
    L, ctx = open_lib(lib_path)
    rng = np.random.default_rng(1)

    def shape(name, n, nq, build):
        kp, desc = features(rng, n)
        qxy = (kp[rng.integers(0, n, nq), :2] + rng.normal(0, 3, (nq, 2))).astype(np.float32); qr = np.full(nq, 40.0, np.float32)
        qd = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
        out = [np.zeros(nq, np.int32) for _ in range(4)]
        set_ = lambda: L.tsorb_match_set_features(ctx, p(kp, F32), p(desc, U8), n, *BOUNDS)
        search = lambda: L.tsorb_match_search(ctx, nq, p(qxy, F32), p(qr, F32), None, p(qd, U8), 0, None, None, p(out[0], I32), p(out[1], I32), p(out[2], I32), p(out[3], I32))
        call = (lambda: set_() | search()) if build else search
        assert set_() == 0
        for _ in range(50):
            assert call() == 0
        meds = []
        for _ in range(groups):
            t = []
            for _ in range(calls):
                t0 = time.perf_counter(); call(); t.append(time.perf_counter() - t0)
            meds.append(pct(t)[0])
        print("shape %s: medians_us " % name + " ".join("%.2f" % m for m in meds) + " checksum %d" % int(out[0].sum() + out[2].astype(np.int64).sum()), flush=True)
    shape("search", 1000, 1000, False)
    for n in BUILD_N:
        shape("build %d" % n, n, 64, True)
    L.tsorb_destroy(ctx)


def single_compare(parent_lib):
    branch_lib = os.path.join(ROOT, "textslam_amd", "libtsorb.so")
    names = ["search"] + ["build %d" % n for n in BUILD_N]
    rows = {(label, nm): [] for label in ("parent", "branch") for nm in names}; sums = {nm: set() for nm in names}
    for rnd in range(5):
        for label, lib in (("parent", parent_lib), ("branch", branch_lib)):
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--single", lib], capture_output=True, text=True, timeout=200)
            if res.returncode != 0:
                sys.exit(res.stdout + res.stderr)
            for line in res.stdout.splitlines():
                nm, rest = line[len("shape "):].split(": ", 1); w = rest.split()
                rows[(label, nm)].append([float(x) for x in w[1:w.index("checksum")]]); sums[nm].add(w[-1])
    lines = ["the single grid: the library of the parent commit against this tree's (%s), tools/diag/gpu_window_sets.py --single-compare, one job on one MI355X;" % commit_text(),
             "child processes parent, branch alternating, five of each; each prints per shape 5 medians of 300 timed units after 50 warm-up units (C ABI through ctypes, host",
             "clock); microseconds.  640 x 480, 40-px radius, max_cand 0.  search: one tsorb_match_search of 1000 queries in a 1000-feature frame (the grid built before).",
             "build N: tsorb_match_set_features of N features + one tsorb_match_search of 64 queries, which waits for the build.  Gated: %s; the others are reported." % ", ".join(GATED)]
    ok = True
    for nm in names:
        pa = np.array(rows[("parent", nm)]).reshape(-1); br = np.array(rows[("branch", nm)]).reshape(-1)
        lines.append("---- %s (the results' checksums agree: %s)" % (nm, len(sums[nm]) == 1))
        for label in ("parent", "branch"):
            for k, r in enumerate(rows[(label, nm)]):
                lines.append("%s process %d: %s" % (label, k + 1, "  ".join("%8.2f" % x for x in r)))
        lo, hi = pa.min(), pa.max()
        lines.append("parent: median of its medians %.2f, spread of its own medians %.2f .. %.2f (the noise of this job)" % (np.median(pa), lo, hi))
        lines.append("branch: median of its medians %.2f, its medians %.2f .. %.2f" % (np.median(br), br.min(), br.max()))
        where = "inside" if lo <= np.median(br) <= hi else ("BELOW" if np.median(br) < lo else "ABOVE")
        lines.append("branch median %s the parent's spread (%s)" % (where, "gated" if nm in GATED else "reported only"))
        ok = ok and len(sums[nm]) == 1 and (nm not in GATED or where != "ABOVE")
    lines.append("gates: %s" % ("hold" if ok else "FAIL"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if not args.no_write:
        open(args.single_out, "w").write(text)


# ------------------------------------------------------------------ the batch call against the loop of single-set calls
def batch_vs_loop(rounds, write):
    sys.path.insert(0, ROOT)
    from textslam_amd import orbextractor
    L = orbextractor.load_library()
    ctx = VP()
    assert L.tsorb_create(C.byref(ctx), 1000, 1.2, 8, 20, 7, 0) == 0
    rng = np.random.default_rng(7)
    NF, NQ, KMAX = 1200, 1500, 24
    sets = [features(rng, NF) for _ in range(KMAX)]
    table = rng.integers(0, 256, (NQ, 32), dtype=np.uint8)
    qxy1 = np.stack([rng.uniform(0, 640, NQ), rng.uniform(0, 480, NQ)], 1).astype(np.float32); qr1 = np.full(NQ, 15.0, np.float32)
    lines = ["loop fusion's window searches: one tsorb_match_search_sets call against the loop of tsorb_match_set_features + tsorb_match_search per set (tools/diag/gpu_window_sets.py)",
             "tree: %s; sets of %d features at 640 x 480, %d queries of radius 15 per set sharing one table of %d descriptors, max_cand 0; C ABI through ctypes, host clock," % (commit_text(), NF, NQ, NQ),
             "median of %d alternating rounds (p10 .. p90), microseconds" % rounds,
             "sets  queries | loop of single-set calls        | batch call                      | batch / loop"]
    for K in (1, 4, 8, 24):
        foff = (np.arange(K + 1) * NF).astype(np.int32)
        kp = np.ascontiguousarray(np.concatenate([s[0] for s in sets[:K]])); desc = np.ascontiguousarray(np.concatenate([s[1] for s in sets[:K]]))
        bounds = np.tile(np.array(BOUNDS), (K, 1)).astype(np.float64)
        qset = np.repeat(np.arange(K, dtype=np.int32), NQ); qdi = np.tile(np.arange(NQ, dtype=np.int32), K)
        qxy = np.ascontiguousarray(np.tile(qxy1, (K, 1))); qr = np.tile(qr1, K)
        ob = [np.zeros(K * NQ, np.int32) for _ in range(3)]; ol = [np.zeros(K * NQ, np.int32) for _ in range(3)]

        def batch():
            return L.tsorb_match_search_sets(ctx, K, p(foff, I32), p(kp, F32), p(desc, U8), p(bounds, F64), NQ, p(table, U8), K * NQ, p(qset, I32), p(qdi, I32), p(qxy, F32), p(qr, F32),
                                             None, 0, None, None, p(ob[0], I32), p(ob[1], I32), p(ob[2], I32), None)

        def loop():
            rc = 0
            for s in range(K):
                rc |= L.tsorb_match_set_features(ctx, p(sets[s][0], F32), p(sets[s][1], U8), NF, *BOUNDS)
                o = [C.cast(C.c_void_p(a.ctypes.data + 4 * s * NQ), I32) for a in ol]
                rc |= L.tsorb_match_search(ctx, NQ, p(qxy1, F32), p(qr1, F32), None, p(table, U8), 0, None, None, o[0], o[1], o[2], None)
            return rc
        for _ in range(10):
            assert batch() == 0 and loop() == 0
        assert all(np.array_equal(a, b) for a, b in zip(ob, ol)), "the two sides disagree"
        tb, tl = [], []
        for _ in range(rounds):
            t0 = time.perf_counter(); loop(); t1 = time.perf_counter(); batch(); t2 = time.perf_counter()
            tl.append(t1 - t0); tb.append(t2 - t1)
        (ml, l10, l90), (mb, b10, b90) = pct(tl), pct(tb)
        lines.append("%4d  %7d | %8.1f (%8.1f .. %8.1f) | %8.1f (%8.1f .. %8.1f) | %.3f" % (K, K * NQ, ml, l10, l90, mb, b10, b90, mb / ml))
    L.tsorb_destroy(ctx)
    lines.append("(the same searches on both sides, the results compared equal before timing; queries with a candidate: %.0f %%)" % (100.0 * (ob[0] > 0).mean()))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if write:
        open(args.out, "w").write(text)


if args.single:
    single(args.single)
elif args.single_compare:
    single_compare(args.single_compare)
elif args.stats:
    with tempfile.TemporaryDirectory() as tmp:
        prof = os.path.join(tmp, "prof")
        res = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", prof, "-o", "window_sets", "--", sys.executable, os.path.abspath(__file__), "--rounds", "50", "--no-write"],
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
            f.write("rocprofv3 --kernel-trace --stats of tools/diag/gpu_window_sets.py --rounds 50 (tree: %s; 1 / 4 / 8 / 24 sets of 1200 features, 1500 queries per set; 50 + 10 rounds each,\n"
                    "a round = the loop of single-set calls, then the batch call)\n" % commit_text() + top.stdout)
else:
    batch_vs_loop(args.rounds, not args.no_write)
