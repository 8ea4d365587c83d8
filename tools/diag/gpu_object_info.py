"""GPU diagnostic (not a pytest): what a new keyframe pays for the constructors of its new text objects (mapText::GetObjectInfo) -- ONE
tsframe_text_object_info call against the loop of the existing single calls fed with the same mu, sigma: per object L x tsframe_neighbours and
2 x tsframe_box_pixels (one to count, one to fill).  The loop cannot compute mu / sigma at all (an integrator would fetch every level and do it on the
host), so its column is a lower bound of the cost before this call existed.

Frame: 640 x 480, 4 levels.  Rows: 1 / 8 / 16 objects, rotated quads of about 120 x 40 pixels, 60 features each (from tsframe_pyramid_pts_batch).
Both sides are timed at the C ABI through ctypes on arrays prepared beforehand (no numpy work inside the clock), host clock around calls that end in a
stream synchronisation, the loop and the one call alternating in one loop, median of --calls rounds after a warm-up.  Before a row is timed the one
call's outputs are compared, byte for byte, with the loop's.  Writes the table to --out (default profiles/object_info_timing.txt).

    python tools/diag/gpu_object_info.py [--calls 300] [--out profiles/object_info_timing.txt]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=300)
ap.add_argument("--warmup", type=int, default=30)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "object_info_timing.txt"))
args = ap.parse_args()
assert args.calls >= 200 or args.out == "/dev/null", "the table wants the median of at least 200 rounds"

from textslam_amd.frame import Frame                    # noqa: E402
from textslam_amd.orbextractor import synthetic_frame   # noqa: E402

L = 4
INV = np.array([1.0, 0.5, 0.25, 0.125])
img = synthetic_frame(1)
assert img.shape == (480, 640)
fr = Frame(0)
fr.GetPyrMat(img, L)
lib, ctx = fr.lib, fr.ctx
rng = np.random.default_rng(7)
ip, dp, up = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def make_objects(n):
    quads, sets = [], []
    for _ in range(n):
        cx, cy, a = rng.uniform(90, 550), rng.uniform(70, 410), rng.uniform(-0.3, 0.3)
        c, s = np.cos(a), np.sin(a)
        q = np.array([(-60, -20), (60, -20), (60, 20), (-60, 20)], np.float64) @ np.array([[c, s], [-s, c]]) + (cx, cy)
        x0, y0, x1, y1 = q[:, 0].min(), q[:, 1].min(), q[:, 0].max(), q[:, 1].max()
        xy = np.stack([rng.uniform(x0, x1, 60), rng.uniform(y0, y1, 60)], 1).astype(np.float32)
        quads.append(q); sets.append((0, xy, (x0, y0, x1, y1)))
    return np.array(quads), fr.GetPyramidPtsBatch(sets, INV)


def prepare(quads, feats):
    n = len(quads)
    lo = np.ascontiguousarray([f["level_off"] for f in feats], np.int32)
    foff = np.zeros(n + 1, np.int32); foff[1:] = np.cumsum(lo[:, 1])                    # the slices of tsframe_pyramid_pts_batch
    cap = int(foff[n])*L
    u = np.zeros(cap); v = np.zeros(cap); I = np.zeros(cap)
    for i, f in enumerate(feats):
        b = int(foff[i])*L; m = int(lo[i, L])
        u[b:b + m] = f["u"]; v[b:b + m] = f["v"]; I[b:b + m] = f["inten"]
    got = fr.GetObjectInfoBatch(quads, INV, feats)
    pcap = sum(len(g["vRefPixs"]["u"]) for g in got)
    one = {"ms": np.zeros((n, L, 2)), "ok": np.zeros((n, L), np.uint8), "N": np.zeros(cap), "I8": np.zeros((cap, 8)), "N8": np.zeros((cap, 8)),
           "in": np.zeros(cap, np.uint8), "poff": np.zeros(n + 1, np.int32), "pu": np.zeros(pcap, np.int32), "pv": np.zeros(pcap, np.int32),
           "pI": np.zeros(pcap), "pN": np.zeros(pcap)}
    call = (n, quads.ctypes.data_as(dp), INV.ctypes.data_as(dp), foff.ctypes.data_as(ip), lo.ctypes.data_as(ip), u.ctypes.data_as(dp), v.ctypes.data_as(dp),
            I.ctypes.data_as(dp), pcap, one["ms"].ctypes.data_as(dp), one["ok"].ctypes.data_as(up), one["N"].ctypes.data_as(dp), one["I8"].ctypes.data_as(dp),
            one["N8"].ctypes.data_as(dp), one["in"].ctypes.data_as(up), one["poff"].ctypes.data_as(ip), one["pu"].ctypes.data_as(ip), one["pv"].ctypes.data_as(ip),
            one["pI"].ctypes.data_as(dp), one["pN"].ctypes.data_as(dp))
    # the loop: the same places, mu / sigma handed in (the loop has no way to compute them)
    lp = {"I8": np.zeros((cap, 8)), "N8": np.zeros((cap, 8)), "in": np.zeros(cap, np.uint8), "pu": np.zeros(pcap, np.int32), "pv": np.zeros(pcap, np.int32),
          "pI": np.zeros(pcap), "pN": np.zeros(pcap), "cnt": np.zeros(n, np.int32)}
    uvs, nb, bx = [], [], []
    pat = 0
    for i, g in enumerate(got):
        assert g["ok"].all()
        for l in range(L):
            a, b = int(foff[i])*L + int(lo[i, l]), int(foff[i])*L + int(lo[i, l + 1])
            uv = np.ascontiguousarray(np.stack([u[a:b], v[a:b]], 1)); uvs.append(uv)
            nb.append((l, uv.ctypes.data_as(dp), b - a, float(g["statistics"][l, 0]), float(g["statistics"][l, 1]), lp["I8"][a:].ctypes.data_as(dp),
                       lp["N8"][a:].ctypes.data_as(dp), lp["in"][a:].ctypes.data_as(up)))
        q = np.ascontiguousarray(quads[i]*INV[0]); uvs.append(q)
        m = len(g["vRefPixs"]["u"])
        bx.append((q.ctypes.data_as(dp), float(g["statistics"][0, 0]), float(g["statistics"][0, 1]), m, lp["cnt"][i:].ctypes.data_as(ip),
                   lp["pu"][pat:].ctypes.data_as(ip), lp["pv"][pat:].ctypes.data_as(ip), lp["pI"][pat:].ctypes.data_as(dp), lp["pN"][pat:].ctypes.data_as(dp)))
        pat += m
    return call, nb, bx, one, lp, (quads, lo, foff, u, v, I, uvs)


def run_one(call):
    rc = lib.tsframe_text_object_info(ctx, *call)
    assert rc == 0, lib.tsframe_last_error(ctx)


def run_loop(nb, bx):
    for l, puv, n, mu, sg, i8, n8, inn in nb:
        rc = lib.tsframe_neighbours(ctx, l, puv, n, mu, sg, i8, n8, inn)
        assert rc == 0, lib.tsframe_last_error(ctx)
    for q, mu, sg, m, cnt, pu, pv, pI, pN in bx:
        rc = lib.tsframe_box_pixels(ctx, 0, q, mu, sg, 0, cnt, None, None, None, None)          # count
        assert rc == 0, lib.tsframe_last_error(ctx)
        rc = lib.tsframe_box_pixels(ctx, 0, q, mu, sg, m, cnt, pu, pv, pI, pN)                  # fill
        assert rc == 0, lib.tsframe_last_error(ctx)


say("mapText::GetObjectInfo for the new text objects of one 640 x 480 keyframe, 4 levels, quads of about 120 x 40 pixels, 60 features each: the loop of single calls "
    "(per object 4 x tsframe_neighbours + 2 x tsframe_box_pixels, mu / sigma handed in) vs one tsframe_text_object_info call (mu / sigma included); C ABI through "
    "ctypes, host clock, median of %d alternating rounds (p10 .. p90), microseconds" % args.calls)
say("%-12s %6s %9s %8s | %-30s | %-30s | %s" % ("objects", "calls", "features", "pixels", "loop of single calls", "one call", "one / loop"))
ratios = {}
for n in (1, 8, 16):
    quads, feats = make_objects(n)
    call, nb, bx, one, lp, keep = prepare(quads, feats)
    run_one(call); run_loop(nb, bx)
    for k in ("I8", "N8", "in", "pu", "pv", "pI", "pN"):                                             # the same results (untouched gaps are zeros on both sides)
        assert one[k].tobytes() == lp[k].tobytes(), (n, k)
    assert np.array_equal(np.diff(one["poff"]), lp["cnt"])
    t_loop, t_one = [], []
    for it in range(args.warmup + args.calls):
        t0 = time.perf_counter(); run_loop(nb, bx); t1 = time.perf_counter(); run_one(call); t2 = time.perf_counter()
        if it >= args.warmup:
            t_loop.append((t1 - t0)*1e6); t_one.append((t2 - t1)*1e6)
    q = lambda t: "%8.1f (%8.1f .. %8.1f)" % (np.median(t), np.percentile(t, 10), np.percentile(t, 90))
    ratios[n] = float(np.median(t_one)/np.median(t_loop))
    say("%-12d %6d %9d %8d | %-30s | %-30s | %.3f" % (n, len(nb) + 2*len(bx), int(keep[1][:, L].sum()), int(one["poff"][n]), q(t_loop), q(t_one), ratios[n]))
say()
say("8 objects: one call / loop of 48 calls = %.3f, the loop takes %.1f times as long -- %s (required: the one call is below the loop)"
    % (ratios[8], 1.0/ratios[8], "holds" if ratios[8] < 1.0 else "does NOT hold"))
say("(the ctypes call overhead, about a microsecond per call, is inside both columns)")
if args.out != "/dev/null":
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
