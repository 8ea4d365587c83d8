"""GPU diagnostic (not a pytest): tsorb_fuse_frame (frame::FeatExtract's text half + frame::FeatFusion + AssignFeaturesToGrid in one call) on a 640 x 480 frame
with the extractor's 1000 scene features resident, for 4, 8 and 16 detections of about 120 x 40 px, nfeatures 500.  Host clock around the C calls (each ends
in a stream synchronise), two paths timed alternately in one job:
  (a) tsorb_fuse_frame: the fused set comes back and is the searched set
  (b) what an integrator had before the call existed: tsorb_text_extract (the raw text features come down), then tsorb_match_set_features on the fused
      arrays (56 bytes per feature go up).  The host work between the two -- two cv::pointPolygonTest per raw feature and the concatenation -- is NOT in
      (b)'s time: the fused arrays are prepared once, outside the clock.  (b) is therefore a lower bound of that path.
After both, one tsorb_match_search of 64 queries on each path's set must answer the same bytes (checked once, outside the clock).
20 warm-up rounds, then REPS rounds; median, p10 and p90 in ms, and the ratio (b) / (a) of the medians.

  python tools/diag/gpu_fuse_frame.py [out.txt]               timing table (also written to out.txt)
  FUSE_ONLY_CALLS=N python tools/diag/gpu_fuse_frame.py       only N calls of (a) with 8 detections (the workload for rocprofv3 --kernel-trace --stats)"""
import ctypes as C
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from textslam_amd.orbextractor import ORBextractor, synthetic_frame      # noqa: E402

REPS = int(os.environ.get("FUSE_REPS", "300"))
ONLY = int(os.environ.get("FUSE_ONLY_CALLS", "0"))
W, H, NF = 640, 480, 500
BOUNDS = (0.0, float(W), 0.0, float(H))
rng = np.random.default_rng(7)


def quads(n):
    """n boxes of about 120 x 40 px, rotated by up to +-12 degrees, anywhere in the frame."""
    out = []
    for _ in range(n):
        cx, cy, a = rng.uniform(80, W - 80), rng.uniform(40, H - 40), np.deg2rad(rng.uniform(-12, 12))
        hw, hh = rng.uniform(54, 66), rng.uniform(17, 23)
        c = np.array([[-hw, -hh], [hw, -hh], [hw, hh], [-hw, hh]]) @ np.array([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]])
        out.append(c + [cx, cy])
    return np.ascontiguousarray(out, np.float64)


up, fp, ip, dp = C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_double)
lines = []


def say(s):
    print(s, flush=True); lines.append(s)


def stats(t):
    return f"{np.median(t):.4f} ms (p10 {np.percentile(t, 10):.4f}, p90 {np.percentile(t, 90):.4f})"


ex = ORBextractor(); lib = ex.lib
ex.extract_batch(synthetic_frame(1, W, H))
n_scene = len(ex.download()[0][0])
cap_text = NF + 64


def run(n):
    q = quads(n); bb = np.ascontiguousarray(np.concatenate([q.min(1), q.max(1)], 1))
    cap = ex.cap + n*cap_text
    kp = np.zeros((cap, 6), np.float32); de = np.zeros((cap, 32), np.uint8); obj = np.zeros(cap, np.int32); src = np.zeros(cap, np.int32)
    off = np.zeros(n + 1, np.int32); raw = np.zeros(n, np.int32); n_out = np.zeros(2, np.int32)
    t_kp = np.zeros((n, cap_text, 6), np.float32); t_de = np.zeros((n, cap_text, 32), np.uint8); t_cn = np.zeros(n, np.int32)

    def fuse():
        assert lib.tsorb_fuse_frame(ex.ctx, 0, n, q.ctypes.data_as(dp), bb.ctypes.data_as(dp), -3.0, NF, cap_text, cap, *BOUNDS, kp.ctypes.data_as(fp), de.ctypes.data_as(up),
                                    obj.ctypes.data_as(ip), src.ctypes.data_as(ip), off.ctypes.data_as(ip), raw.ctypes.data_as(ip), n_out.ctypes.data_as(ip)) == 0
    fuse()
    f_kp = kp[:n_out[1]].copy(); f_de = de[:n_out[1]].copy(); nf = int(n_out[1])     # the fused arrays of path (b), prepared outside the clock

    def old():
        assert lib.tsorb_text_extract(ex.ctx, 0, n, q.ctypes.data_as(dp), NF, cap_text, t_kp.ctypes.data_as(fp), t_de.ctypes.data_as(up), t_cn.ctypes.data_as(ip)) == 0
        assert lib.tsorb_match_set_features(ex.ctx, f_kp.ctypes.data_as(fp), f_de.ctypes.data_as(up), nf, *BOUNDS) == 0
    return fuse, old, (f_kp, f_de, raw.copy(), int(n_out[0]), nf)


if ONLY:
    fuse, _, info = run(8)
    for _ in range(ONLY):
        fuse()
    print("ran", ONLY, "calls of 8 detections; raw", info[2].tolist(), "scene", info[3], "fused", info[4])
    sys.exit(0)

say(f"tsorb_fuse_frame, {W} x {H} frame, {n_scene} scene features resident, quads of about 120 x 40 px, nfeatures {NF}; 20 warm-up rounds, {REPS} rounds, (a) and (b) timed alternately")
say("(a) tsorb_fuse_frame   (b) tsorb_text_extract + tsorb_match_set_features on the fused arrays; the host filter and concatenation between them are NOT in (b)'s time")
for n in (4, 8, 16):
    fuse, old, (f_kp, f_de, raw, ns, nf) = run(n)
    sel = rng.choice(nf, 64, replace=False)
    args = (f_kp[sel, :2] + rng.uniform(-3, 3, (64, 2)).astype(np.float32), np.full(64, 12.0, np.float32), None, f_de[sel])
    fuse(); m_a = ex.match_search(*args); old(); m_b = ex.match_search(*args)
    assert all(m_a[k].tobytes() == m_b[k].tobytes() for k in m_a)
    t_a, t_b = [], []
    for r in range(20 + REPS):
        t0 = time.perf_counter(); fuse(); t1 = time.perf_counter(); old(); t2 = time.perf_counter()
        if r >= 20:
            t_a.append((t1 - t0)*1e3); t_b.append((t2 - t1)*1e3)
    say(f"n_dete={n:2d}  (a) {stats(t_a)}   (b) {stats(t_b)}   (b)/(a) {np.median(t_b)/np.median(t_a):.2f}   raw text keypoints {int(raw.sum())} (per detection min {int(raw.min())} "
        f"median {int(np.median(raw))} max {int(raw.max())}), fused {nf} = {ns} scene + {nf - ns} text")
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
