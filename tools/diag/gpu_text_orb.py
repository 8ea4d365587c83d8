"""GPU diagnostic (not a pytest): tsorb_text_extract (frame::FeatExtracText: cv::ORB detect on the masked frame + compute on the frame, every detection of
a frame in one call) for 1, 4, 8 and 16 detections on a 640 x 480 frame, quads of about 200 x 60 px (the text-box scale of the reference's sample
sequences), nfeatures 500.  Per call, host clock around the C call (it ends in a stream synchronise):
  resident   the frame is already in the context (the scene extraction uploaded it): tsorb_text_extract alone
  one-shot   tsorb_extract_batch of the frame (upload + scene extraction) followed by tsorb_text_extract
Beside them the project's own extractor on the same number of FULL frames (tsorb_extract_batch, n frames): the yardstick the call is expected to stay
under -- at worst it runs the same stages on n masked frames plus one shared description pyramid.  There is no OpenCV here to compare with.
The three are timed alternately, 20 warm-up rounds, then REPS rounds; median, p10 and p90 in ms.

  python tools/diag/gpu_text_orb.py [out.txt]             timing table (also written to out.txt)
  TEXT_ORB_ONLY_CALLS=N python tools/diag/gpu_text_orb.py   only N resident calls of 8 detections (the workload for rocprofv3 --kernel-trace --stats)"""
import ctypes as C
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from textslam_amd.orbextractor import ORBextractor, synthetic_frame      # noqa: E402

REPS = int(os.environ.get("TEXT_ORB_REPS", "200"))
ONLY = int(os.environ.get("TEXT_ORB_ONLY_CALLS", "0"))
W, H, NF = 640, 480, 500
rng = np.random.default_rng(7)
frames = np.stack([synthetic_frame(s, W, H) for s in range(1, 17)])


def quads(n):
    """n boxes of about 200 x 60 px, rotated by up to +-12 degrees, anywhere in the frame."""
    out = []
    for _ in range(n):
        cx, cy, a = rng.uniform(110, W - 110), rng.uniform(50, H - 50), np.deg2rad(rng.uniform(-12, 12))
        hw, hh = rng.uniform(90, 110), rng.uniform(25, 35)
        c = np.array([[-hw, -hh], [hw, -hh], [hw, hh], [-hw, hh]]) @ np.array([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]])
        out.append(c + [cx, cy])
    return np.ascontiguousarray(out, np.float64)


up, fp, ip, dp = C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_double)
lines = []


def say(s):
    print(s, flush=True); lines.append(s)


def stats(t):
    return f"{np.median(t):.4f} ms (p10 {np.percentile(t, 10):.4f}, p90 {np.percentile(t, 90):.4f})"


text = ORBextractor(); lib = text.lib                   # the frame's context: scene extraction + text extraction
batch = ORBextractor()                                  # the yardstick: n full frames
cap = NF + 64
one = np.ascontiguousarray(frames[:1])
s_kp = np.zeros((1, text.cap, 6), np.float32); s_de = np.zeros((1, text.cap, 32), np.uint8); s_cn = np.zeros(1, np.int32)


def scene():
    assert lib.tsorb_extract_batch(text.ctx, one.ctypes.data_as(up), 1, W, H, W, s_kp.ctypes.data_as(fp), s_de.ctypes.data_as(up), s_cn.ctypes.data_as(ip), text.cap) == 0


if ONLY:
    scene(); q = quads(8)
    kp = np.zeros((8, cap, 6), np.float32); de = np.zeros((8, cap, 32), np.uint8); cn = np.zeros(8, np.int32)
    for _ in range(ONLY):
        assert lib.tsorb_text_extract(text.ctx, 0, 8, q.ctypes.data_as(dp), NF, cap, kp.ctypes.data_as(fp), de.ctypes.data_as(up), cn.ctypes.data_as(ip)) == 0
    print("ran", ONLY, "resident calls of 8 detections; keypoints", cn.tolist())
    sys.exit(0)

say(f"tsorb_text_extract, {W} x {H} frame, quads of about 200 x 60 px, nfeatures {NF}; 20 warm-up rounds, {REPS} rounds, the three timed alternately")
for n in (1, 4, 8, 16):
    q = quads(n)
    kp = np.zeros((n, cap, 6), np.float32); de = np.zeros((n, cap, 32), np.uint8); cn = np.zeros(n, np.int32)
    b_img = np.ascontiguousarray(frames[:n])
    b_kp = np.zeros((n, batch.cap, 6), np.float32); b_de = np.zeros((n, batch.cap, 32), np.uint8); b_cn = np.zeros(n, np.int32)

    def text_call():
        assert lib.tsorb_text_extract(text.ctx, 0, n, q.ctypes.data_as(dp), NF, cap, kp.ctypes.data_as(fp), de.ctypes.data_as(up), cn.ctypes.data_as(ip)) == 0

    def batch_call():
        assert lib.tsorb_extract_batch(batch.ctx, b_img.ctypes.data_as(up), n, W, H, W, b_kp.ctypes.data_as(fp), b_de.ctypes.data_as(up), b_cn.ctypes.data_as(ip), batch.cap) == 0

    t_res, t_shot, t_scene, t_batch = [], [], [], []
    for r in range(20 + REPS):
        scene()
        t0 = time.perf_counter(); text_call(); t1 = time.perf_counter()
        scene(); text_call()
        t2 = time.perf_counter(); scene(); t3 = time.perf_counter(); text_call(); t4 = time.perf_counter()
        batch_call()
        t5 = time.perf_counter(); batch_call(); t6 = time.perf_counter()
        if r >= 20:
            t_res.append((t1 - t0)*1e3); t_shot.append((t4 - t2)*1e3); t_scene.append((t3 - t2)*1e3); t_batch.append((t6 - t5)*1e3)
    say(f"n_dete={n:2d}  resident {stats(t_res)}   one-shot {stats(t_shot)} (its scene extraction {np.median(t_scene):.4f})   "
        f"tsorb_extract_batch of {n:2d} full frames {stats(t_batch)}   text keypoints per detection: min {int(cn.min())} median {int(np.median(cn))} max {int(cn.max())}")
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
