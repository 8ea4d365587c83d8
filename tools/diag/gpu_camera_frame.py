"""GPU diagnostic (not a pytest): what the first stage of a camera frame costs at the C ABI.

  (a) tsframe_set_raw_image + tsorb_extract_device: ONE upload of the raw frame (BGR, and grey), undistortion, grey conversion, BA pyramid and ORB
      from the resident level 0;
  (b) the path before these calls existed, on the same box in the same job: tsframe_set_image + tsorb_extract_batch on a grey image that is already
      undistorted and already on the host (two uploads; the host's cv::undistort and cvtColor are NOT in this column: no OpenCV here to time);
  (c) the numpy restatement of the undistortion and grey conversion (tests/camera_frame_ref.py) -- NOT OpenCV, only the one host figure that can be
      taken here; it says nothing about cv::undistort's speed;
  and tsframe_set_camera once (the map, per camera).

Sizes 640 x 480 and 1241 x 376, the ORB benchmark's synthetic frame as the raw image, the barrel camera of tests/test_gpu_camera_frame.py, 4 pyramid levels, ORB 1000 features / 8 levels.  Timed through
ctypes on arrays prepared beforehand, host clock around calls that end in a stream synchronisation, (a) and (b) alternating in one loop, median of
--calls rounds after a warm-up with the 10th .. 90th percentiles.  Before a row is timed (a)'s outputs are compared, byte for byte, with (b)'s on the
restatement's grey image.  Writes the table to --out (default profiles/camera_frame_timing.txt).

    python tools/diag/gpu_camera_frame.py [--calls 300] [--out profiles/camera_frame_timing.txt]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=300)
ap.add_argument("--warmup", type=int, default=30)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "camera_frame_timing.txt"))
args = ap.parse_args()
assert args.calls >= 200 or args.out == "/dev/null", "the table wants the median of at least 200 rounds"

import camera_frame_ref as R                             # noqa: E402
from textslam_amd.frame import Frame                     # noqa: E402
from textslam_amd.orbextractor import ORBextractor, synthetic_frame       # noqa: E402

NL = 4
fp, up, ip, dp = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_double)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def q(t):
    return "%8.1f (%8.1f .. %8.1f)" % (np.median(t), np.percentile(t, 10), np.percentile(t, 90))


say("first stage of a camera frame: (a) tsframe_set_raw_image + tsorb_extract_device (one upload of the raw frame) vs (b) tsframe_set_image + "
    "tsorb_extract_batch on an undistorted grey image already on the host (two uploads; the host undistort / cvtColor of that path are not timed: no "
    "OpenCV here); barrel camera, %d pyramid levels, ORB 1000 x 8; C ABI through ctypes, host clock, median of %d alternating rounds (p10 .. p90), microseconds" % (NL, args.calls))
say("%-12s %-5s %9s | %-30s | %-30s | %7s | %-30s | %s" % ("size", "raw", "bytes up", "(a) raw frame, one upload", "(b) grey image, two uploads", "(a)/(b)",
                                                        "(a) without ORB", "tsframe_set_camera, once"))
dist, K_new = R.CAMERAS["barrel"]
ratios = []
for w, h in ((640, 480), (1241, 376)):
    fr, fr_b = Frame(0), Frame(0)
    ex_a, ex_b = ORBextractor(device=0), ORBextractor(device=0)
    K = np.array(R.K_REF); d = np.array(dist)
    t_cam = []
    for _ in range(5):
        t0 = time.perf_counter(); fr.SetCamera(w, h, K, d, K_new); t_cam.append((time.perf_counter() - t0)*1e6)
    maps = fr.undist_map()
    cap = ex_a.cap
    out = {s: (np.zeros((cap, 6), np.float32), np.zeros((cap, 32), np.uint8), np.zeros(1, np.int32)) for s in "ab"}
    for fmt, ch, label in ((R.RAW_BGR, 3, "BGR"), (R.RAW_GREY, 1, "grey")):
        scene = synthetic_frame(1, w, h)                                     # the ORB benchmark's frame; as BGR the same plane three times (its grey is the plane)
        raw = np.ascontiguousarray(np.stack([scene]*3, -1) if ch == 3 else scene)
        t0 = time.perf_counter(); _, grey = R.camera_frame(raw, fmt, None, None, maps=maps); t_np = (time.perf_counter() - t0)*1e6      # (c), the map given
        grey = np.ascontiguousarray(grey)
        p_raw, p_grey = raw.ctypes.data_as(up), grey.ctypes.data_as(up)
        dev0 = C.c_void_p()

        def run_a(orb=True):
            rc = fr.lib.tsframe_set_raw_image(fr.ctx, p_raw, w*ch, fmt, NL, None)
            assert rc == 0, fr.lib.tsframe_last_error(fr.ctx)
            if orb:
                fr.lib.tsframe_level_ptr(fr.ctx, 0, 0, C.byref(dev0))
                rc = ex_a.lib.tsorb_extract_device(ex_a.ctx, dev0, 1, w, h, w, out["a"][0].ctypes.data_as(fp), out["a"][1].ctypes.data_as(up), out["a"][2].ctypes.data_as(ip), cap)
                assert rc == 0, ex_a.lib.tsorb_last_error(ex_a.ctx)

        def run_b():
            rc = fr_b.lib.tsframe_set_image(fr_b.ctx, p_grey, w, h, NL)
            assert rc == 0, fr_b.lib.tsframe_last_error(fr_b.ctx)
            rc = ex_b.lib.tsorb_extract_batch(ex_b.ctx, p_grey, 1, w, h, w, out["b"][0].ctypes.data_as(fp), out["b"][1].ctypes.data_as(up), out["b"][2].ctypes.data_as(ip), cap)
            assert rc == 0, ex_b.lib.tsorb_last_error(ex_b.ctx)

        run_a(); run_b()
        n = int(out["a"][2][0])
        assert n == int(out["b"][2][0]) and n > 100 and out["a"][0][:n].tobytes() == out["b"][0][:n].tobytes() and out["a"][1][:n].tobytes() == out["b"][1][:n].tobytes()
        assert all(np.array_equal(fr.level(l, k), fr_b.level(l, k)) for l in range(NL) for k in range(4))
        ta, tb, tp = [], [], []
        for it in range(args.warmup + args.calls):
            t0 = time.perf_counter(); run_a(); t1 = time.perf_counter(); run_b(); t2 = time.perf_counter(); run_a(False); t3 = time.perf_counter()
            if it >= args.warmup:
                ta.append((t1 - t0)*1e6); tb.append((t2 - t1)*1e6); tp.append((t3 - t2)*1e6)
        r = float(np.median(ta)/np.median(tb)); ratios.append(("%d x %d %s" % (w, h, label), r))
        say("%-12s %-5s %9d | %-30s | %-30s | %7.3f | %-30s | %.1f (first %.1f)" % ("%d x %d" % (w, h), label, w*h*ch, q(ta), q(tb), r, q(tp), np.median(t_cam[1:]), t_cam[0]))
        if ex_a.lib.tsorb_debug_fallbacks(ex_a.ctx) or ex_b.lib.tsorb_debug_fallbacks(ex_b.ctx):
            say("%-12s %-5s (the ORB quadtree's serial pass ran in this row or an earlier one of this size: the ORB part is not the usual one)" % ("", label))
        say("%-12s %-5s (c) numpy restatement of remap + grey, map given, one run: %.0f us -- NOT OpenCV, no statement about cv::undistort's speed" % ("", label, t_np))
    ex_a.close(); ex_b.close()
say()
for name, r in ratios:
    say("%s: (a) / (b) = %.3f -- (a) is %s (b)" % (name, r, "ahead of" if r < 1.0 else "behind"))
say("(b) moves w * h bytes twice (614 KB at 640 x 480); (a) moves the raw frame once (921 KB for BGR, 307 KB for grey) and does the undistortion and the grey conversion that (b) leaves "
    "to the host, where they are not timed here")
if args.out != "/dev/null":
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
