"""GPU diagnostic (not a pytest): what the text paths cost on images above 640 x 480, where a projected text box's fill mask takes more than one row band
(csrc/tsraster.h raster_quad_rows, csrc/tsquadstat.h quad_moments), and the judge's association tests points instead of building a mask.

One mid-sized window (8 keyframes x 600 points x 12 text planes, synth.camera) at 640 x 480, 1280 x 720 and 1920 x 1080.  At each size, host clock around the
call (every call ends in a stream synchronisation), median of --calls calls after a warm-up:
  tsba_local_ba one-shot, tsba_pose_optim one-shot on the window's newest keyframe (synth.window_of), tsba_text_label_image of the newest keyframe at level 0,
  tsframe_text_judge with detections (synth.text_judge_planes, ZNCC on), and a worst case for mu / sigma: the 5-keyframe tiny() window once as it is and once
  with EVERY plane's box over the whole frame (all four corners outside: every observation's histogram reads every pixel of its image, in every band) --
  the difference of the two local BAs, divided by the window's mu / sigma evaluations (observations x passes), is what one whole-frame box costs.
The one-shot calls include the upload of the window's images, which grows with the image; the table says how many bytes that is.
Writes the table to --out (default profiles/large_image_timing.txt).

    python tools/diag/gpu_large_images.py [--calls 30] [--out profiles/large_image_timing.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import oracle                                            # noqa: E402
from textslam_amd import synth, abi                      # noqa: E402
from textslam_amd.optimizer import Optimizer             # noqa: E402
from textslam_amd.frame import Frame                     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "large_image_timing.txt"))
args = ap.parse_args()

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def camera_K(w, h):
    fx, fy, cx, cy = synth.K_GENERAL_MOTION
    return np.array([fx*w/640.0, fy*w/640.0, cx*w/640.0, cy*h/480.0])


def timed(fn):
    t = []
    for it in range(args.warmup + args.calls):
        t0 = time.perf_counter(); fn(); t1 = time.perf_counter()
        if it >= args.warmup:
            t.append((t1 - t0)*1e3)
    return "%8.3f (%7.3f .. %7.3f)" % (np.median(t), np.percentile(t, 10), np.percentile(t, 90)), float(np.median(t))


def whole_frame_boxes(P, w, h):
    """P with every plane's box rays replaced by the frame's outline blown up by a third (host rays: the box covers every observer's image, corners outside)"""
    Q = P.copy()
    fx, fy, cx, cy = P.K
    uv = np.array([(-0.3*w, -0.3*h), (1.3*w, -0.3*h), (1.3*w, 1.3*h), (-0.3*w, 1.3*h)])
    ray = np.stack([(uv[:, 0] - cx)/fx, (uv[:, 1] - cy)/fy], 1)
    Q.text_box_ray = np.repeat(ray[None], P.n_text, 0)
    return Q.normalise()


g = Optimizer(0)
say("text paths by image size: host clock around the call, median of %d calls (p10 .. p90), milliseconds" % args.calls)
say("%-12s %-10s | %-28s | %-28s | %-28s | %-28s | %s" % ("size", "images MB", "local_ba one-shot", "pose_optim one-shot", "label_image (level 0)", "text_judge + detections",
                                                          "whole-frame mu / sigma"))
for w, h in ((640, 480), (1280, 720), (1920, 1080)):
    with synth.camera(w, h, camera_K(w, h)):
        P = synth.make_problem(8, 600, 12, 61, feats=(16, 8, 6))
        T = synth.tiny()
        S = synth.text_judge_planes(seed=3, n=8)
    o_l, o_p = abi.options_local(), abi.options_pose()
    mb = sum(P.img[l].nbytes for l in range(P.n_levels))/1e6
    c_local, _ = timed(lambda: g.LocalBundleAdjustment(P.copy(), options=o_l))
    Wd = synth.window_of(P, P.n_kf - 1, 1)
    c_pose, _ = timed(lambda: g.PoseOptim(Wd.copy(), options=o_p))
    g.LocalBundleAdjustment(P.copy(), options=o_l)
    c_label, _ = timed(lambda: g.TextLabelImage(P.n_kf - 1, 0, (h, w)))
    # judge
    off, uv, inten = [0], [], []
    for q in S["quad"]:
        u, v, I, _ = oracle.frame_box_pixels(S["ref_img"], q, 0.0, 1.0)
        uv.append(np.stack([u, v], 1)); inten.append(I.astype(np.uint8)); off.append(off[-1] + len(u))
    off, uv, inten = np.array(off, np.int32), np.concatenate(uv).astype(np.int16), np.concatenate(inten)
    fr = Frame(0); fr.GetPyrMat(S["cur_img"], 2)
    c_judge, _ = timed(lambda: fr.TextJudgeBatch(0, S["theta"], S["Tcr"], S["box_ray"], off, uv, inten, S["K"], S["K"], cos_min=0.0, out_margin=6, zncc_min=0.1,
                                                 dete_xy=S["dete_xy"]))
    # worst-case mu / sigma: the same small window with its own boxes and with whole-frame boxes
    Tw = whole_frame_boxes(T, w, h)
    _, m_own = timed(lambda: g.LocalBundleAdjustment(T.copy(), options=o_l))
    _, m_all = timed(lambda: g.LocalBundleAdjustment(Tw.copy(), options=o_l))
    n_eval = int((np.asarray(T.tobs_kf) != np.asarray(T.text_host)[T.tobs_text]).sum())*o_l.n_passes
    c_ms = "%.3f vs %.3f ms: %+.1f us per box (%d evaluations)" % (m_all, m_own, (m_all - m_own)*1e3/max(n_eval, 1), n_eval)
    say("%-12s %-10.1f | %-28s | %-28s | %-28s | %-28s | %s" % ("%d x %d" % (w, h), mb, c_local, c_pose, c_label, c_judge, c_ms))
say()
say("(Python call overhead -- ctypes, copies of the problem, the label image's allocation -- is inside every column.  Every size runs the same banded mask: one band per box at")
say(" 640 x 480 (and the judge's mask), several at level 0 of the larger sizes (1920 x 1080: levels 0 and 1), where the judge tests points.  The whole-frame column compares two")
say(" different solves -- the boxes change mu / sigma and with them the residuals -- so it bounds the cost of a box from above only loosely.)")
if args.out != "/dev/null":
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
