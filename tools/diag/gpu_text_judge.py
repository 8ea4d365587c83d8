"""GPU diagnostic (not a pytest): tsframe_text_judge (tracking::TextJudgeSingle for a frame's planes, one launch) per call, for 1 / 8 / 32 planes of
~1000 - 2600 reference pixels (synth.text_judge_planes: the rendered planes, tiled), ZNCC on (TextJudge / SearchLocalObjs: 0.1 with detections, 0.8)
and off (TextUpdate: -3).  Median of warm calls, in ms; 'raw' = the C call through prebuilt ctypes arguments, 'py' = Frame.TextJudgeBatch.
TSFRAME_LIB = another build of libtsframe.so (e.g. -DJUDGE_CACHE=0) to compare."""
import ctypes as C
import os
import sys
import time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from textslam_amd import synth, frame                     # noqa: E402
import oracle                                              # noqa: E402

if os.environ.get("TSFRAME_LIB"):
    frame._LIBPATH = os.environ["TSFRAME_LIB"]
REPS = int(os.environ.get("TEXT_JUDGE_REPS", "200"))
S = synth.text_judge_planes(seed=3, n=8, tiny=False, huge=False)
pool = [i for i, k in enumerate(S["kind"]) if k in ("true", "perturbed", "oblique")]
fr = frame.Frame(0); fr.GetPyrMat(S["cur_img"], 4)
pix = []
for i in pool:
    u, v, I, _ = oracle.frame_box_pixels(S["ref_img"], S["quad"][i], 0.0, 1.0)
    pix.append((np.stack([u, v], 1).astype(np.int16), I.astype(np.uint8)))
print(f"library {os.path.relpath(frame._LIBPATH, ROOT)}; {REPS} warm calls per figure (median)")
dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
for N in (1, 8, 32):
    sel = [pool[k % len(pool)] for k in range(N)]
    pk = [pix[k % len(pool)] for k in range(N)]
    off = np.concatenate([[0], np.cumsum([len(p[1]) for p in pk])]).astype(np.int32)
    uv = np.ascontiguousarray(np.concatenate([p[0] for p in pk])); inten = np.ascontiguousarray(np.concatenate([p[1] for p in pk]))
    th = np.ascontiguousarray(S["theta"][sel]); T = np.ascontiguousarray(S["Tcr"][sel]).reshape(N, 12); ray = np.ascontiguousarray(S["box_ray"][sel])
    dete = np.ascontiguousarray(S["dete_xy"]); K = np.ascontiguousarray(S["K"])
    outs = [np.zeros(N, np.uint8), np.zeros(N, np.int32), np.zeros(N), np.zeros(N), np.zeros((N, 8)), np.zeros((N, (len(dete) + 31)//32), np.uint32)]
    for label, zmin, with_dete in (("zncc 0.1 + detections", 0.1, True), ("zncc 0.8", 0.8, False), ("zncc off", -3.0, False)):
        args = (fr.ctx, 0, N, dp(th), dp(T), dp(ray), off.ctypes.data_as(C.POINTER(C.c_int32)), uv.ctypes.data_as(C.POINTER(C.c_int16)),
                inten.ctypes.data_as(C.POINTER(C.c_uint8)), dp(K), dp(K), 0.0, 6, zmin, len(dete) if with_dete else 0, dp(dete) if with_dete else None,
                outs[0].ctypes.data_as(C.POINTER(C.c_uint8)), outs[1].ctypes.data_as(C.POINTER(C.c_int32)), dp(outs[2]), dp(outs[3]), dp(outs[4]),
                outs[5].ctypes.data_as(C.POINTER(C.c_uint32)) if with_dete else None)
        f = fr.lib.tsframe_text_judge
        for _ in range(10):
            assert f(*args) == 0
        tr = []
        for _ in range(REPS):
            t0 = time.perf_counter(); f(*args); tr.append((time.perf_counter() - t0)*1e3)
        tp = []
        for _ in range(max(REPS // 4, 10)):
            t0 = time.perf_counter()
            fr.TextJudgeBatch(0, th, S["Tcr"][sel], ray, off, uv, inten, K, K, 0.0, 6, zmin, dete if with_dete else None)
            tp.append((time.perf_counter() - t0)*1e3)
        print(f"N={N:2d}  pixels {int(off[-1]):6d}  {label:22s} raw {np.median(tr):.4f} ms (p10 {np.percentile(tr, 10):.4f}, p90 {np.percentile(tr, 90):.4f})"
              f"   py {np.median(tp):.4f} ms   pass {int(outs[0].sum())}/{N}")
