"""Host-side mirror of the reference's BA-pyramid / reference-feature construction on the MI355X (libtsframe.so, include/tsframe.h).

  Frame.GetPyrMat(img, iScaleLevels)                  frame::GetPyrMat          /root/reference/src/frame.cc:178-204
  Frame.GetPyramidPts(...) / GetPyramidPtsScene(...)  tool::GetPyramidPts       /root/reference/src/tool.cc:564-710, 862-980
  Frame.GetPyramidPtsBatch(sets, vInvScalefactor)     the loop of frame::TextFeaProc src/frame.cc:359-370 (+ the scene set), one launch
  Frame.CalNormvec(level, uv, mu, std)                tool::CalNormvec          /root/reference/src/tool.cc:1342-1364 (GetNeighbour INTERVAL8)
  Frame.GetBoxAllPixs(level, vTextDete, mu, std, K)   tool::GetBoxAllPixs       /root/reference/src/tool.cc:1264-1337
  Frame.TextJudgeBatch(...)                           tracking::TextJudgeSingle /root/reference/src/tracking.cc:1991-2131 (n planes, one launch)
  Frame.TrackKLT(prev_frame, pts, ...)                tracking::TrackNewTextFeat /root/reference/src/tracking.cc:1752-1785 (all points, one launch)
  Frame.GetObjectInfoBatch(quads, inv_scale, feats)   mapText::GetObjectInfo    src/mapText.cc:64-107 (all new objects, one launch)
  Frame.SetCamera(w, h, K, dist) / SetRawImage(raw)   cv::undistort + cvtColor + GetPyrMat   main.cpp:73, src/tracking.cc:69-73 (one upload per camera frame)

No CPU fallback: without the HIP library / a GPU every call raises.
"""
import ctypes as C
import os
import re
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBPATH = os.path.join(_HERE, "libtsframe.so")
EXPORTED_SYMBOLS = ["tsframe_create", "tsframe_destroy", "tsframe_last_error", "tsframe_set_image", "tsframe_level_size", "tsframe_level_ptr",
                    "tsframe_get_level", "tsframe_pyramid_pts", "tsframe_pyramid_pts_batch", "tsframe_neighbours", "tsframe_box_pixels", "tsframe_text_judge", "tsframe_klt_track",
                    "tsframe_text_object_info", "tsframe_set_camera", "tsframe_set_raw_image", "tsframe_get_undist_map"]
IMG, GRAD, GRADX, GRADY = 0, 1, 2, 3
RAW_BGR, RAW_RGB, RAW_GREY = 0, 1, 2                                     # TSFRAME_RAW_* of include/tsframe.h
JUDGE_PASS, JUDGE_ORIENT, JUDGE_DEPTH, JUDGE_BOX, JUDGE_ZNCC = 0, 1, 2, 3, 4


def _csrc_define(header, name):
    text = open(os.path.join(_HERE, "csrc", header)).read()
    return int(re.search(r"^#define\s+%s\s+(\d+)" % name, text, re.M).group(1))


# cells of a (set, level) grid that tsframe_pyramid_pts_batch keeps in LDS; a larger grid goes to the device scratch (csrc/tspts.h)
PTS_LDS_CELLS = _csrc_define("tspts.h", "PTS_LDS_CELLS")


class FrameError(RuntimeError):
    pass


def _load():
    if not os.path.exists(_LIBPATH):
        raise FrameError("libtsframe.so is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = C.CDLL(_LIBPATH)
    vp, dp, ip, up = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    L.tsframe_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.tsframe_destroy.argtypes = [vp]; L.tsframe_destroy.restype = None
    L.tsframe_last_error.argtypes = [vp]; L.tsframe_last_error.restype = C.c_char_p
    L.tsframe_set_image.argtypes = [vp, up, C.c_int, C.c_int, C.c_int]
    L.tsframe_level_size.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.tsframe_level_ptr.argtypes = [vp, C.c_int, C.c_int, C.POINTER(vp)]
    L.tsframe_get_level.argtypes = [vp, C.c_int, C.c_int, up]
    L.tsframe_pyramid_pts.argtypes = [vp, C.c_int, C.POINTER(C.c_float), C.c_int, dp, dp, ip, dp, dp, ip, dp, up]
    L.tsframe_pyramid_pts_batch.argtypes = [vp, C.c_int, ip, ip, C.POINTER(C.c_float), dp, dp, ip, dp, dp, ip, dp, up]
    L.tsframe_pyramid_pts_batch.restype = C.c_int
    L.tsframe_neighbours.argtypes = [vp, C.c_int, dp, C.c_int, C.c_double, C.c_double, dp, dp, up]
    L.tsframe_box_pixels.argtypes = [vp, C.c_int, dp, C.c_double, C.c_double, C.c_int, ip, ip, ip, dp, dp]
    L.tsframe_text_judge.argtypes = [vp, C.c_int, C.c_int, dp, dp, dp, ip, C.POINTER(C.c_int16), up, dp, dp, C.c_double, C.c_int, C.c_double,
                                     C.c_int, dp, up, ip, dp, dp, dp, C.POINTER(C.c_uint32)]
    L.tsframe_text_judge.restype = C.c_int
    L.tsframe_klt_track.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_float), up]
    L.tsframe_klt_track.restype = C.c_int
    L.tsframe_text_object_info.argtypes = [vp, C.c_int, dp, dp, ip, ip, dp, dp, dp, C.c_int, dp, up, dp, dp, dp, up, ip, ip, ip, dp, dp]
    L.tsframe_text_object_info.restype = C.c_int
    L.tsframe_set_camera.argtypes = [vp, C.c_int, C.c_int, dp, dp, dp]
    L.tsframe_set_camera.restype = C.c_int
    L.tsframe_set_raw_image.argtypes = [vp, up, C.c_int, C.c_int, C.c_int, up]
    L.tsframe_set_raw_image.restype = C.c_int
    L.tsframe_get_undist_map.argtypes = [vp, C.POINTER(C.c_int16), C.POINTER(C.c_uint16)]
    L.tsframe_get_undist_map.restype = C.c_int
    return L


def _dp(a): return a.ctypes.data_as(C.POINTER(C.c_double))
def _up(a): return a.ctypes.data_as(C.POINTER(C.c_uint8))


class Frame:
    """The image side of a `frame` / `keyframe`: pyramid and gradient planes resident in HBM."""

    def __init__(self, device: int = 0):
        self.lib = _load()
        self.ctx = C.c_void_p()
        rc = self.lib.tsframe_create(device, C.byref(self.ctx))
        if rc != 0:
            raise FrameError("tsframe_create failed (%d): no usable GPU %d" % (rc, device))
        self.n_levels = 0

    def __del__(self):
        if getattr(self, "ctx", None) and self.ctx:
            self.lib.tsframe_destroy(self.ctx); self.ctx = None

    def _check(self, rc, what):
        if rc != 0:
            raise FrameError("%s failed (%d): %s" % (what, rc, self.lib.tsframe_last_error(self.ctx).decode()))

    def GetPyrMat(self, img, iScaleLevels: int):
        img = np.ascontiguousarray(img, np.uint8)
        self._check(self.lib.tsframe_set_image(self.ctx, _up(img), img.shape[1], img.shape[0], iScaleLevels), "tsframe_set_image")
        self.n_levels = iScaleLevels

    def SetCamera(self, w, h, K, dist, K_new=None):
        """cv::undistort's map for a w x h camera, built and kept on the device (include/tsframe.h: tsframe_set_camera).  K, K_new = (fx, fy, cx, cy),
        dist = (k1, k2, p1, p2, k3); K_new None: K."""
        K = np.ascontiguousarray(K, np.float64).reshape(4); dist = np.ascontiguousarray(dist, np.float64).reshape(5)
        Kn = None if K_new is None else np.ascontiguousarray(K_new, np.float64).reshape(4)
        self._check(self.lib.tsframe_set_camera(self.ctx, int(w), int(h), _dp(K), _dp(dist), _dp(Kn) if Kn is not None else None), "tsframe_set_camera")
        self.camera_shape = (int(h), int(w))

    def SetRawImage(self, raw, fmt, iScaleLevels: int, want_undistorted=False):
        """One raw camera frame -> undistorted, grey, BA pyramid (include/tsframe.h: tsframe_set_raw_image).  raw: uint8 [h, w, 3] (RAW_BGR / RAW_RGB) or
        [h, w] (RAW_GREY) of the camera's size; a row-padded image is handed in as the view buf[:, :w] of its buffer and goes to the library as it lies in
        memory (no copy).  Returns the undistorted image in raw's channel order when want_undistorted, else None."""
        ch = 1 if fmt == RAW_GREY else 3
        h, w = raw.shape[:2]
        if raw.dtype != np.uint8 or raw.shape != ((h, w) if ch == 1 else (h, w, 3)) or (h, w) != getattr(self, "camera_shape", (h, w)):
            raise ValueError("raw is not a uint8 image of the camera's size with %d channel(s): shape %s" % (ch, raw.shape))
        if raw.strides[1:] != ((1,) if ch == 1 else (3, 1)) or raw.strides[0] < w*ch:
            raw = np.ascontiguousarray(raw)
        out = np.zeros(raw.shape, np.uint8) if want_undistorted else None
        self._check(self.lib.tsframe_set_raw_image(self.ctx, C.cast(raw.ctypes.data, C.POINTER(C.c_uint8)), int(raw.strides[0]), int(fmt), int(iScaleLevels),
                                                   _up(out) if out is not None else None), "tsframe_set_raw_image")
        self.n_levels = iScaleLevels
        return out

    def undist_map(self):
        """Test hook: the resident map as cv::initUndistortRectifyMap(CV_16SC2) leaves it: (xy int16 [h, w, 2], frac uint16 [h, w])."""
        h, w = getattr(self, "camera_shape", (1, 1))
        xy = np.zeros((h, w, 2), np.int16); frac = np.zeros((h, w), np.uint16)
        self._check(self.lib.tsframe_get_undist_map(self.ctx, xy.ctypes.data_as(C.POINTER(C.c_int16)), frac.ctypes.data_as(C.POINTER(C.c_uint16))),
                    "tsframe_get_undist_map")
        return xy, frac

    def level_shape(self, level):
        w, h = C.c_int(0), C.c_int(0)
        self._check(self.lib.tsframe_level_size(self.ctx, level, C.byref(w), C.byref(h)), "tsframe_level_size")
        return h.value, w.value

    def level(self, level, which=IMG):
        out = np.zeros(self.level_shape(level), np.uint8)
        self._check(self.lib.tsframe_get_level(self.ctx, level, which, _up(out)), "tsframe_get_level")
        return out

    def level_device_ptr(self, level, which=IMG) -> int:
        p = C.c_void_p()
        self._check(self.lib.tsframe_level_ptr(self.ctx, level, which, C.byref(p)), "tsframe_level_ptr")
        return p.value

    def _pts(self, mode, xy, box, inv_scale):
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2); n = len(xy); nl = self.n_levels; cap = max(1, n*nl)
        inv = np.ascontiguousarray(inv_scale, np.float64); assert len(inv) == nl
        bx = np.ascontiguousarray(box, np.float64) if box is not None else None
        off = np.zeros(nl + 1, np.int32); u = np.zeros(cap); v = np.zeros(cap); idx = np.zeros(cap, np.int32); I = np.zeros(cap); inn = np.zeros(cap, np.uint8)
        self._check(self.lib.tsframe_pyramid_pts(self.ctx, mode, xy.ctypes.data_as(C.POINTER(C.c_float)), n, _dp(bx) if bx is not None else None, _dp(inv),
                                                 off.ctypes.data_as(C.POINTER(C.c_int32)), _dp(u), _dp(v), idx.ctypes.data_as(C.POINTER(C.c_int32)), _dp(I), _up(inn)),
                    "tsframe_pyramid_pts")
        m = int(off[nl])
        return {"level_off": off, "u": u[:m], "v": v[:m], "idx": idx[:m], "inten": I[:m], "in": inn[:m]}

    def GetPyramidPts(self, vObvRaw, PMin, PMax, vInvScalefactor):
        """Text features of one detection box: vObvRaw = keypoint (x, y) at level 0."""
        return self._pts(0, vObvRaw, [PMin[0], PMin[1], PMax[0], PMax[1]], vInvScalefactor)

    def GetPyramidPtsScene(self, vObvRaw, vInvScalefactor):
        return self._pts(1, vObvRaw, None, vInvScalefactor)

    def GetPyramidPtsBatch(self, sets, vInvScalefactor):
        """tool::GetPyramidPts for every feature set of the frame in one launch (include/tsframe.h: tsframe_pyramid_pts_batch).
        sets = [(mode, xy, box-or-None)]: mode 0 = text (box = (PMin.x, PMin.y, PMax.x, PMax.y)), 1 = scene.  Returns one dict per set, the same
        as GetPyramidPts / GetPyramidPtsScene give for that set alone."""
        ns = len(sets); nl = self.n_levels
        inv = np.ascontiguousarray(vInvScalefactor, np.float64); assert len(inv) == nl
        xys = [np.ascontiguousarray(s[1], np.float32).reshape(-1, 2) for s in sets]
        mode = np.array([s[0] for s in sets], np.int32).reshape(ns)
        off = np.zeros(ns + 1, np.int32); off[1:] = np.cumsum([len(a) for a in xys])
        xy = np.concatenate(xys) if ns else np.zeros((0, 2), np.float32)
        box = np.zeros((max(ns, 1), 4)); tot = int(off[ns]); cap = max(1, tot*nl)
        for i, s in enumerate(sets):
            if s[2] is not None:
                box[i] = np.asarray(s[2], np.float64).reshape(4)
        lo = np.zeros((max(ns, 1), nl + 1), np.int32); u = np.zeros(cap); v = np.zeros(cap); idx = np.zeros(cap, np.int32); I = np.zeros(cap); inn = np.zeros(cap, np.uint8)
        ip = C.POINTER(C.c_int32)
        self._check(self.lib.tsframe_pyramid_pts_batch(self.ctx, ns, mode.ctypes.data_as(ip), off.ctypes.data_as(ip), xy.ctypes.data_as(C.POINTER(C.c_float)), _dp(box),
                                                       _dp(inv), lo.ctypes.data_as(ip), _dp(u), _dp(v), idx.ctypes.data_as(ip), _dp(I), _up(inn)),
                    "tsframe_pyramid_pts_batch")
        out = []
        for i in range(ns):
            b = int(off[i])*nl; e = b + int(lo[i, nl])
            out.append({"level_off": lo[i].copy(), "u": u[b:e], "v": v[b:e], "idx": idx[b:e], "inten": I[b:e], "in": inn[b:e]})
        return out

    def CalNormvec(self, level, uv, mu, std):
        """Returns (neighbourInten [n, 8], neighbourNInten [n, 8], IN [n]); std == 0 raises (the reference returns false)."""
        uv = np.ascontiguousarray(uv, np.float64).reshape(-1, 2); n = len(uv)
        I = np.zeros((n, 8)); N = np.zeros((n, 8)); inn = np.zeros(n, np.uint8)
        self._check(self.lib.tsframe_neighbours(self.ctx, level, _dp(uv), n, float(mu), float(std), _dp(I), _dp(N), _up(inn)), "tsframe_neighbours")
        return I, N, inn

    def GetBoxAllPixs(self, level, vTextDete, mu, std, K=None):
        """All pixels of the level image inside the detection quad vTextDete (4 x (x, y)); returns a dict with u, v (int32), featureInten,
        featureNInten and -- when K = (fx, fy, cx, cy) is given -- ray [n, 3]; entry i has IdxToRaw = i, level 0, IN = True."""
        quad = np.ascontiguousarray(vTextDete, np.float64).reshape(4, 2)
        ip = C.POINTER(C.c_int32); n = C.c_int32(0)
        self._check(self.lib.tsframe_box_pixels(self.ctx, level, _dp(quad), float(mu), float(std), 0, C.byref(n), None, None, None, None), "tsframe_box_pixels")
        m = n.value; cap = max(1, m)
        u = np.zeros(cap, np.int32); v = np.zeros(cap, np.int32); I = np.zeros(cap); N = np.zeros(cap)
        if m > 0:
            self._check(self.lib.tsframe_box_pixels(self.ctx, level, _dp(quad), float(mu), float(std), cap, C.byref(n), u.ctypes.data_as(ip), v.ctypes.data_as(ip),
                                                    _dp(I), _dp(N)), "tsframe_box_pixels")
        out = {"u": u[:m], "v": v[:m], "featureInten": I[:m], "featureNInten": N[:m]}
        if K is not None:
            fx, fy, cx, cy = K
            out["ray"] = np.stack([(out["u"] - cx)/fx, (out["v"] - cy)/fy, np.ones(m)], 1)
        return out

    def TextJudgeBatch(self, level, theta, Tcr, box_ray, pix_off, pix_uv, pix_inten, K_ref, K, cos_min=0.0, out_margin=6, zncc_min=0.1,
                       dete_xy=None):
        """tracking::TextJudgeSingle for n planes on this frame's level image in one launch (include/tsframe.h: tsframe_text_judge).
        theta [n, 3]; Tcr [n, 3, 4] (or [n, 4, 4]: the top three rows); box_ray [n, 4, 2]; the reference pixels in CSR: pix_off [n + 1],
        pix_uv [m, 2] (level-0 u, v), pix_inten [m]; K_ref, K = (fx, fy, cx, cy).  dete_xy [n_dete, 2] or None (the 4-argument overload).
        Returns a dict of pass (bool), reason (JUDGE_*), cos, zncc, box_uv [n, 4, 2] and, with dete_xy, dete [n, n_dete] (bool) and the raw
        dete_bits [n, (n_dete + 31) // 32]."""
        theta = np.ascontiguousarray(theta, np.float64).reshape(-1, 3); n = len(theta)
        T = np.asarray(Tcr, np.float64).reshape(n, -1, 4)[:, :3, :]
        T = np.ascontiguousarray(T).reshape(n, 12)
        ray = np.ascontiguousarray(box_ray, np.float64).reshape(n, 8)
        off = np.ascontiguousarray(pix_off, np.int32).reshape(-1); assert len(off) == n + 1
        uv = np.ascontiguousarray(pix_uv, np.int16).reshape(-1, 2); I = np.ascontiguousarray(pix_inten, np.uint8).reshape(-1)
        Kr = np.ascontiguousarray(K_ref, np.float64).reshape(4); Kc = np.ascontiguousarray(K, np.float64).reshape(4)
        nd = 0 if dete_xy is None else len(dete_xy)
        dxy = None if dete_xy is None else np.ascontiguousarray(dete_xy, np.float64).reshape(nd, 2)
        words = (nd + 31)//32
        m = max(n, 1)
        ok = np.zeros(m, np.uint8); reason = np.zeros(m, np.int32); cs = np.zeros(m); zn = np.zeros(m); box = np.zeros((m, 8))
        bits = np.zeros((m, max(words, 1)), np.uint32)
        self._check(self.lib.tsframe_text_judge(self.ctx, level, n, _dp(theta), _dp(T), _dp(ray), off.ctypes.data_as(C.POINTER(C.c_int32)),
                                                uv.ctypes.data_as(C.POINTER(C.c_int16)), _up(I), _dp(Kr), _dp(Kc), float(cos_min), int(out_margin),
                                                float(zncc_min), nd, _dp(dxy) if dxy is not None else None, _up(ok),
                                                reason.ctypes.data_as(C.POINTER(C.c_int32)), _dp(cs), _dp(zn), _dp(box),
                                                bits.ctypes.data_as(C.POINTER(C.c_uint32)) if dxy is not None else None), "tsframe_text_judge")
        out = {"pass": ok[:n].astype(bool), "reason": reason[:n], "cos": cs[:n], "zncc": zn[:n], "box_uv": box[:n].reshape(n, 4, 2)}
        if dxy is not None:
            b = bits[:n, :words]
            out["dete_bits"] = b
            j = np.arange(nd)
            out["dete"] = ((b[:, j // 32] >> (j % 32).astype(np.uint32)) & 1).astype(bool) if nd else np.zeros((n, 0), bool)
        return out

    def TrackKLT(self, prev_frame, pts, win=21, max_level=3, max_iter=30, eps=0.01, min_eig=1e-4):
        """cv::calcOpticalFlowPyrLK(prev_frame, this frame, pts) on the two resident pyramids in one launch (include/tsframe.h: tsframe_klt_track;
        the arithmetic is docs/klt_recalled.md).  pts [n, 2] float32 level-0 positions in prev_frame, all detections concatenated.
        Returns (next_xy float32 [n, 2], status uint8 [n])."""
        xy = np.ascontiguousarray(pts, np.float32).reshape(-1, 2); n = len(xy)
        nxt = np.zeros((max(n, 1), 2), np.float32); st = np.zeros(max(n, 1), np.uint8)
        fp = C.POINTER(C.c_float)
        self._check(self.lib.tsframe_klt_track(prev_frame.ctx, self.ctx, n, xy.ctypes.data_as(fp), int(win), int(max_level), int(max_iter), float(eps),
                                               float(min_eig), nxt.ctypes.data_as(fp), _up(st)), "tsframe_klt_track")
        return nxt[:n], st[:n]

    def GetObjectInfoBatch(self, quads, vInvScalefactor, feats, K=None):
        """mapText::GetObjectInfo for every new text object of the keyframe in one launch (include/tsframe.h: tsframe_text_object_info).
        quads [n, 4, 2] = vTextDete (level-0 corners); feats = one dict per object as GetPyramidPtsBatch returns it (level_off, u, v, inten are read).
        Returns one dict per object: statistics [L, 2] (mu, sigma), ok [L], and per feature (the order of feats[i]) featureNInten, neighbourInten [m, 8],
        neighbourNInten [m, 8], IN; vRefPixs = the level-0 box pixels as GetBoxAllPixs returns them (with ray when K = (fx, fy, cx, cy) is given).
        The pixel capacity is the sum of the clamped level-0 boxes, so one call does it."""
        nl = self.n_levels
        q = np.ascontiguousarray(quads, np.float64).reshape(-1, 4, 2); n = len(q); assert len(feats) == n
        inv = np.ascontiguousarray(vInvScalefactor, np.float64); assert len(inv) == nl
        if n == 0:
            return []
        lo = np.ascontiguousarray([f["level_off"] for f in feats], np.int32).reshape(n, nl + 1)
        cnt = [int(r[nl]) for r in lo]
        foff = np.zeros(n + 1, np.int32); foff[1:] = np.cumsum([(c + nl - 1)//nl for c in cnt])      # the smallest slices that hold the features
        cap = max(1, int(foff[n])*nl)
        u = np.zeros(cap); v = np.zeros(cap); I = np.zeros(cap)
        for i, f in enumerate(feats):
            b = int(foff[i])*nl
            u[b:b + cnt[i]] = f["u"][:cnt[i]]; v[b:b + cnt[i]] = f["v"][:cnt[i]]; I[b:b + cnt[i]] = f["inten"][:cnt[i]]
        h0, w0 = self.level_shape(0)
        c0 = q*inv[0]
        x0 = np.clip(np.floor(c0[:, :, 0].min(1)), 0, w0 - 1); x1 = np.clip(np.ceil(c0[:, :, 0].max(1)), 0, w0 - 1)
        y0 = np.clip(np.floor(c0[:, :, 1].min(1)), 0, h0 - 1); y1 = np.clip(np.ceil(c0[:, :, 1].max(1)), 0, h0 - 1)
        pcap = max(1, int(np.sum((x1 - x0 + 1)*(y1 - y0 + 1))))
        ms = np.zeros((n, nl, 2)); ok = np.zeros((n, nl), np.uint8)
        N = np.zeros(cap); I8 = np.zeros((cap, 8)); N8 = np.zeros((cap, 8)); inn = np.zeros(cap, np.uint8)
        poff = np.zeros(n + 1, np.int32); pu = np.zeros(pcap, np.int32); pv = np.zeros(pcap, np.int32); pI = np.zeros(pcap); pN = np.zeros(pcap)
        ip = C.POINTER(C.c_int32)
        self._check(self.lib.tsframe_text_object_info(self.ctx, n, _dp(q), _dp(inv), foff.ctypes.data_as(ip), lo.ctypes.data_as(ip), _dp(u), _dp(v), _dp(I), pcap,
                                                      _dp(ms), _up(ok), _dp(N), _dp(I8), _dp(N8), _up(inn),
                                                      poff.ctypes.data_as(ip), pu.ctypes.data_as(ip), pv.ctypes.data_as(ip), _dp(pI), _dp(pN)),
                    "tsframe_text_object_info")
        out = []
        for i in range(n):
            b = int(foff[i])*nl; e = b + cnt[i]; a, z = int(poff[i]), int(poff[i + 1])
            pix = {"u": pu[a:z], "v": pv[a:z], "featureInten": pI[a:z], "featureNInten": pN[a:z]}
            if K is not None:
                fx, fy, cx, cy = K
                pix["ray"] = np.stack([(pix["u"] - cx)/fx, (pix["v"] - cy)/fy, np.ones(z - a)], 1)
            out.append({"statistics": ms[i].copy(), "ok": ok[i].astype(bool), "level_off": lo[i].copy(), "featureNInten": N[b:e],
                        "neighbourInten": I8[b:e], "neighbourNInten": N8[b:e], "IN": inn[b:e], "vRefPixs": pix})
        return out
