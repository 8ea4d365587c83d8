"""Host-side mirror of TextSLAM's ORBextractor (src/ORBextractor.h:48-88) over the C ABI of libtsorb.so (include/tsorb.h).

`ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)` and `__call__(image)` keep the reference's
constructor / operator() meaning; `extract_batch` is the batched form the GPU wants.  No CPU fallback."""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBPATH = os.environ.get("TSORB_LIB", os.path.join(_HERE, "libtsorb.so"))     # TSORB_LIB: instrumented build for diagnostics
_lib = None

EXPORTED_SYMBOLS = ["tsorb_create", "tsorb_destroy", "tsorb_last_error", "tsorb_get_levels", "tsorb_get_scale_factors",
                    "tsorb_get_features_per_level", "tsorb_extract_batch", "tsorb_upload", "tsorb_run", "tsorb_download",
                    "tsorb_debug_level", "tsorb_debug_fast_shape", "tsorb_debug_pyramid", "tsorb_debug_fallbacks", "tsorb_match_set_frame", "tsorb_match_set_features", "tsorb_match_search",
                    "tsorb_text_extract", "tsorb_match_brute_text", "tsorb_match_brute_scene", "tsorb_match_search_sets", "tsorb_match_pnp_ransac",
                    "tsorb_match_two_view_ransac", "tsorb_match_two_view_reconstruct", "tsorb_match_text_theta_ransac", "tsorb_match_search_claim",
                    "tsorb_match_new_points", "tsorb_upload_device", "tsorb_extract_device", "tsorb_fuse_frame"]
BRUTE_MAX_FEAT = 65536                                                  # TSORB_BRUTE_MAX_FEAT of include/tsorb.h
SETS_MAX = 1024                                                         # TSORB_SETS_MAX of include/tsorb.h
PNP_MAX_HYP = 128                                                       # TSORB_PNP_MAX_HYP of include/tsorb.h
PNP_MAX_POINTS = 65536                                                  # TSORB_PNP_MAX_POINTS of include/tsorb.h
TWOVIEW_MAX_HYP = 256                                                   # TSORB_TWOVIEW_MAX_HYP of include/tsorb.h
TWOVIEW_MAX_POINTS = 65536                                              # TSORB_TWOVIEW_MAX_POINTS of include/tsorb.h
TWOVIEW_REC_HYP = 8                                                     # TSORB_TWOVIEW_REC_HYP of include/tsorb.h
TEXT_THETA_MAX_FEAT = 1024                                              # TSORB_THETA_MAX_FEAT of include/tsorb.h
TEXT_THETA_MAX_HYP = 65536                                              # TSORB_THETA_MAX_HYP of include/tsorb.h


class TsorbError(RuntimeError):
    pass


def load_library():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIBPATH):
            raise TsorbError(f"{_LIBPATH} not found: build the HIP extension first")
        L = C.CDLL(_LIBPATH)
        vp, up, fp, ip = C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_int32)
        L.tsorb_create.argtypes = [C.POINTER(vp), C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int]
        L.tsorb_destroy.argtypes = [vp]
        L.tsorb_last_error.argtypes = [vp]; L.tsorb_last_error.restype = C.c_char_p
        L.tsorb_get_levels.argtypes = [vp]
        L.tsorb_get_scale_factors.argtypes = [vp, fp, fp]
        L.tsorb_get_features_per_level.argtypes = [vp, ip]
        L.tsorb_extract_batch.argtypes = [vp, up, C.c_int, C.c_int, C.c_int, C.c_int, fp, up, ip, C.c_int]
        L.tsorb_upload.argtypes = [vp, up, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        L.tsorb_upload_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        L.tsorb_upload_device.restype = C.c_int
        L.tsorb_extract_device.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, fp, up, ip, C.c_int]
        L.tsorb_extract_device.restype = C.c_int
        L.tsorb_run.argtypes = [vp]
        L.tsorb_download.argtypes = [vp, fp, up, ip]
        L.tsorb_debug_level.argtypes = [vp, C.c_int, C.c_int, C.c_int, up, ip, ip]
        L.tsorb_debug_fast_shape.argtypes = [vp, C.c_int]
        L.tsorb_debug_pyramid.argtypes = [vp, C.c_int]
        L.tsorb_debug_fallbacks.argtypes = [vp]
        L.tsorb_match_set_frame.argtypes = [vp, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double]
        L.tsorb_match_set_features.argtypes = [vp, fp, up, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double]
        L.tsorb_match_search.argtypes = [vp, C.c_int, fp, fp, ip, up, C.c_int, ip, ip, ip, ip, ip, ip]
        L.tsorb_text_extract.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int, C.c_int, fp, up, ip]
        L.tsorb_text_extract.restype = C.c_int
        dp = C.POINTER(C.c_double)
        L.tsorb_match_brute_text.argtypes = [vp, C.c_int, ip, up, ip, up, ip, ip, up]
        L.tsorb_match_brute_text.restype = C.c_int
        L.tsorb_match_brute_scene.argtypes = [vp, C.c_int, C.c_int, C.c_int, fp, up, up, C.c_int, ip, fp, up, up, ip, dp, dp, C.c_int, C.c_double, ip, ip]
        L.tsorb_match_brute_scene.restype = C.c_int
        L.tsorb_match_search_sets.argtypes = [vp, C.c_int, ip, fp, up, dp, C.c_int, up, C.c_int, ip, ip, fp, fp, ip, C.c_int, ip, ip, ip, ip, ip, ip]
        L.tsorb_match_search_sets.restype = C.c_int
        L.tsorb_match_pnp_ransac.argtypes = [vp, C.c_int, fp, fp, dp, C.c_int, ip, C.c_double, C.c_double, up, ip, dp, ip, dp]
        L.tsorb_match_pnp_ransac.restype = C.c_int
        L.tsorb_match_two_view_ransac.argtypes = [vp, C.c_int, fp, fp, fp, fp, C.c_int, ip, C.c_float, up, up, fp, fp, fp, ip, fp, fp]
        L.tsorb_match_two_view_ransac.restype = C.c_int
        L.tsorb_match_two_view_reconstruct.argtypes = [vp, C.c_int, fp, fp, up, C.c_int, fp, fp, C.c_float, C.c_float, C.c_int, ip, fp, fp, fp, up, ip, fp, fp, fp, up, fp]
        L.tsorb_match_two_view_reconstruct.restype = C.c_int
        L.tsorb_match_text_theta_ransac.argtypes = [vp, C.c_int, ip, fp, fp, dp, dp, dp, ip, ip, ip, dp, dp, fp, dp, dp, dp]
        L.tsorb_match_text_theta_ransac.restype = C.c_int
        L.tsorb_match_search_claim.argtypes = [vp, C.c_int, fp, fp, ip, up, up, C.c_int, C.c_int, C.c_double, ip, ip, ip]
        L.tsorb_match_search_claim.restype = C.c_int
        L.tsorb_match_new_points.argtypes = [vp, C.c_int, fp, fp, ip, up, up, C.c_int, C.c_int, C.c_double, fp, dp, dp, dp, C.c_int, ip, ip, fp, up, ip]
        L.tsorb_match_new_points.restype = C.c_int
        L.tsorb_fuse_frame.argtypes = [vp, C.c_int, C.c_int, dp, dp, C.c_double, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                                       fp, up, ip, ip, ip, ip, ip]
        L.tsorb_fuse_frame.restype = C.c_int
        _lib = L
    return _lib


class ORBextractor:
    def __init__(self, nfeatures=1000, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7, device=0):
        self.lib = load_library()
        self.ctx = C.c_void_p()
        rc = self.lib.tsorb_create(C.byref(self.ctx), nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, device)
        if rc != 0:
            raise TsorbError(f"tsorb_create failed with {rc}: no usable HIP device" if rc == -2 else f"tsorb_create failed with {rc}")
        self.nlevels, self.cap = nlevels, nfeatures + 8 * nlevels + 64
        self._shape = None

    def close(self):
        if self.ctx:
            self.lib.tsorb_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            msg = self.lib.tsorb_last_error(self.ctx)
            raise TsorbError(f"{what} failed with {rc}: {msg.decode() if msg else ''}")

    # getters of the reference class
    def GetLevels(self):
        return self.lib.tsorb_get_levels(self.ctx)

    def GetScaleFactors(self):
        sf = np.zeros(self.nlevels, np.float32)
        self._check(self.lib.tsorb_get_scale_factors(self.ctx, sf.ctypes.data_as(C.POINTER(C.c_float)), None), "tsorb_get_scale_factors")
        return sf

    def GetFeaturesPerLevel(self):
        n = np.zeros(self.nlevels, np.int32)
        self._check(self.lib.tsorb_get_features_per_level(self.ctx, n.ctypes.data_as(C.POINTER(C.c_int32))), "tsorb_get_features_per_level")
        return n

    def upload(self, imgs, stride=None):
        """imgs [n, h, w] uint8.  stride (default w): the images are the first w columns of an [n, h, stride] buffer -- a row-padded cv::Mat -- handed in as
        the view buf[:, :, :w]; the buffer goes to the library as it lies in memory, pad bytes included (no copy)."""
        if stride is None:
            imgs = np.ascontiguousarray(imgs, np.uint8)
        if imgs.ndim == 2:
            imgs = imgs[None]
        n, h, w = imgs.shape
        if stride is None:
            stride = w
        elif imgs.dtype != np.uint8 or imgs.strides[1:] != (stride, 1) or (n > 1 and imgs.strides[0] != h * stride):
            raise ValueError(f"imgs is not the first {w} columns of a uint8 [n, h, {stride}] buffer: strides {imgs.strides}")
        self._check(self.lib.tsorb_upload(self.ctx, C.cast(imgs.ctypes.data, C.POINTER(C.c_uint8)), n, w, h, int(stride), self.cap), "tsorb_upload")
        self._shape = (n, h, w)

    def upload_device(self, dev_ptr, n, h, w, stride=None):
        """upload() with the batch already on this extractor's device: dev_ptr = the device address (an int) of n frames of h rows of stride bytes,
        e.g. Frame.level_device_ptr(0) after Frame.SetRawImage (n = 1, stride = w).  The copy is complete when this returns."""
        stride = w if stride is None else stride
        self._check(self.lib.tsorb_upload_device(self.ctx, C.c_void_p(dev_ptr), int(n), int(w), int(h), int(stride), self.cap), "tsorb_upload_device")
        self._shape = (int(n), int(h), int(w))

    def extract_device(self, dev_ptr, n, h, w, stride=None):
        """extract_batch() with the batch already on this extractor's device (see upload_device), in one library call."""
        stride = w if stride is None else stride
        kp = np.zeros((n, self.cap, 6), np.float32); desc = np.zeros((n, self.cap, 32), np.uint8); cnt = np.zeros(n, np.int32)
        self._check(self.lib.tsorb_extract_device(self.ctx, C.c_void_p(dev_ptr), int(n), int(w), int(h), int(stride), kp.ctypes.data_as(C.POINTER(C.c_float)),
                                                  desc.ctypes.data_as(C.POINTER(C.c_uint8)), cnt.ctypes.data_as(C.POINTER(C.c_int32)), self.cap), "tsorb_extract_device")
        self._shape = (int(n), int(h), int(w))
        return [(kp[i, :cnt[i]].copy(), desc[i, :cnt[i]].copy()) for i in range(n)]

    def run(self):
        self._check(self.lib.tsorb_run(self.ctx), "tsorb_run")

    def download(self):
        n = self._shape[0]
        kp = np.zeros((n, self.cap, 6), np.float32)
        desc = np.zeros((n, self.cap, 32), np.uint8)
        cnt = np.zeros(n, np.int32)
        self._check(self.lib.tsorb_download(self.ctx, kp.ctypes.data_as(C.POINTER(C.c_float)), desc.ctypes.data_as(C.POINTER(C.c_uint8)),
                                            cnt.ctypes.data_as(C.POINTER(C.c_int32))), "tsorb_download")
        return [(kp[i, :cnt[i]].copy(), desc[i, :cnt[i]].copy()) for i in range(n)]

    def extract_batch(self, imgs, stride=None):
        """imgs [n, h, w] uint8 (stride: see upload) -> list of (keypoints [k, 6] = x, y, size, angle, response, octave ; descriptors [k, 32])."""
        self.upload(imgs, stride)
        self.run()
        return self.download()

    def __call__(self, image, mask=None):
        """ORBextractor::operator()(image, mask, keypoints, descriptors) -- the mask is ignored, as in the reference."""
        return self.extract_batch(image)[0]

    # ---- window / projection search (frame::GetFeaturesInArea + tracking::DescriptorDistance)
    def match_set_frame(self, frame, bounds):
        """Search in frame `frame` of the resident batch (features stay on the device); bounds = (mnMinX, mnMaxX, mnMinY, mnMaxY)."""
        self._check(self.lib.tsorb_match_set_frame(self.ctx, int(frame), *[float(b) for b in bounds]), "tsorb_match_set_frame")

    def match_set_features(self, kp6, desc, bounds):
        kp6 = np.ascontiguousarray(kp6, np.float32); desc = np.ascontiguousarray(desc, np.uint8)
        self._check(self.lib.tsorb_match_set_features(self.ctx, kp6.ctypes.data_as(C.POINTER(C.c_float)), desc.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                      kp6.shape[0], *[float(b) for b in bounds]), "tsorb_match_set_features")

    def match_search(self, qxy, qr, qlev, qdesc, max_cand=64):
        qxy = np.ascontiguousarray(qxy, np.float32); qr = np.ascontiguousarray(qr, np.float32); qdesc = np.ascontiguousarray(qdesc, np.uint8)
        nq = qxy.shape[0]
        qlev_p = None if qlev is None else np.ascontiguousarray(qlev, np.int32)
        ci = np.full((nq, max_cand), -1, np.int32); cd = np.full((nq, max_cand), -1, np.int32)
        cc = np.zeros(nq, np.int32); bi = np.zeros(nq, np.int32); bd = np.zeros(nq, np.int32); bd2 = np.zeros(nq, np.int32)
        ip_ = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        self._check(self.lib.tsorb_match_search(self.ctx, nq, qxy.ctypes.data_as(C.POINTER(C.c_float)), qr.ctypes.data_as(C.POINTER(C.c_float)),
                                                None if qlev_p is None else ip_(qlev_p), qdesc.ctypes.data_as(C.POINTER(C.c_uint8)), max_cand,
                                                ip_(ci), ip_(cd), ip_(cc), ip_(bi), ip_(bd), ip_(bd2)), "tsorb_match_search")
        return dict(cand_idx=ci, cand_dist=cd, cand_cnt=cc, best_idx=bi, best_dist=bd, best_dist2=bd2)

    # ---- text features (frame::FeatExtracText: cv::ORB detect on the masked frame + compute on the frame, docs/cvorb_recalled.md)
    def extract_text(self, frame, quads, nfeatures=500, cap=None):
        """Text features of frame `frame` of the resident batch for every detection quad in one call.  quads [n, 4, 2] (x, y in level-0 pixels).
        Returns a list of (keypoints [k, 6] = x, y, size, angle, Harris response, octave ; descriptors [k, 32]), one pair per detection: level-major,
        raster order inside a level.  cap = rows per detection (default: nfeatures + 64 for the ties a cut keeps); a detection with more raises."""
        quads = np.ascontiguousarray(quads, np.float64).reshape(-1, 4, 2)
        n = quads.shape[0]
        cap = int(nfeatures) + 64 if cap is None else int(cap)
        kp = np.zeros((n, max(cap, 1), 6), np.float32)
        desc = np.zeros((n, max(cap, 1), 32), np.uint8)
        cnt = np.zeros(max(n, 1), np.int32)
        self._check(self.lib.tsorb_text_extract(self.ctx, int(frame), n, quads.ctypes.data_as(C.POINTER(C.c_double)), int(nfeatures), cap,
                                                kp.ctypes.data_as(C.POINTER(C.c_float)), desc.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                cnt.ctypes.data_as(C.POINTER(C.c_int32))), "tsorb_text_extract")
        return [(kp[i, :cnt[i]].copy(), desc[i, :cnt[i]].copy()) for i in range(n)]

    # ---- the frame's searched set (frame::FeatExtract's boundary test + frame::FeatFusion + AssignFeaturesToGrid, docs/pointpolygon_recalled.md)
    def fuse_frame(self, frame, quads, bbox, bounds, win=-3.0, nfeatures=500, cap_text=None, cap=None):
        """The fused scene + text feature set of frame `frame` of the resident batch, left as the searched set of match_search / match_search_claim /
        match_new_points.  quads [n, 4, 2] = vTextDete, bbox [n, 4] = vTextDeteMin x, y, vTextDeteMax x, y, bounds = (mnMinX, mnMaxX, mnMinY, mnMaxY).
        cap_text = raw rows per detection (default nfeatures + 64), cap = fused rows (default: the extractor's rows per frame + n * cap_text).
        Returns a dict: kp [n, 6], desc [n, 32], obj [n] int32 (vTextObjInfo: -1 = scene), src [n] int32 (the row itself for a scene row, the index among the
        detection's raw keypoints for a text row), text_off [n_dete + 1] int32, raw_count [n_dete] int32, n_scene."""
        quads = np.ascontiguousarray(quads, np.float64).reshape(-1, 4, 2); bbox = np.ascontiguousarray(bbox, np.float64).reshape(-1, 4)
        nd = quads.shape[0]
        if bbox.shape[0] != nd:
            raise ValueError("quads and bbox have different lengths")
        cap_text = int(nfeatures) + 64 if cap_text is None else int(cap_text)
        cap = self.cap + nd * max(cap_text, 0) if cap is None else int(cap)
        kp = np.zeros((max(cap, 1), 6), np.float32); desc = np.zeros((max(cap, 1), 32), np.uint8)
        obj = np.zeros(max(cap, 1), np.int32); src = np.zeros(max(cap, 1), np.int32)
        off = np.zeros(nd + 1, np.int32); raw = np.zeros(max(nd, 1), np.int32); n_out = np.zeros(2, np.int32)
        ptr = lambda a, t: a.ctypes.data_as(C.POINTER(t)) if a.size else None
        self._check(self.lib.tsorb_fuse_frame(self.ctx, int(frame), nd, ptr(quads, C.c_double), ptr(bbox, C.c_double), float(win), int(nfeatures), cap_text, cap,
                                              *[float(b) for b in bounds], ptr(kp, C.c_float), ptr(desc, C.c_uint8), ptr(obj, C.c_int32), ptr(src, C.c_int32),
                                              ptr(off, C.c_int32), ptr(raw, C.c_int32), ptr(n_out, C.c_int32)), "tsorb_fuse_frame")
        n = int(n_out[1])
        return dict(kp=kp[:n].copy(), desc=desc[:n].copy(), obj=obj[:n].copy(), src=src[:n].copy(), text_off=off, raw_count=raw[:nd].copy(), n_scene=int(n_out[0]))

    # ---- loop closing's all-pairs matching (loopClosing::SearchMatch_Text / SearchMatch_Other), every loop candidate in one call
    def match_brute_text(self, pairs):
        """pairs: list of (desc1 [n1, 32], desc2 [n2, 32]), one per matched text pair of any candidate.  Returns per pair a dict train_idx [n1] int32
        (the nearest row of desc2, first index on a tie; -1 for an empty desc2), dist [n1] int32, good [n1] uint8 (dist < max(2 min_dist, 30.0))."""
        d1 = [np.ascontiguousarray(a, np.uint8).reshape(-1, 32) for a, _ in pairs]; d2 = [np.ascontiguousarray(b, np.uint8).reshape(-1, 32) for _, b in pairs]
        n = len(pairs)
        off1 = np.zeros(n + 1, np.int32); off2 = np.zeros(n + 1, np.int32)
        off1[1:] = np.cumsum([len(a) for a in d1]); off2[1:] = np.cumsum([len(b) for b in d2])
        a1 = np.concatenate(d1) if n else np.zeros((0, 32), np.uint8); a2 = np.concatenate(d2) if n else np.zeros((0, 32), np.uint8)
        nq = int(off1[n])
        ti = np.zeros(max(nq, 1), np.int32); di = np.zeros(max(nq, 1), np.int32); good = np.zeros(max(nq, 1), np.uint8)
        ip_ = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)); up_ = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
        a1 = np.ascontiguousarray(a1); a2 = np.ascontiguousarray(a2)
        self._check(self.lib.tsorb_match_brute_text(self.ctx, n, ip_(off1), up_(a1) if a1.size else None, ip_(off2), up_(a2) if a2.size else None,
                                                    ip_(ti), ip_(di), up_(good)), "tsorb_match_brute_text")
        return [dict(train_idx=ti[off1[p]:off1[p + 1]].copy(), dist=di[off1[p]:off1[p + 1]].copy(), good=good[off1[p]:off1[p + 1]].copy()) for p in range(n)]

    def match_brute_scene(self, w, h, xy1, desc1, has3d1, cands, th_low=50, ratio=0.9):
        """The current keyframe's features (xy1 [n1, 2], desc1 [n1, 32], has3d1 [n1]) against every loop candidate.  cands: list of dicts
        xy [n2, 2], desc [n2, 32], has3d [n2], quad_cur [nq, 4, 2], quad_can [nq, 4, 2] (the text boxes SearchMatch_Text painted for this candidate into
        the current keyframe's and the candidate's label image).  w, h: the label images' size.  Returns (match12 [n_cand, n1] int32, n_match [n_cand] int32)."""
        xy1 = np.ascontiguousarray(xy1, np.float32).reshape(-1, 2); desc1 = np.ascontiguousarray(desc1, np.uint8).reshape(-1, 32)
        has3d1 = np.ascontiguousarray(has3d1, np.uint8).reshape(-1)
        n1, nc = xy1.shape[0], len(cands)
        off2 = np.zeros(nc + 1, np.int32); qoff = np.zeros(nc + 1, np.int32)
        xy2 = [np.asarray(c["xy"], np.float32).reshape(-1, 2) for c in cands]
        qc = [np.asarray(c["quad_cur"], np.float64).reshape(-1, 4, 2) for c in cands]; qn = [np.asarray(c["quad_can"], np.float64).reshape(-1, 4, 2) for c in cands]
        off2[1:] = np.cumsum([len(a) for a in xy2]); qoff[1:] = np.cumsum([len(a) for a in qc])
        cat = lambda parts, shape, dt: np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(shape, dt), dt)
        xy2 = cat(xy2, (0, 2), np.float32)
        desc2 = cat([np.asarray(c["desc"], np.uint8).reshape(-1, 32) for c in cands], (0, 32), np.uint8)
        has3d2 = cat([np.asarray(c["has3d"], np.uint8).reshape(-1) for c in cands], (0,), np.uint8)
        qc = cat(qc, (0, 4, 2), np.float64); qn = cat(qn, (0, 4, 2), np.float64)
        m12 = np.zeros((max(nc, 1), max(n1, 1)), np.int32); nm = np.zeros(max(nc, 1), np.int32)
        ptr = lambda a, t: a.ctypes.data_as(C.POINTER(t)) if a.size else None
        self._check(self.lib.tsorb_match_brute_scene(self.ctx, int(w), int(h), n1, ptr(xy1, C.c_float), ptr(desc1, C.c_uint8), ptr(has3d1, C.c_uint8),
                                                     nc, ptr(off2, C.c_int32), ptr(xy2, C.c_float), ptr(desc2, C.c_uint8), ptr(has3d2, C.c_uint8),
                                                     ptr(qoff, C.c_int32), ptr(qc, C.c_double), ptr(qn, C.c_double), int(th_low), float(ratio),
                                                     ptr(m12, C.c_int32), ptr(nm, C.c_int32)), "tsorb_match_brute_scene")
        return m12[:nc, :n1].copy(), nm[:nc].copy()

    # ---- loop fusion's window searches (loopClosing::SearchAndFuse_Scene / MatchMore), every searched keyframe in one call
    def match_search_sets(self, sets, qset, qxy, qr, qdesc, qdi=None, qlev=None, max_cand=0):
        """sets: list of (kp6 [n, 6], desc [n, 32], bounds = (mnMinX, mnMaxX, mnMinY, mnMaxY)), one per searched keyframe.  Query q searches sets[qset[q]] at qxy[q] with
        radius qr[q] and descriptor qdesc[qdi[q]] (qdi None: qdesc[q]); qlev [nq, 2] or None = no level check.  Returns match_search's dictionary, indices relative to
        the query's set: what match_set_features(*sets[qset[q]]) + match_search of that one query returns."""
        kps = [np.ascontiguousarray(k, np.float32).reshape(-1, 6) for k, _, _ in sets]; ds = [np.ascontiguousarray(d, np.uint8).reshape(-1, 32) for _, d, _ in sets]
        ns = len(sets)
        foff = np.zeros(ns + 1, np.int32); foff[1:] = np.cumsum([len(k) for k in kps])
        kp = np.ascontiguousarray(np.concatenate(kps) if ns else np.zeros((0, 6), np.float32)); desc = np.ascontiguousarray(np.concatenate(ds) if ns else np.zeros((0, 32), np.uint8))
        bounds = np.ascontiguousarray([[float(v) for v in b] for _, _, b in sets], np.float64).reshape(-1, 4)
        qset = np.ascontiguousarray(qset, np.int32).reshape(-1); qxy = np.ascontiguousarray(qxy, np.float32).reshape(-1, 2); qr = np.ascontiguousarray(qr, np.float32).reshape(-1)
        qdesc = np.ascontiguousarray(qdesc, np.uint8).reshape(-1, 32)
        qdi_p = None if qdi is None else np.ascontiguousarray(qdi, np.int32).reshape(-1); qlev_p = None if qlev is None else np.ascontiguousarray(qlev, np.int32).reshape(-1, 2)
        nq = qxy.shape[0]
        ci = np.full((nq, max_cand), -1, np.int32); cd = np.full((nq, max_cand), -1, np.int32)
        cc = np.zeros(nq, np.int32); bi = np.zeros(nq, np.int32); bd = np.zeros(nq, np.int32); bd2 = np.zeros(nq, np.int32)
        ptr = lambda a, t: None if a is None or a.size == 0 else a.ctypes.data_as(C.POINTER(t))
        self._check(self.lib.tsorb_match_search_sets(self.ctx, ns, ptr(foff, C.c_int32), ptr(kp, C.c_float), ptr(desc, C.c_uint8), ptr(bounds, C.c_double),
                                                     qdesc.shape[0], ptr(qdesc, C.c_uint8), nq, ptr(qset, C.c_int32), ptr(qdi_p, C.c_int32), ptr(qxy, C.c_float), ptr(qr, C.c_float),
                                                     ptr(qlev_p, C.c_int32), int(max_cand), ptr(ci, C.c_int32), ptr(cd, C.c_int32), ptr(cc, C.c_int32), ptr(bi, C.c_int32),
                                                     ptr(bd, C.c_int32), ptr(bd2, C.c_int32)), "tsorb_match_search_sets")
        return dict(cand_idx=ci, cand_dist=cd, cand_cnt=cc, best_idx=bi, best_dist=bd, best_dist2=bd2)

    # ---- the outlier gate before PoseOptim (tracking::CheckMatch: cv::solvePnPRansac with EPnP, docs/pnpransac_recalled.md)
    def match_pnp_ransac(self, Pw, uv, K, subsets, reproj_err=5.0, confidence=0.98):
        """Pw [n, 3] world points and uv [n, 2] keypoints of the matches (floats), K = (fx, fy, cx, cy), subsets [H, 5]: the hypotheses' matches, drawn by the caller.
        Returns a dict: ok, n_inlier, sel (-1: none), n_run of the reference's loop, inlier [n] bool (the kept hypothesis' mask), pose [3, 4] = R | t of the kept
        hypothesis, and of EVERY hypothesis hyp_count [H] int32 and hyp_pose [H, 3, 4]."""
        Pw = np.ascontiguousarray(Pw, np.float32).reshape(-1, 3); uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        K = np.ascontiguousarray(K, np.float64).reshape(4); subsets = np.ascontiguousarray(subsets, np.int32).reshape(-1, 5)
        n, H = Pw.shape[0], subsets.shape[0]
        inl = np.zeros(max(n, 1), np.uint8); res = np.zeros(4, np.int32); pose = np.zeros(12, np.float64)
        hc = np.zeros(max(H, 1), np.int32); hp = np.zeros((max(H, 1), 12), np.float64)
        ptr = lambda a, t: a.ctypes.data_as(C.POINTER(t)) if a.size else None
        self._check(self.lib.tsorb_match_pnp_ransac(self.ctx, n, ptr(Pw, C.c_float), ptr(uv, C.c_float), ptr(K, C.c_double), H, ptr(subsets, C.c_int32),
                                                    float(reproj_err), float(confidence), ptr(inl, C.c_uint8), ptr(res, C.c_int32), ptr(pose, C.c_double),
                                                    ptr(hc, C.c_int32), ptr(hp, C.c_double)), "tsorb_match_pnp_ransac")
        return dict(ok=bool(res[0]), n_inlier=int(res[1]), sel=int(res[2]), n_run=int(res[3]), inlier=inl[:n].astype(bool), pose=pose.reshape(3, 4),
                    hyp_count=hc[:H].copy(), hyp_pose=hp[:H].reshape(H, 3, 4).copy())

    # ---- the two-view initializer's RANSAC (initializer::FindHomography + FindFundamental, docs/twoview_recalled.md)
    def match_two_view_ransac(self, xy1, xy2, norm1, norm2, subset, sigma=1.0):
        """xy1, xy2 [n, 2] the matched keypoints of frame 1 / frame 2 (floats), norm1, norm2 = (meanX, meanY, sX, sY) of initializer::Normalize over ALL keypoints of
        each frame, subset [H, 8]: the hypotheses' matches, drawn by the caller.  Returns a dict: sel [2] int32 (kept H / F hypothesis, -1: none), score [2] float32
        (SH, SF), H21, F21 [3, 3] float32, inlier_h, inlier_f [n] bool, and of EVERY hypothesis hyp_score [2, H] float32 and hyp_model [2, H, 3, 3] float32 (H first)."""
        xy1 = np.ascontiguousarray(xy1, np.float32).reshape(-1, 2); xy2 = np.ascontiguousarray(xy2, np.float32).reshape(-1, 2)
        norm1 = np.ascontiguousarray(norm1, np.float32).reshape(4); norm2 = np.ascontiguousarray(norm2, np.float32).reshape(4)
        subset = np.ascontiguousarray(subset, np.int32).reshape(-1, 8)
        n, H = xy1.shape[0], subset.shape[0]
        if xy2.shape[0] != n:
            raise ValueError("xy1 and xy2 have different lengths")
        ih = np.zeros(max(n, 1), np.uint8); jf = np.zeros(max(n, 1), np.uint8); H21 = np.zeros(9, np.float32); F21 = np.zeros(9, np.float32)
        score = np.zeros(2, np.float32); sel = np.zeros(2, np.int32); hs = np.zeros((2, max(H, 1)), np.float32); hm = np.zeros((2, max(H, 1), 9), np.float32)
        ptr = lambda a, t: a.ctypes.data_as(C.POINTER(t)) if a.size else None
        self._check(self.lib.tsorb_match_two_view_ransac(self.ctx, n, ptr(xy1, C.c_float), ptr(xy2, C.c_float), ptr(norm1, C.c_float), ptr(norm2, C.c_float), H,
                                                         ptr(subset, C.c_int32), float(sigma), ptr(ih, C.c_uint8), ptr(jf, C.c_uint8), ptr(H21, C.c_float), ptr(F21, C.c_float),
                                                         ptr(score, C.c_float), ptr(sel, C.c_int32), ptr(hs, C.c_float), ptr(hm, C.c_float)), "tsorb_match_two_view_ransac")
        return dict(sel=sel, score=score, H21=H21.reshape(3, 3), F21=F21.reshape(3, 3), inlier_h=ih[:n].astype(bool), inlier_f=jf[:n].astype(bool),
                    hyp_score=hs[:, :H].copy(), hyp_model=hm[:, :H].reshape(2, H, 3, 3).copy())

    # ---- the two-view initializer's reconstruction (initializer::ReconstructH / ReconstructF with CheckRT, docs/twoview_reconstruct_recalled.md)
    def match_two_view_reconstruct(self, xy1, xy2, inlier, model, M21, K, sigma=1.0, min_parallax=1.0, min_triangulated=50):
        """xy1, xy2 [n, 2] the matched keypoints (floats), inlier [n] the chosen model's vbMatchesInliers, model 0: M21 is H21, 1: M21 is F21 ([3, 3] floats),
        K = (fx, fy, cx, cy).  Returns a dict: ok, sel (-1: none), result [6] int32 (ok, sel, N, best nGood, second best nGood / nsimilar, exit bits), R21 [3, 3], t21 [3],
        p3d [n, 3] float32 and triangulated [n] bool of the kept hypothesis (per match; zeros when nothing is kept), and of EVERY hypothesis hyp_good [8] int32, hyp_cos [8],
        hyp_parallax [8] float32, hyp_pose [8, 3, 4] = R | t, hyp_state [8, n] uint8 (the exit each match took) and hyp_p3d [8, n, 3] float32."""
        xy1 = np.ascontiguousarray(xy1, np.float32).reshape(-1, 2); xy2 = np.ascontiguousarray(xy2, np.float32).reshape(-1, 2)
        inlier = np.ascontiguousarray(np.asarray(inlier).reshape(-1) != 0, np.uint8)
        M21 = np.ascontiguousarray(M21, np.float32).reshape(9); K = np.ascontiguousarray(K, np.float32).reshape(4)
        n, H = xy1.shape[0], TWOVIEW_REC_HYP
        if xy2.shape[0] != n or inlier.shape[0] != n:
            raise ValueError("xy1, xy2 and inlier have different lengths")
        m = max(n, 1)
        res = np.zeros(6, np.int32); R21 = np.zeros(9, np.float32); t21 = np.zeros(3, np.float32); p3d = np.zeros((m, 3), np.float32); tri = np.zeros(m, np.uint8)
        hg = np.zeros(H, np.int32); hc = np.zeros(H, np.float32); hp = np.zeros(H, np.float32); pose = np.zeros((H, 12), np.float32)
        hs = np.zeros((H, m), np.uint8); hx = np.zeros((H, m, 3), np.float32)
        ptr = lambda a, t: a.ctypes.data_as(C.POINTER(t)) if a.size else None
        self._check(self.lib.tsorb_match_two_view_reconstruct(self.ctx, n, ptr(xy1, C.c_float), ptr(xy2, C.c_float), ptr(inlier, C.c_uint8), int(model), ptr(M21, C.c_float),
                                                              ptr(K, C.c_float), float(sigma), float(min_parallax), int(min_triangulated), ptr(res, C.c_int32),
                                                              ptr(R21, C.c_float), ptr(t21, C.c_float), ptr(p3d, C.c_float), ptr(tri, C.c_uint8), ptr(hg, C.c_int32),
                                                              ptr(hc, C.c_float), ptr(hp, C.c_float), ptr(pose, C.c_float), ptr(hs, C.c_uint8), ptr(hx, C.c_float)),
                    "tsorb_match_two_view_reconstruct")
        return dict(ok=bool(res[0]), sel=int(res[1]), result=res, R21=R21.reshape(3, 3), t21=t21, p3d=p3d[:n], triangulated=tri[:n].astype(bool), hyp_good=hg, hyp_cos=hc,
                    hyp_parallax=hp, hyp_pose=pose.reshape(H, 3, 4), hyp_state=hs[:, :n].copy(), hyp_p3d=hx[:, :n].copy())

    # ---- the planes of new text detections (tracking::GetTextTheta / initializer::CalculateTextTheta, docs/texttheta_recalled.md)
    def match_text_theta_ransac(self, off, host_xy, targ_xy, Tcr, K, hyp_off, triple, rho=None):
        """off [P+1] the planes' feature ranges, host_xy / targ_xy [N, 2] the features in the host keyframe and the target frame (floats), Tcr [3, 4] (or [4, 4]) = R | t host ->
        target and K = (fx, fy, cx, cy) in double, hyp_off [P+1] the planes' hypothesis ranges, triple [H, 3] feature indices within the plane in the order drawn;
        rho [N] the inverse depths, or None: triangulated on the device.  Returns a dict: sel [P] int32 (-1: none), theta [P, 3] and score [P] of the kept hypothesis,
        p3d [N, 3] float32 (zeros when rho is given), rho [N] the rho that was used, and of EVERY hypothesis hyp_score [H] and hyp_theta [H, 3]."""
        off = np.ascontiguousarray(off, np.int32).reshape(-1); hyp_off = np.ascontiguousarray(hyp_off, np.int32).reshape(-1)
        host_xy = np.ascontiguousarray(host_xy, np.float32).reshape(-1, 2); targ_xy = np.ascontiguousarray(targ_xy, np.float32).reshape(-1, 2)
        triple = np.ascontiguousarray(triple, np.int32).reshape(-1, 3)
        Tcr = np.ascontiguousarray(np.asarray(Tcr, np.float64).reshape(-1, 4)[:3]).reshape(12); K = np.ascontiguousarray(K, np.float64).reshape(4)
        P = off.shape[0] - 1
        if P < 0 or hyp_off.shape[0] != P + 1:
            raise ValueError("off and hyp_off have different lengths")
        N, H = host_xy.shape[0], triple.shape[0]
        if targ_xy.shape[0] != N or (P > 0 and (int(off[-1]) != N or int(hyp_off[-1]) != H)):
            raise ValueError("host_xy, targ_xy or triple does not have the length off / hyp_off give")
        if rho is not None:
            rho = np.ascontiguousarray(rho, np.float64).reshape(-1)
            if rho.shape[0] != N:
                raise ValueError("rho and host_xy have different lengths")
        sel = np.full(max(P, 1), -1, np.int32); theta = np.zeros((max(P, 1), 3)); score = np.zeros(max(P, 1))
        p3d = np.zeros((max(N, 1), 3), np.float32); rho_out = np.zeros(max(N, 1)); hs = np.zeros(max(H, 1)); ht = np.zeros((max(H, 1), 3))
        ptr = lambda a, t: a.ctypes.data_as(C.POINTER(t)) if a is not None and a.size else None
        self._check(self.lib.tsorb_match_text_theta_ransac(self.ctx, P, ptr(off, C.c_int32), ptr(host_xy, C.c_float), ptr(targ_xy, C.c_float), ptr(rho, C.c_double),
                                                           ptr(Tcr, C.c_double), ptr(K, C.c_double), ptr(hyp_off, C.c_int32), ptr(triple, C.c_int32), ptr(sel, C.c_int32),
                                                           ptr(theta, C.c_double), ptr(score, C.c_double), ptr(p3d, C.c_float), ptr(rho_out, C.c_double),
                                                           ptr(hs, C.c_double), ptr(ht, C.c_double)), "tsorb_match_text_theta_ransac")
        return dict(sel=sel[:P], theta=theta[:P], score=score[:P], p3d=p3d[:N], rho=rho_out[:N], hyp_score=hs[:H], hyp_theta=ht[:H])

    # ---- the stateful window searches (tracking::SearchForTriangular / SearchForInitializ, GetForTriangular + CheckTriangular; docs/newpoints_recalled.md)
    def _claim_args(self, qxy, qr, qlev, qdesc, elig2):
        qxy = np.ascontiguousarray(qxy, np.float32).reshape(-1, 2); qr = np.ascontiguousarray(qr, np.float32).reshape(-1); qdesc = np.ascontiguousarray(qdesc, np.uint8).reshape(-1, 32)
        qlev = None if qlev is None else np.ascontiguousarray(qlev, np.int32).reshape(-1, 2)
        elig2 = None if elig2 is None else np.ascontiguousarray(np.asarray(elig2).reshape(-1) != 0, np.uint8)
        nq = qxy.shape[0]
        if qr.shape[0] != nq or qdesc.shape[0] != nq or (qlev is not None and qlev.shape[0] != nq):
            raise ValueError("qxy, qr, qlev and qdesc have different lengths")
        return nq, qxy, qr, qlev, qdesc, elig2

    def match_search_claim(self, qxy, qr, qlev, qdesc, elig2=None, th_low=50, use_ratio=False, ratio=0.9):
        """The reference's claim chain over the queries in order against the current grid (match_set_frame / match_set_features): qxy [nq, 2], qr [nq], qlev [nq, 2] or
        None, qdesc [nq, 32]; elig2 [n2] (non-zero = may be matched) or None = all.  SearchForTriangular: the defaults with qr = 80*1.2f and qlev = (octave, octave);
        SearchForInitializ: use_ratio=True.  Returns a dict: match12 [nq] int32 (-1 = none), match_dist [nq] int32 (-1 = none), n_match."""
        nq, qxy, qr, qlev, qdesc, elig2 = self._claim_args(qxy, qr, qlev, qdesc, elig2)
        m12 = np.full(max(nq, 1), -1, np.int32); md = np.full(max(nq, 1), -1, np.int32); nm = np.zeros(1, np.int32)
        ptr = lambda a, t: a.ctypes.data_as(C.POINTER(t)) if a is not None and a.size else None
        self._check(self.lib.tsorb_match_search_claim(self.ctx, nq, ptr(qxy, C.c_float), ptr(qr, C.c_float), ptr(qlev, C.c_int32), ptr(qdesc, C.c_uint8), ptr(elig2, C.c_uint8),
                                                      int(th_low), int(bool(use_ratio)), float(ratio), ptr(m12, C.c_int32), ptr(md, C.c_int32), ptr(nm, C.c_int32)),
                    "tsorb_match_search_claim")
        return dict(match12=m12[:nq], match_dist=md[:nq], n_match=int(nm[0]))

    def match_new_points(self, qxy, qr, qlev, qdesc, q_px, Trw, Tcw, K, elig2=None, th_low=50, use_ratio=False, ratio=0.9, th_reproj=9):
        """match_search_claim, then GetForTriangular's point and CheckTriangular's verdict of every match in the same call: q_px [nq, 2] the queries' pixels in the
        keyframe, Trw / Tcw [3, 4] (or [4, 4]) the keyframe's and the frame's pose, K = (fx, fy, cx, cy) in double.  Returns a dict: match12 [nq] int32, n_match,
        p3d [nq, 3] float32 and good [nq] bool per query (zeros without a match), n_good."""
        nq, qxy, qr, qlev, qdesc, elig2 = self._claim_args(qxy, qr, qlev, qdesc, elig2)
        q_px = np.ascontiguousarray(q_px, np.float32).reshape(-1, 2)
        if q_px.shape[0] != nq:
            raise ValueError("q_px and qxy have different lengths")
        Trw = np.ascontiguousarray(np.asarray(Trw, np.float64).reshape(-1, 4)[:3]).reshape(12); Tcw = np.ascontiguousarray(np.asarray(Tcw, np.float64).reshape(-1, 4)[:3]).reshape(12)
        K = np.ascontiguousarray(K, np.float64).reshape(4)
        m12 = np.full(max(nq, 1), -1, np.int32); cnt = np.zeros(2, np.int32); p3d = np.zeros((max(nq, 1), 3), np.float32); good = np.zeros(max(nq, 1), np.uint8)
        ptr = lambda a, t: a.ctypes.data_as(C.POINTER(t)) if a is not None and a.size else None
        self._check(self.lib.tsorb_match_new_points(self.ctx, nq, ptr(qxy, C.c_float), ptr(qr, C.c_float), ptr(qlev, C.c_int32), ptr(qdesc, C.c_uint8), ptr(elig2, C.c_uint8),
                                                    int(th_low), int(bool(use_ratio)), float(ratio), ptr(q_px, C.c_float), ptr(Trw, C.c_double), ptr(Tcw, C.c_double),
                                                    ptr(K, C.c_double), int(th_reproj), ptr(m12, C.c_int32), ptr(cnt[0:1], C.c_int32), ptr(p3d, C.c_float), ptr(good, C.c_uint8),
                                                    ptr(cnt[1:2], C.c_int32)), "tsorb_match_new_points")
        return dict(match12=m12[:nq], n_match=int(cnt[0]), p3d=p3d[:nq], good=good[:nq].astype(bool), n_good=int(cnt[1]))

    def debug_fast_shape(self, shape=-1):
        """Diagnostics: the shape of the FAST launches (include/tsorb.h); -1 = chosen by the batch size."""
        self._check(self.lib.tsorb_debug_fast_shape(self.ctx, int(shape)), "tsorb_debug_fast_shape")

    def debug_pyramid(self, shape=-1):
        """Diagnostics: how the pyramid is formed (include/tsorb.h): 0 a launch per level, 1 every level from the input image in one launch, -1 by the batch size."""
        self._check(self.lib.tsorb_debug_pyramid(self.ctx, int(shape)), "tsorb_debug_pyramid")

    def debug_fallbacks(self):
        """Runs of this extractor that took the serial quadtree pass (include/tsorb.h)."""
        return int(self.lib.tsorb_debug_fallbacks(self.ctx))

    def debug_level(self, frame, level, blurred=False):
        n, h, w = self._shape
        out = np.zeros((h + 38) * (w + 38), np.uint8)
        lw, lh = C.c_int32(0), C.c_int32(0)
        self._check(self.lib.tsorb_debug_level(self.ctx, frame, level, int(blurred), out.ctypes.data_as(C.POINTER(C.c_uint8)),
                                               C.byref(lw), C.byref(lh)), "tsorb_debug_level")
        if blurred:
            return out[:lw.value * lh.value].reshape(lh.value, lw.value).copy()
        return out[:(lw.value + 38) * (lh.value + 38)].reshape(lh.value + 38, lw.value + 38).copy()


def synthetic_frame(seed, w=640, h=480):
    """Seeded test frame: flat rectangles, discs and noise (corners at every contrast and scale)."""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 100.0)
    for _ in range(120):
        x0, y0 = rng.integers(0, w), rng.integers(0, h)
        ww, hh = rng.integers(8, 80), rng.integers(8, 60)
        img[y0:y0 + hh, x0:x0 + ww] = rng.uniform(20, 235)
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(60):
        cx, cy, r = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(3, 25)
        img[(xx - cx) ** 2 + (yy - cy) ** 2 < r * r] = rng.uniform(10, 245)
    img += rng.normal(0, 3, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)
