"""Host-side mirror of the reference's loop-closure optimisers on the MI355X (libtsloop.so, include/tsloop.h).

  LoopOptimizer.OptimizeSim3(...)     optimizer::OptimizeSim3     /root/reference/src/optimizer.cc:626-731
  LoopOptimizer.OptimizeLoop(...)     optimizer::OptimizeLoop     /root/reference/src/optimizer.cc:733-957 (the solve; the map update stays with the caller)
  LoopOptimizer.Sim3Batch(...)        Sim3Solver::iterate + optimizer::OptimizeSim3 of every loop candidate, one launch (src/Sim3Solver.cc:59-253)
  LoopOptimizer.DetectLoop(...)       loopClosing::DetectLoop: the string scan, the match lists, the vote and the candidates (src/loopClosing.cc:119-304)

No CPU fallback: without the HIP library / a GPU every call raises.
"""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBPATH = os.path.join(_HERE, "libtsloop.so")
EXPORTED_SYMBOLS = ["tsloop_default_options_sim3", "tsloop_default_options_loop", "tsloop_create", "tsloop_destroy", "tsloop_last_error",
                    "tsloop_optimize_sim3", "tsloop_optimize_loop", "tsloop_default_options_sim3_ransac", "tsloop_sim3_batch",
                    "tsloop_default_options_detect", "tsloop_detect_loop"]
RANSAC_MAX_HYP = 64                    # TSLOOP_RANSAC_MAX_HYP
TEXT_MAX_LEN = 64                      # TSLOOP_TEXT_MAX_LEN


class TsloopOptions(C.Structure):
    _fields_ = [("max_it", C.c_int32), ("pad", C.c_int32), ("huber_delta", C.c_double), ("thresh_outlier", C.c_double),
                ("initial_radius", C.c_double), ("max_radius", C.c_double), ("min_radius", C.c_double), ("min_relative_decrease", C.c_double),
                ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double), ("parameter_tolerance", C.c_double),
                ("min_diagonal", C.c_double), ("max_diagonal", C.c_double)]


class TsloopReport(C.Structure):
    _fields_ = [("iters", C.c_int32), ("accepted", C.c_int32), ("termination", C.c_int32), ("n_inlier", C.c_int32),
                ("cost0", C.c_double), ("cost1", C.c_double), ("t_ms", C.c_double)]


class TsloopSim3Problem(C.Structure):
    _fields_ = [("n", C.c_int32), ("pad", C.c_int32), ("P1", C.POINTER(C.c_double)), ("P2", C.POINTER(C.c_double)),
                ("uv1", C.POINTER(C.c_float)), ("uv2", C.POINTER(C.c_float)), ("inlier", C.POINTER(C.c_uint8)),
                ("K", C.c_double*4), ("sim", C.c_double*8)]


class TsloopGraphProblem(C.Structure):
    _fields_ = [("n_kf", C.c_int32), ("n_edge", C.c_int32), ("pose", C.POINTER(C.c_double)), ("fixed", C.POINTER(C.c_uint8)),
                ("edge_i", C.POINTER(C.c_int32)), ("edge_j", C.POINTER(C.c_int32)), ("meas", C.POINTER(C.c_double))]


class TsloopSim3BatchProblem(C.Structure):
    _fields_ = [("n_cand", C.c_int32), ("optimise", C.c_int32),
                ("off", C.POINTER(C.c_int32)), ("hyp_off", C.POINTER(C.c_int32)), ("triple", C.POINTER(C.c_int32)),
                ("P1", C.POINTER(C.c_double)), ("P2", C.POINTER(C.c_double)), ("pred1", C.POINTER(C.c_double)), ("pred2", C.POINTER(C.c_double)),
                ("uv1", C.POINTER(C.c_float)), ("uv2", C.POINTER(C.c_float)), ("K2", C.POINTER(C.c_double)),
                ("K1", C.c_double*4), ("K", C.c_double*4), ("min_inliers", C.c_int32), ("pad", C.c_int32), ("max_err2", C.c_double),
                ("ok", C.POINTER(C.c_uint8)), ("sel", C.POINTER(C.c_int32)), ("n_inlier_ransac", C.POINTER(C.c_int32)),
                ("sim_ransac", C.POINTER(C.c_double)), ("sim", C.POINTER(C.c_double)), ("rep", C.POINTER(TsloopReport)),
                ("inlier", C.POINTER(C.c_uint8)), ("hyp_count", C.POINTER(C.c_int32)), ("hyp_sim", C.POINTER(C.c_double))]


def make_sim3_batch_problem(cands, K1, K, optimise=True, min_inliers=20, max_err2=45.0, fill=None):
    """cands: per candidate a dict(P1 [n,3], P2, pred1 [n,2], pred2, uv1, uv2, triples [H,3], K2 [4]).  Returns (struct, arrays): arrays holds the flat inputs
    and the outputs the struct points at.  fill = (byte, int32, float64): what the outputs hold before the call (tests look for what is left untouched)."""
    nc = len(cands)
    cat = lambda key, dt, w: np.ascontiguousarray(np.concatenate([np.asarray(c[key], dt).reshape(-1, w) for c in cands]) if nc else np.zeros((0, w), dt))
    A = {"P1": cat("P1", np.float64, 3), "P2": cat("P2", np.float64, 3), "pred1": cat("pred1", np.float64, 2), "pred2": cat("pred2", np.float64, 2),
         "uv1": cat("uv1", np.float32, 2), "uv2": cat("uv2", np.float32, 2), "triple": cat("triples", np.int32, 3), "K2": cat("K2", np.float64, 4)}
    ns = [len(np.asarray(c["P1"]).reshape(-1, 3)) for c in cands]; hs = [len(np.asarray(c["triples"]).reshape(-1, 3)) for c in cands]
    for c, n in zip(cands, ns):
        assert all(np.asarray(c[key]).size == n*w for key, w in (("P2", 3), ("pred1", 2), ("pred2", 2), ("uv1", 2), ("uv2", 2)))
    A["off"] = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32); A["hyp_off"] = np.concatenate([[0], np.cumsum(hs)]).astype(np.int32)
    n, nh = int(A["off"][-1]), int(A["hyp_off"][-1])
    fb, fi, fd = fill if fill is not None else (0, 0, 0.0)
    A["ok"] = np.full(nc, fb, np.uint8); A["sel"] = np.full(nc, fi, np.int32); A["n_inlier_ransac"] = np.full(nc, fi, np.int32)
    A["sim_ransac"] = np.full((nc, 8), fd); A["sim"] = np.full((nc, 8), fd); A["inlier"] = np.full(n, fb, np.uint8)
    A["hyp_count"] = np.full(nh, fi, np.int32); A["hyp_sim"] = np.full((nh, 8), fd)
    A["rep"] = (TsloopReport*max(nc, 1))()
    if fill is not None:
        C.memset(A["rep"], fb, C.sizeof(A["rep"]))
    p = TsloopSim3BatchProblem()
    p.n_cand = nc; p.optimise = 1 if optimise else 0; p.min_inliers = int(min_inliers); p.max_err2 = float(max_err2)
    for k in range(4):
        p.K1[k] = float(K1[k]); p.K[k] = float(K[k])
    for name, ct in (("off", C.c_int32), ("hyp_off", C.c_int32), ("triple", C.c_int32), ("P1", C.c_double), ("P2", C.c_double), ("pred1", C.c_double),
                     ("pred2", C.c_double), ("uv1", C.c_float), ("uv2", C.c_float), ("K2", C.c_double), ("ok", C.c_uint8), ("sel", C.c_int32),
                     ("n_inlier_ransac", C.c_int32), ("sim_ransac", C.c_double), ("sim", C.c_double), ("inlier", C.c_uint8), ("hyp_count", C.c_int32),
                     ("hyp_sim", C.c_double)):
        setattr(p, name, A[name].ctypes.data_as(C.POINTER(ct)))
    p.rep = C.cast(A["rep"], C.POINTER(TsloopReport))
    return p, A


class TsloopDetectProblem(C.Structure):
    _fields_ = [("n_query", C.c_int32), ("n_map", C.c_int32), ("n_kf", C.c_int32), ("top_n", C.c_int32),
                ("q_off", C.POINTER(C.c_int32)), ("q_str", C.POINTER(C.c_uint8)), ("q_self", C.POINTER(C.c_int32)),
                ("m_off", C.POINTER(C.c_int32)), ("m_str", C.POINTER(C.c_uint8)), ("m_skip", C.POINTER(C.c_uint8)),
                ("obs_off", C.POINTER(C.c_int32)), ("obs_kf", C.POINTER(C.c_int32)),
                ("min_str_score", C.c_double), ("score_thresh_min", C.c_double), ("min_matched_words", C.c_int32), ("max_match", C.c_int32),
                ("match_cnt", C.POINTER(C.c_int32)), ("match_idx", C.POINTER(C.c_int32)), ("match_dist", C.POINTER(C.c_int32)),
                ("match_score", C.POINTER(C.c_double)), ("kf_score", C.POINTER(C.c_int32)), ("kf_nobj", C.POINTER(C.c_int32)),
                ("n_cand", C.POINTER(C.c_int32)), ("cand", C.POINTER(C.c_int32))]


def _flat_bytes(strings):
    """bytes-like strings -> ([n + 1] int32 offsets, uint8 bytes; one spare byte so that the array is never empty)."""
    bs = [bytes(x) for x in strings]
    off = np.concatenate([[0], np.cumsum([len(b) for b in bs], dtype=np.int64)]).astype(np.int32)
    return off, np.frombuffer(b"".join(bs) + b"\0", np.uint8).copy()


def make_detect_problem(queries, q_self, map_texts, m_skip, obs_rows, n_kf, min_matched_words=1, score_thresh_min=0.51, min_str_score=0.3, top_n=10,
                        max_match=64, fill=None):
    """queries / map_texts: bytes per text (textCur.mean / TextMean.mean);  q_self [n_query]: the map index of a query's own object or -1;  m_skip [n_map]:
    1 = TEXTBAD;  obs_rows: per map text the eligible keyframes that observe it, as increasing indices in [0, n_kf).  Returns (struct, arrays): arrays holds the
    flat inputs and the outputs the struct points at.  fill = (int32, float64): what the outputs hold before the call."""
    nq, nm = len(queries), len(map_texts)
    assert len(q_self) == nq and len(m_skip) == nm and len(obs_rows) == nm
    A = {}
    A["q_off"], A["q_str"] = _flat_bytes(queries); A["m_off"], A["m_str"] = _flat_bytes(map_texts)
    A["q_self"] = np.ascontiguousarray(q_self, np.int32).reshape(nq).copy(); A["m_skip"] = np.ascontiguousarray(m_skip, np.uint8).reshape(nm).copy()
    A["m_skip"] = np.concatenate([A["m_skip"], np.zeros(1, np.uint8)]); A["q_self"] = np.concatenate([A["q_self"], np.zeros(1, np.int32)])      # (never empty)
    A["obs_off"] = np.concatenate([[0], np.cumsum([len(r) for r in obs_rows], dtype=np.int64)]).astype(np.int32)
    A["obs_kf"] = np.concatenate([np.asarray(r, np.int32).reshape(-1) for r in obs_rows] + [np.zeros(1, np.int32)]).astype(np.int32)
    fi, fd = fill if fill is not None else (0, 0.0)
    mm = max(int(max_match), 1)
    A["match_cnt"] = np.full(max(nq, 1), fi, np.int32); A["match_idx"] = np.full((max(nq, 1), mm), fi, np.int32); A["match_dist"] = np.full((max(nq, 1), mm), fi, np.int32)
    A["match_score"] = np.full((max(nq, 1), mm), fd, np.float64); A["kf_score"] = np.full(max(int(n_kf), 1), fi, np.int32); A["kf_nobj"] = np.full(max(int(n_kf), 1), fi, np.int32)
    A["n_cand"] = np.full(1, fi, np.int32); A["cand"] = np.full(max(int(top_n), 1), fi, np.int32)
    p = TsloopDetectProblem()
    p.n_query = nq; p.n_map = nm; p.n_kf = int(n_kf); p.top_n = int(top_n); p.max_match = int(max_match); p.min_matched_words = int(min_matched_words)
    p.min_str_score = float(min_str_score); p.score_thresh_min = float(score_thresh_min)
    for name, ct in TsloopDetectProblem._fields_:
        if name in A:
            setattr(p, name, A[name].ctypes.data_as(ct))
    return p, A


def detect_result(p, A):
    """The outputs of a tsloop_detect_loop call as a dict: per query the match list (idx, dist, score arrays; None for a list that did not fit max_match)."""
    nq, nk = p.n_query, p.n_kf
    cnt = A["match_cnt"][:nq].copy()
    fits = [int(n) <= p.max_match for n in cnt]
    nc = int(A["n_cand"][0])
    return {"match_cnt": cnt,
            "match_idx": [A["match_idx"][q, :cnt[q]].copy() if fits[q] else None for q in range(nq)],
            "match_dist": [A["match_dist"][q, :cnt[q]].copy() if fits[q] else None for q in range(nq)],
            "match_score": [A["match_score"][q, :cnt[q]].copy() if fits[q] else None for q in range(nq)],
            "kf_score": A["kf_score"][:nk].copy(), "kf_nobj": A["kf_nobj"][:nk].copy(), "n_cand": nc, "cand": A["cand"][:nc].copy()}


def make_graph_problem(pose, fixed, edge_i, edge_j, meas):
    pose = np.ascontiguousarray(pose, np.float64).reshape(-1, 8).copy(); fixed = np.ascontiguousarray(fixed, np.uint8)
    ei = np.ascontiguousarray(edge_i, np.int32); ej = np.ascontiguousarray(edge_j, np.int32); meas = np.ascontiguousarray(meas, np.float64).reshape(-1, 8)
    assert len(fixed) == len(pose) and len(ei) == len(ej) == len(meas)
    p = TsloopGraphProblem()
    p.n_kf = len(pose); p.n_edge = len(ei)
    p.pose = pose.ctypes.data_as(C.POINTER(C.c_double)); p.fixed = fixed.ctypes.data_as(C.POINTER(C.c_uint8))
    p.edge_i = ei.ctypes.data_as(C.POINTER(C.c_int32)); p.edge_j = ej.ctypes.data_as(C.POINTER(C.c_int32)); p.meas = meas.ctypes.data_as(C.POINTER(C.c_double))
    return p, (fixed, ei, ej, meas), pose


class LoopError(RuntimeError):
    pass


def make_sim3_problem(P1, P2, uv1, uv2, inliers, sim, K):
    """Packs numpy arrays into the ABI struct; returns (struct, keep-alive tuple, inlier array)."""
    P1 = np.ascontiguousarray(P1, np.float64).reshape(-1, 3); P2 = np.ascontiguousarray(P2, np.float64).reshape(-1, 3)
    uv1 = np.ascontiguousarray(uv1, np.float32).reshape(-1, 2); uv2 = np.ascontiguousarray(uv2, np.float32).reshape(-1, 2)
    inl = np.ascontiguousarray(inliers, np.uint8).copy()
    assert len(P1) == len(P2) == len(uv1) == len(uv2) == len(inl)          # assert((int)vFeat1.size()==(int)vFeat2.size()), optimizer.cc:655
    p = TsloopSim3Problem()
    p.n = len(P1)
    p.P1 = P1.ctypes.data_as(C.POINTER(C.c_double)); p.P2 = P2.ctypes.data_as(C.POINTER(C.c_double))
    p.uv1 = uv1.ctypes.data_as(C.POINTER(C.c_float)); p.uv2 = uv2.ctypes.data_as(C.POINTER(C.c_float))
    p.inlier = inl.ctypes.data_as(C.POINTER(C.c_uint8))
    for k in range(4): p.K[k] = float(K[k])
    for k in range(8): p.sim[k] = float(sim[k])
    return p, (P1, P2, uv1, uv2), inl


def report_dict(r):
    return {k: getattr(r, k) for k, _ in TsloopReport._fields_}


class LoopOptimizer:
    def __init__(self, device: int = 0):
        if not os.path.exists(_LIBPATH):
            raise LoopError("libtsloop.so is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950); there is no CPU fallback")
        L = self.lib = C.CDLL(_LIBPATH)
        L.tsloop_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        L.tsloop_destroy.argtypes = [C.c_void_p]; L.tsloop_destroy.restype = None
        L.tsloop_last_error.argtypes = [C.c_void_p]; L.tsloop_last_error.restype = C.c_char_p
        L.tsloop_default_options_sim3.argtypes = [C.POINTER(TsloopOptions)]; L.tsloop_default_options_sim3.restype = None
        L.tsloop_optimize_sim3.argtypes = [C.c_void_p, C.POINTER(TsloopSim3Problem), C.POINTER(TsloopOptions), C.POINTER(TsloopReport)]
        L.tsloop_default_options_loop.argtypes = [C.POINTER(TsloopOptions)]; L.tsloop_default_options_loop.restype = None
        L.tsloop_optimize_loop.argtypes = [C.c_void_p, C.POINTER(TsloopGraphProblem), C.POINTER(TsloopOptions), C.POINTER(TsloopReport)]
        L.tsloop_default_options_sim3_ransac.argtypes = [C.POINTER(TsloopSim3BatchProblem)]; L.tsloop_default_options_sim3_ransac.restype = None
        L.tsloop_sim3_batch.argtypes = [C.c_void_p, C.POINTER(TsloopSim3BatchProblem), C.POINTER(TsloopOptions)]; L.tsloop_sim3_batch.restype = C.c_int
        L.tsloop_default_options_detect.argtypes = [C.POINTER(TsloopDetectProblem)]; L.tsloop_default_options_detect.restype = None
        L.tsloop_detect_loop.argtypes = [C.c_void_p, C.POINTER(TsloopDetectProblem)]; L.tsloop_detect_loop.restype = C.c_int
        self.ctx = C.c_void_p()
        rc = L.tsloop_create(device, C.byref(self.ctx))
        if rc != 0:
            raise LoopError("tsloop_create failed (%d): no usable GPU %d" % (rc, device))

    def __del__(self):
        if getattr(self, "ctx", None) and self.ctx:
            self.lib.tsloop_destroy(self.ctx); self.ctx = None

    def default_options_sim3(self):
        o = TsloopOptions(); self.lib.tsloop_default_options_sim3(C.byref(o)); return o

    def OptimizeSim3(self, P1, uv1, P2, uv2, vbInliers, Sim12, K, options=None):
        """vFeat1 = (posObv P1, obv2d uv1), vFeat2 = (P2, uv2); Sim12 = (qw, qx, qy, qz, t, s).
        Returns (numInlier, Sim12 [8], vbInliers, report) -- the reference updates Sim12 / vbInliers in place and returns the count."""
        o = options or self.default_options_sim3()
        p, keep, inl = make_sim3_problem(P1, P2, uv1, uv2, vbInliers, Sim12, K)
        r = TsloopReport()
        rc = self.lib.tsloop_optimize_sim3(self.ctx, C.byref(p), C.byref(o), C.byref(r))
        if rc not in (0, -3):
            raise LoopError("tsloop_optimize_sim3 failed (%d): %s" % (rc, self.lib.tsloop_last_error(self.ctx).decode()))
        rep = report_dict(r); rep["status"] = rc
        return r.n_inlier, np.array(list(p.sim)), inl.astype(bool), rep

    def Sim3Batch(self, cands, K1, K, optimise=True, min_inliers=None, max_err2=None, options=None):
        """loopClosing::ComputeSim3's Sim3Solver + OptimizeSim3 for every candidate in one launch.  cands: per candidate a dict(P1, P2 (posObv), pred1, pred2
        (obv2dPred), uv1, uv2 (obv2d.pt), triples [H, 3] (the caller's draws), K2 [4]).  Returns one dict per candidate: ok, sel, n_inlier_ransac, sim_ransac [8],
        inlier [n] bool, hyp_count [H], hyp_sim [H, 8], and for an ok candidate with optimise sim [8] and report (else None)."""
        o = options or self.default_options_sim3()
        d = TsloopSim3BatchProblem(); self.lib.tsloop_default_options_sim3_ransac(C.byref(d))
        p, A = make_sim3_batch_problem(cands, K1, K, optimise, d.min_inliers if min_inliers is None else min_inliers, d.max_err2 if max_err2 is None else max_err2)
        rc = self.lib.tsloop_sim3_batch(self.ctx, C.byref(p), C.byref(o))
        if rc not in (0, -3):
            raise LoopError("tsloop_sim3_batch failed (%d): %s" % (rc, self.lib.tsloop_last_error(self.ctx).decode()))
        out = []
        for k in range(len(cands)):
            a, b, ha, hb = int(A["off"][k]), int(A["off"][k + 1]), int(A["hyp_off"][k]), int(A["hyp_off"][k + 1])
            done = bool(A["ok"][k]) and bool(optimise)
            rep = None
            if done:
                rep = report_dict(A["rep"][k]); rep["status"] = -3 if rep["termination"] == 5 else 0
            out.append({"ok": bool(A["ok"][k]), "sel": int(A["sel"][k]), "n_inlier_ransac": int(A["n_inlier_ransac"][k]), "sim_ransac": A["sim_ransac"][k].copy(),
                        "inlier": A["inlier"][a:b].astype(bool), "hyp_count": A["hyp_count"][ha:hb].copy(), "hyp_sim": A["hyp_sim"][ha:hb].copy(),
                        "sim": A["sim"][k].copy() if done else None, "report": rep})
        return out

    def DetectLoop(self, queries, q_self, map_texts, m_skip, obs_rows, n_kf, min_matched_words=1, score_thresh_min=None, min_str_score=None, top_n=None,
                   max_match=None):
        """loopClosing::DetectLoop's scan, lists, vote and candidates in one call (make_detect_problem names the arguments; None = the library's default).
        Returns detect_result's dict plus "status": 0, or -1 when a query has more matches than max_match -- then match_cnt, kf_score, kf_nobj, n_cand and cand
        are complete and that query's lists are None (call again with max_match = match_cnt.max())."""
        d = TsloopDetectProblem(); self.lib.tsloop_default_options_detect(C.byref(d))
        p, A = make_detect_problem(queries, q_self, map_texts, m_skip, obs_rows, n_kf, min_matched_words,
                                   d.score_thresh_min if score_thresh_min is None else score_thresh_min, d.min_str_score if min_str_score is None else min_str_score,
                                   d.top_n if top_n is None else top_n, d.max_match if max_match is None else max_match)
        A["match_cnt"][:] = 0
        rc = self.lib.tsloop_detect_loop(self.ctx, C.byref(p))
        if rc != 0 and not (rc == -1 and p.n_query > 0 and int(A["match_cnt"][:p.n_query].max()) > p.max_match):
            raise LoopError("tsloop_detect_loop failed (%d): %s" % (rc, self.lib.tsloop_last_error(self.ctx).decode()))
        out = detect_result(p, A); out["status"] = rc
        return out

    def default_options_loop(self):
        o = TsloopOptions(); self.lib.tsloop_default_options_loop(C.byref(o)); return o

    def OptimizeLoop(self, pose, fixed, edge_i, edge_j, meas, options=None):
        """Sim3 pose graph: pose [n_kf, 8] initial (q | t | s), fixed [n_kf], connections (edge_i, edge_j, meas = Sji).
        Returns (corrected poses [n_kf, 8], report)."""
        o = options or self.default_options_loop()
        p, keep, x = make_graph_problem(pose, fixed, edge_i, edge_j, meas)
        r = TsloopReport()
        rc = self.lib.tsloop_optimize_loop(self.ctx, C.byref(p), C.byref(o), C.byref(r))
        if rc not in (0, -3):
            raise LoopError("tsloop_optimize_loop failed (%d): %s" % (rc, self.lib.tsloop_last_error(self.ctx).decode()))
        rep = report_dict(r); rep["status"] = rc
        return x, rep
