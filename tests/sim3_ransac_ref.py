"""numpy restatement of the reference's Sim3Solver as loopClosing::ComputeSim3 drives it (src/Sim3Solver.cc:59-253, docs/sim3solver_recalled.md):
Horn's closed-form Sim3 of three matches per hypothesis, the two-way projection test of every match, the selection loop of iterate(), the caller-side
hypothesis-count rule and index draws -- and the synthetic world the tests of tsloop_sim3_batch run on.  np.linalg.eigh stands where the reference calls
Eigen::EigenSolver and the device a cyclic Jacobi iteration: the three agree up to the sign of the eigenvector and rounding."""
import math
import numpy as np

from textslam_amd import synth

MIN_INLIERS = 20
MAX_ERR2 = 45.0
MAX_HYP = 64


# ------------------------------------------------------------------------------------------------ one hypothesis (ComputeSim3, :124-193)
def quat_to_R(q):
    w, x, y, z = q
    return np.array([[1 - 2*(y*y + z*z), 2*(x*y - w*z), 2*(x*z + w*y)], [2*(x*y + w*z), 1 - 2*(x*x + z*z), 2*(y*z - w*x)], [2*(x*z - w*y), 2*(y*z + w*x), 1 - 2*(x*x + y*y)]])


def horn_N(P1, P2):
    """P1, P2: [3 points][3].  Returns (N 4x4, O1, O2, Pr1, Pr2) with the points as COLUMNS of Pr1 / Pr2, as the reference holds them."""
    A1 = np.asarray(P1, np.float64).T; A2 = np.asarray(P2, np.float64).T
    O1 = A1.sum(1)/3.0; O2 = A2.sum(1)/3.0
    Pr1 = A1 - O1[:, None]; Pr2 = A2 - O2[:, None]
    M = Pr2 @ Pr1.T
    N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                  [M[1, 2] - M[2, 1], M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                  [M[2, 0] - M[0, 2], M[0, 1] + M[1, 0], -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                  [M[0, 1] - M[1, 0], M[2, 0] + M[0, 2], M[1, 2] + M[2, 1], -M[0, 0] - M[1, 1] + M[2, 2]]])
    return N, O1, O2, Pr1, Pr2


def hypothesis(P1, P2):
    """Horn 1987 from three matches.  Returns dict(q (qw >= 0), R, t, s, sim [8], T12 (3x4), T21 (3x4), gap: relative gap of N's two largest eigenvalues)."""
    with np.errstate(all="ignore"):
        N, O1, O2, Pr1, Pr2 = horn_N(P1, P2)
        w, V = np.linalg.eigh(N)
        k = int(np.argmax(w))                                  # the first maximum
        q = V[:, k]/np.linalg.norm(V[:, k])
        if q[0] < 0:
            q = -q
        R = quat_to_R(q)
        P3 = R @ Pr2
        s = (Pr1*P3).sum()/(P3*P3).sum()
        t = O1 - s*(R @ O2)
        sR = s*R; sRinv = (1.0/s)*R.T
        T12 = np.concatenate([sR, t[:, None]], 1); T21 = np.concatenate([sRinv, (-(sRinv @ t))[:, None]], 1)
        ws = np.sort(w)
        gap = (ws[3] - ws[2])/max(abs(ws[3]), abs(ws[0]), 1e-300)
    return {"q": q, "R": R, "t": t, "s": s, "sim": np.concatenate([q, t, [s]]), "T12": T12, "T21": T21, "gap": gap}


# ------------------------------------------------------------------------------------------------ Project / CheckInliers (:195-241)
def project(T, K, P):
    """K * (R P + t) with the 3x3 K, then the division: u = (fx X + cx Z) / Z."""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        X = ((T[0, 0]*P[:, 0] + T[0, 1]*P[:, 1]) + T[0, 2]*P[:, 2]) + T[0, 3]
        Y = ((T[1, 0]*P[:, 0] + T[1, 1]*P[:, 1]) + T[1, 2]*P[:, 2]) + T[1, 3]
        Z = ((T[2, 0]*P[:, 0] + T[2, 1]*P[:, 1]) + T[2, 2]*P[:, 2]) + T[2, 3]
        return np.stack([(K[0]*X + K[2]*Z)/Z, (K[1]*Y + K[3]*Z)/Z], 1)


def errors(h, P1, P2, pred1, pred2, K1, K2):
    """err1, err2 of every match: squared pixel distances formed in double, rounded to float."""
    with np.errstate(all="ignore"):
        d1 = np.asarray(pred1, np.float64).reshape(-1, 2) - project(h["T12"], K1, P2)
        d2 = project(h["T21"], K2, P1) - np.asarray(pred2, np.float64).reshape(-1, 2)
        e1 = (d1[:, 0]*d1[:, 0] + d1[:, 1]*d1[:, 1]).astype(np.float32)
        e2 = (d2[:, 0]*d2[:, 0] + d2[:, 1]*d2[:, 1]).astype(np.float32)
    return e1, e2


def inlier_mask(h, P1, P2, pred1, pred2, K1, K2, max_err2=MAX_ERR2):
    e1, e2 = errors(h, P1, P2, pred1, pred2, K1, K2)
    with np.errstate(invalid="ignore"):
        return (e1.astype(np.float64) < max_err2) & (e2.astype(np.float64) < max_err2)        # NaN compares false


# ------------------------------------------------------------------------------------------------ iterate (:59-121), called once
def select(counts, min_inliers=MIN_INLIERS):
    """Returns (sel, best, ok): `>=` lets the later of equal counts win; ok is strict."""
    best, sel = 0, -1
    for h, c in enumerate(counts):
        if c >= best:
            best, sel = int(c), h
    return sel, best, best > min_inliers


def ransac(P1, P2, pred1, pred2, triples, K1, K2, min_inliers=MIN_INLIERS, max_err2=MAX_ERR2):
    """One candidate.  Returns dict(ok, sel, n_inlier, sim [8], mask [n], counts [H], hyps [H] (hypothesis dicts), masks [H][n])."""
    P1 = np.asarray(P1, np.float64).reshape(-1, 3); P2 = np.asarray(P2, np.float64).reshape(-1, 3); n = len(P1)
    hyps, masks = [], []
    for tr in np.asarray(triples, np.int64).reshape(-1, 3):
        h = hypothesis(P1[tr], P2[tr]); hyps.append(h)
        masks.append(inlier_mask(h, P1, P2, pred1, pred2, K1, K2, max_err2))
    counts = [int(m.sum()) for m in masks]
    sel, best, ok = select(counts, min_inliers)
    return {"ok": bool(ok), "sel": sel, "n_inlier": best if sel >= 0 else 0, "sim": hyps[sel]["sim"] if sel >= 0 else np.zeros(8),
            "mask": masks[sel].copy() if ok else np.zeros(n, bool), "counts": counts, "hyps": hyps, "masks": masks}


# ------------------------------------------------------------------------------------------------ the caller's side (SetRansacParameters, :41-57; the draws, :72-90)
def n_hypotheses(N, prob=0.99, min_inliers=MIN_INLIERS, max_its=300, per_call=5):
    if N < min_inliers:
        return 0
    if N == min_inliers:
        n_it = 1
    else:
        eps = np.float32(np.float32(min_inliers)/np.float32(N))                 # float epsilon = (float)mRansacMinInliers / N
        n_it = int(math.ceil(math.log(1.0 - prob)/math.log(1.0 - float(eps)**3)))         # pow(float, int) promotes to double
    return min(per_call, max(1, min(n_it, max_its)))


def draw_triples(N, H, random_int):
    """H triples from one list of available indices that is not refilled: r = random_int(0, size - 1), take avail[r], move the last entry into slot r, pop."""
    avail = list(range(N)); out = []
    for _ in range(H):
        tr = []
        for _ in range(3):
            r = random_int(0, len(avail) - 1)
            tr.append(avail[r]); avail[r] = avail[-1]; avail.pop()
        out.append(tr)
    return np.asarray(out, np.int32).reshape(-1, 3)


class Lcg32:
    """The 32-bit linear congruential generator of tests/cxx/sim3_ransac_from_cxx.cpp (written for that driver; not the reference's DUtils::Random)."""
    def __init__(self, seed):
        self.x = seed & 0xffffffff

    def random_int(self, lo, hi):
        self.x = (self.x*1664525 + 1013904223) & 0xffffffff
        return lo + (self.x >> 8) % (hi - lo + 1)


# ------------------------------------------------------------------------------------------------ the test world
def pred_of(P, K):
    return np.stack([(K[0]*P[:, 0] + K[2]*P[:, 2])/P[:, 2], (K[1]*P[:, 1] + K[3]*P[:, 2])/P[:, 2]], 1)


def world(seed, n, bad3d, H=5, own_k2=False):
    """synth.sim3_matches(seed, n, outlier_frac=0.1) (its outliers displace uv1 only: the LM's 4-px test sees them, RANSAC does not), a fraction bad3d of P2
    replaced by fresh points of the generator's box (wrong 3D matches), the predicted pixels of the final points, and H triples of the draw scheme.
    own_k2: the candidate keyframe has intrinsics of its own (Sim3Solver takes pKF2->mK), and its predicted pixels are formed with them."""
    m = synth.sim3_matches(seed, n, outlier_frac=0.1)
    rng = np.random.default_rng(1000 + seed)
    bad = rng.random(n) < bad3d; k = int(bad.sum())
    P2 = m["P2"].copy()
    P2[bad] = np.stack([rng.uniform(-1.5, 1.5, k), rng.uniform(-1.0, 1.0, k), rng.uniform(2.5, 7.0, k)], 1)
    K = m["K"]; K2 = K*np.array([1.04, 0.97, 1.01, 0.99]) if own_k2 else K.copy()
    g = np.random.default_rng(100 + seed)
    tri = draw_triples(n, H, lambda lo, hi: lo + int(g.random()*(hi - lo + 1))) if n >= 3*H else np.zeros((0, 3), np.int32)
    return {"P1": np.ascontiguousarray(m["P1"]), "P2": P2, "pred1": pred_of(m["P1"], K), "pred2": pred_of(P2, K2), "uv1": m["uv1"], "uv2": m["uv2"],
            "K": K, "K1": K.copy(), "K2": K2, "triples": tri, "bad3d": bad}


def run_world(w, **kw):
    return ransac(w["P1"], w["P2"], w["pred1"], w["pred2"], w["triples"], w["K1"], w["K2"], **kw)


# (seed, n, bad3d, H): the smallest shapes that cross each boundary -- N = 21, 64 / 65 around a wave, 257 a block plus one, 1500 six strides, H = 5 / 64,
# ties won by the later hypothesis (2, 4, 3, 5, 12) and candidates that fail (6, 8)
CASES = [(1, 300, 0.3, 5), (2, 60, 0.2, 5), (3, 1500, 0.4, 5), (4, 21, 0.0, 5), (5, 257, 0.3, 64), (6, 40, 0.6, 5), (8, 300, 0.3, 5), (11, 64, 0.1, 5), (12, 65, 0.1, 5)]
# beside them: H = 3 and H = 1 as the caller's rule gives them for N = 21 and N = 20, and a candidate whose K2 is not K1
EXTRA = [(4, 21, 0.0, 3), (13, 20, 0.0, 1), (11, 64, 0.1, 5, True)]
# what a prototype of this recipe gave: counts (first 8), sel, ok, LM inliers from the selection (oracle)
EXPECT = {1: ([2, 3, 0, 205, 0], 3, True, 182), 2: ([43, 0, 43, 30, 43], 4, True, 37), 3: ([877, 2, 877, 718, 3], 2, True, 794), 4: ([20, 18, 21, 21, 19], 3, True, 20),
          5: ([0, 1, 11, 0, 1, 181, 0, 181], 58, True, 156), 6: ([0, 0, 2, 0, 0], 2, False, None), 8: ([0, 0, 1, 1, 0], 3, False, None),
          11: ([2, 14, 54, 27, 56], 4, True, 49), 12: ([41, 60, 60, 56, 0], 2, True, 54)}


def conditions(w, res, oracle=None):
    """The conditions of the inputs (not measurements): returns dict(err_margin, gap, lm_margin) -- relative distance of the nearest err to the threshold,
    smallest relative eigenvalue gap, and with an oracle the nearest final LM residual of an LM inlier to 4.0 px."""
    em = np.inf; gap = np.inf
    for h in res["hyps"]:
        e1, e2 = errors(h, w["P1"], w["P2"], w["pred1"], w["pred2"], w["K1"], w["K2"])
        e = np.concatenate([e1, e2]).astype(np.float64); e = e[np.isfinite(e)]
        if len(e):
            em = min(em, float(np.min(np.abs(e - MAX_ERR2)/MAX_ERR2)))
        if np.isfinite(h["gap"]):
            gap = min(gap, float(h["gap"]))
    out = {"err_margin": em, "gap": gap, "lm_margin": np.inf}
    if oracle is not None and res["ok"]:
        n, sim, inl, rep = oracle.optimize_sim3(w["P1"], w["uv1"], w["P2"], w["uv2"], res["mask"].astype(np.uint8), res["sim"], w["K"])
        out["lm"] = (n, sim, inl, rep)
        for i in np.flatnonzero(res["mask"]):
            r, _ = oracle.sim3_eval(sim, w["P1"][i], w["P2"][i], w["uv1"][i], w["uv2"][i], w["K"])
            out["lm_margin"] = min(out["lm_margin"], float(np.min(np.abs(np.abs(r) - 4.0))))
    return out
